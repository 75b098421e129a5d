"""CPU: how the likelihood kernel's chunk loop waits on memory, read off the gfx950 code object inside libspvipes_hip.so (llvm-objdump,
no GPU needed; the queue model is tests/_isa_waits.py).

csrc/spv_decoder.h: dec_nb_body keeps the loads of the following chunks in flight while a chunk is evaluated and issues them ahead of
the chunk's gradient stores.  That only pays if the compiled loop (a) never waits for the stores of the chunk just before -- vmcnt
retires in order and counts stores, a store leaves the queue when L2 acknowledges it --, (b) does not wait on vector memory at all
between a chunk's last gradient store and the next chunk's first MFMA, and (c) never copies a register a load is still writing (the
copy would wait for the load: a rotation of pipeline registers at the bottom of the loop does exactly that).  Checked for every TRAIN
instantiation of dec_nb_kernel and dec_nb_pair_kernel, over two steady-state trips of the loop's hot path."""
import os

import pytest

from tests import _isa_waits as W


@pytest.fixture(scope="module")
def nb_kernels(tmp_path_factory):
    from spvipes_amd import _abi
    from spvipes_amd.build import build

    if not os.path.exists(W.OBJDUMP):
        pytest.skip("llvm-objdump not available")
    build()
    funcs = W.disassemble(_abi.LIB_PATH, str(tmp_path_factory.mktemp("isa_nb")))
    ks = {k: v for k, v in funcs.items() if "13dec_nb_kernelILb1" in k or "18dec_nb_pair_kernelILb1" in k}   # the TRAIN instantiations
    assert sum("13dec_nb_kernel" in k for k in ks) >= 6 and sum("18dec_nb_pair_kernel" in k for k in ks) >= 6, sorted(ks)
    out = {}
    for name, ins in ks.items():
        header, back = W.find_chunk_loop(ins)
        trip = W.hot_trip(ins, header)
        mfma = sum(ins[i].op.startswith("v_mfma") for i in trip)
        stores = sum(ins[i].op.startswith("global_store") for i in trip)
        loads = sum(ins[i].op.startswith("global_load") for i in trip)
        # a trip of the hot path is whole chunks: 6 (narrow) or 15 (wide layout) MFMAs, 3 (bf16) or 6 (hi / lo planes) stores each
        assert mfma % 3 == 0 and stores % 3 == 0 and mfma >= 6 and stores >= 3 and loads >= 6, (name, mfma, stores, loads)
        out[name] = W.walk(ins, trip)
    return out


def test_no_wait_retires_the_previous_chunks_stores(nb_kernels):
    for name, events in nb_kernels.items():
        waits = [e for e in events if e["kind"] == "wait"]
        assert waits, name
        bad = [(e["ins"], r["ins"]) for e in waits for r in e["retired"] if r["kind"] == "store" and r["chunk"] == e["chunk"] - 1]
        assert not bad, f"{name}: {bad[0][0]} retires a gradient store of the chunk before ({bad[0][1]})"
        same = [(e["ins"], r["ins"]) for e in waits for r in e["retired"] if r["kind"] == "store" and r["chunk"] == e["chunk"]]
        assert not same, f"{name}: {same[0][0]} retires a gradient store of its own chunk ({same[0][1]})"


def test_no_vector_memory_wait_between_the_stores_and_the_next_mfma(nb_kernels):
    for name, events in nb_kernels.items():
        bad = [e["ins"] for e in events if e["kind"] == "wait_before_mfma"]
        assert not bad, f"{name}: {bad[0]} between a chunk's last gradient store and the next chunk's first MFMA"


def test_no_copy_of_a_register_a_load_is_still_writing(nb_kernels):
    for name, events in nb_kernels.items():
        bad = [(e["ins"], e["entry"]["ins"]) for e in events if e["kind"] == "mov_of_load"]
        assert not bad, f"{name}: {bad[0][0]} copies the destination of the load in flight {bad[0][1]}"
        # the compiler puts a wait in front of such a copy, which takes the load out of the modelled queue: so also no copy of what a
        # load of the SAME chunk fetched (every load of the loop is for a later chunk), whether a wait stands in between or not
        bad = [(e["ins"], e["load"]) for e in events if e["kind"] == "mov_of_chunk_load"]
        assert not bad, f"{name}: {bad[0][0]} copies what {bad[0][1]} fetched in the same chunk"
