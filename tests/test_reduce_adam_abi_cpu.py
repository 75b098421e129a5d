"""CPU: the ctypes mirrors of the slab-sum + Adam structs have the sizes and field offsets the C header gives (plain gcc, no GPU)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reduce_adam_structs_match_the_header(tmp_path):
    from spvipes_amd import _abi

    sizes = {"spv_adam_range": _abi.SpvAdamRange, "spv_adam_image": _abi.SpvAdamImage, "spv_reduce_adam_prob": _abi.SpvReduceAdamProb,
             "spv_reduce_adam_batch": _abi.SpvReduceAdamBatch}
    offsets = {("spv_reduce_adam_prob", f): getattr(_abi.SpvReduceAdamProb, f).offset for f in ("r", "p", "m", "v", "img")}
    offsets[("spv_reduce_adam_batch", "nprob")] = _abi.SpvReduceAdamBatch.nprob.offset
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "spvipes_hip.h")}"', "int main(void) {"]
    lines += [f'  printf("{n} %zu\\n", sizeof({n}));' for n in sizes]
    lines += [f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for s, f in offsets]
    lines += [f'  printf("SPV_MAXRA %d\\nSPV_ADAM_MAX_SKIP %d\\n", SPV_MAXRA, SPV_ADAM_MAX_SKIP);', "  return 0;", "}"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for name, cls in sizes.items():
        assert int(got[name]) == ctypes.sizeof(cls), name
    for (s, f), off in offsets.items():
        assert int(got[f"{s}.{f}"]) == off, (s, f)
    assert int(got["SPV_MAXRA"]) == _abi.SPV_MAXRA and int(got["SPV_ADAM_MAX_SKIP"]) == _abi.ADAM_MAX_SKIP
