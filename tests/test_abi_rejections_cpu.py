"""CPU: what the C-ABI entry points REJECT, and with which words (no GPU: every case returns from an argument check, ahead of the first
HIP call).  The table pins the return code and the ``spv_last_error()`` text of the fc1, 320-column GEMM, decoder and small-layer entry
points for one fault at a time -- every distinct text their checks can give before a launch, a misaligned pointer wherever the check is
a 16-byte alignment test -- and, for a few pairs of faults, WHICH of the two is reported.  The `_grouped` entry points are held to the
same: a fault in a group is reported in the words of the per-group entry point (or of the pair check), before anything is launched.

Pointers are made-up device addresses (the host code never dereferences them); the argument structs are real."""
import ctypes as C

import pytest

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
P, Q = 0x7F0000001000, 0x7F0000001008   # made-up device addresses: on a 16-byte boundary / 8 bytes off one


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def _abi():
    from spvipes_amd import _abi
    return _abi


def _struct(cls, fields):
    s = cls()
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def _array(cls, groups):
    arr = (cls * len(groups))()
    for a, fields in zip(arr, groups):
        for k, v in fields.items():
            setattr(a, k, v)
    return arr


def counts(**o):
    return C.pointer(_struct(_abi().SpvCounts, dict(dict(X=P, ld=64, rows=None, col_off=0, dtype=1), **o)))


# ---- argument sets every check accepts (the call would go on to a launch), by entry point; a case overrides one or two of them ----------
def fc1_fwd(**o):   # B 128, G 64, 2H = 256 output units; xb_all = None: the counts themselves
    return dict(dict(x=counts(), B=128, G=64, W1_hi=P, W1_lo=None, ldw=64, N1=256, bias=P, bias2=None, n_first=128, nsplit=1, splits=1, slabs=P,
                     rowsum_ws=P, h1=P, library=P, xb_all=None, ld_xb=0, library_all=None, cov=None, cov_idx=None), **o)


def fc1_fwd_split(**o):   # "fp32" mode on a resident split image: the LDS-DMA kernel's shapes (spv_enc_fc1_fwd_uses_dma says 1)
    return fc1_fwd(**dict(dict(nsplit=3, W1_lo=P, xb_all=P, ld_xb=128, library_all=P), **o))


def fc1_wgrad(**o):
    return dict(dict(x=counts(), B=64, G=96, dh_hi=P, dh_lo=None, ld_dh=256, N1=256, nsplit=1, dW=P, dW2=P, rows_first=128, ldc=96, xb=None, ld_xb=0,
                     dh_scale=P), **o)


def fc1_wgrad_split(**o):   # (spv_enc_fc1_wgrad_split_uses_dma says 1)
    return fc1_wgrad(**dict(dict(nsplit=3, dh_lo=P, xb=P, ld_xb=256, dh_scale=None), **o))


def fc1_prep(**o):
    return dict(dict(dh1=P, h1=P, B=100, N1=256, img_hi=P, img_lo=None, ld_img=256, Bp=128, part=P, db=P, db2=P, n_first=128, scale_ws=P), **o)


def fc1_bwd_group(**o):
    return dict(dict(dh1=P, h1=P, x=counts(), B=64, G=96, N1=256, n_first=128, nsplit=1, Bp=64, dh_hi=P, dh_lo=None, ld_dh=256, part=P, db=P, db2=P,
                     dW=P, dW2=P, ldc=96, xb=P, ld_xb=128, scale_ws=P), **o)


def gemm(**o):   # 128 x 320 x 64 on a tile-ordered A operand: the LDS-DMA 320-column kernel's shapes (spv_gemm_bf16_uses_dma says 1)
    return dict(dict(a_kmajor=0, A_hi=P, A_lo=None, lda=64, B_hi=P, B_lo=None, ldb=320, C=P, ldc=320, M=128, N=320, K=64, nsplit=1, splits=2,
                     slab_stride=128 * 320, a_tiles=2), **o)


def fixup(**o):
    return C.pointer(_struct(_abi().SpvGemmFixup, dict(dict(counters=P, alpha=None, dst0=P, ld0=16, n0=16, dst1=None, ld1=0, c1=0, n1=0), **o)))


def gemm_fix(**o):
    return dict(gemm(), **dict(dict(fix=fixup()), **o))


def gemm_group(**o):
    g = gemm(**o)
    return {k: g[k] for k in ("a_kmajor", "A_hi", "A_lo", "lda", "B_hi", "B_lo", "ldb", "C", "ldc", "M", "N", "K", "nsplit", "splits", "a_tiles", "slab_stride")}


def heads_wgrad(**o):
    return dict(dict(tP=P, tS=P, a_tiles=8, Aps=P, G=256, Bp=64, splits=1, slabP=P, slabS=P), **o)


def dec(**o):   # spv_dec_params with every pointer set: 128 cells x 64 genes, one split each way, narrow layout, bf16 gradient words
    ptrs = ("X", "logits", "Wps_hi", "Wps_lo", "Aps_hi", "Aps_lo", "gene_tab", "cnt_tab", "a_p", "a_s", "lse_p", "lse_s", "w_row", "part_max_p", "part_sum_p",
            "part_max_s", "part_sum_s", "rec_part", "tp_part", "ts_part", "dtheta_part", "dL", "tP", "tS")
    return dict(dict({k: P for k in ptrs}, ldx=64, rows=None, col_off=0, count_is_u16=1, B=128, G=64, Bp=128, Gp=64, n_gene_tiles=2, logits_f32=0,
                     gene_splits=1, genes_per_split=64, grads_f32=0, nb_splits=1, nb_genes_per_split=64, nb_cell_tiles=1, kslots=0), **o)


def dec_p(**o):
    return C.pointer(_struct(_abi().SpvDecParams, dec(**o)))


def dec_group(p=None, **o):
    return dict(dict(p=_struct(_abi().SpvDecParams, dec(**(p or {}))), library=P, px_r=P, Am_hi=P, Am_lo=None, Wm_hi=P, Wm_lo=None, K=64, nsplit=1, Tp=P, Ts=P,
                     dz_part=P, dw_part=P), **o)


def expected_args(**o):
    return C.pointer(_struct(_abi().SpvDecExpectedArgs, dict(dict(Am_hi=P, Am_lo=None, Wm_hi=P, Wm_lo=None, K=64, nsplit=1, genes=None, n_genes=64, what=0, out=P,
                                                                 ld_out=64, alpha=1.0, accumulate=0), **o)))


def sample_args(**o):
    return C.pointer(_struct(_abi().SpvDecSampleArgs, dict(dict(Am_hi=P, Am_lo=None, Wm_hi=P, Wm_lo=None, K=64, nsplit=1, genes=None, n_genes=64, ld_gene=1, theta=P,
                                                               cell_ids=None, key=1, sample=0, out=P, ld_out=64), **o)))


def linear(nprob=2, prob=None, probs=None, **o):   # two 24 x 16 problems on 300 rows, relu: Y is needed on the way back
    b = _struct(_abi().SpvLinearBatch, dict(dict(nprob=nprob, B=300, relu=1, drop_p=0.0, seed=0, seed_ptr=None, accumulate=0), **o))
    for i in range(max(nprob, 0) if nprob <= 8 else 0):
        fields = dict(dict(X=P, ldx=16, W=P, bias=P, Y=P, ldy=24, dY=P, lddy=24, dX=P, lddx=16, dW=P, db=P, N=24, K=16), **(prob or {}))
        if probs and i in probs:
            fields.update(probs[i])
        for k, v in fields.items():
            setattr(b.p[i], k, v)
    return C.pointer(b)


WPART = 16 * 24 * 17 * 2   # WG_SLICES * nmax * (kmax + 1) * nprob: the smallest workspace spv_linear_wgrad takes for linear()


def pending(nprob=1, **o):
    r = _struct(_abi().SpvLinearPending, dict(dict(nprob=nprob, wpart=P + (1 << 20), prob_stride=16 * 24 * 17), **{k: v for k, v in o.items() if k != "prob"}))
    for i in range(max(nprob, 0) if nprob <= 8 else 0):
        for k, v in dict(dict(dW=P, db=P, N=24, K=16), **o.get("prob", {})).items():
            setattr(r.p[i], k, v)
    return C.pointer(r)


def _call(lib, entry, args):
    """args: dict (in the entry point's parameter order; the stream is appended), list of group dicts (a `_grouped` entry point: array, count,
    [extra], stream) or tuple (passed as it is, stream appended)"""
    abi = _abi()
    group_struct = {"spv_enc_fc1_fwd_grouped": abi.SpvFc1FwdArgs, "spv_enc_fc1_bwd_grouped": abi.SpvFc1BwdArgs, "spv_gemm_bf16_grouped": abi.SpvGemmArgs}
    if isinstance(args, dict):
        argv = list(args.values())
    elif isinstance(args, list):
        groups, extra = (args[:-1], [args[-1]]) if args and isinstance(args[-1], int) else (args, [])
        argv = [_array(group_struct.get(entry, abi.SpvDecGroup), groups), len(groups)] + extra
        if entry.startswith("spv_enc_fc1"):   # (declared void* in _abi)
            argv[0] = C.cast(argv[0], C.c_void_p)
    else:
        argv = list(args)
    rc = getattr(lib, entry)(*argv, None)
    return rc, (lib.spv_last_error() or b"").decode()


DEC_BP = "decoder: Bp must be a multiple of 128 and Gp of 32"
DEC_2_30 = "decoder: Bp * Gp must stay below 2^30 elements (and Gp below 2^24)"
DEC_SPLITS = "decoder: gene splits must be multiples of 32 covering G"
DEC_OPERANDS = "decoder: missing packed regressor operands"
DEC_KSLOTS = "decoder: kslots must be 0 (16 / 32 K slots) or 1 (32 / 64)"
FWD_SPLIT_ONLY_DMA = "spv_enc_fc1_fwd: a split (nsplit 3) resident image is only taken by the LDS-DMA kernel (ask spv_enc_fc1_fwd_uses_dma)"
WGRAD_SPLIT_ONLY_DMA = "spv_enc_fc1_wgrad: a split (nsplit 3) resident image is only taken by the LDS-DMA kernel (ask spv_enc_fc1_wgrad_split_uses_dma)"
HEADS_WGRAD_SHAPE = "spv_dec_heads_wgrad: Bp must be a multiple of 64 and the tile arrays must cover round_up(G, 128) genes"
NB_SPLITS = "spv_dec_nb_fwd: nb_genes_per_split must be a multiple of 32, at most 160, and the splits must cover G"

# (case, entry point, arguments, return code, spv_last_error()) -- recorded from the library before the wrappers were rewritten around shared
# helpers; the rewrite must not change a row
CASES = [
    # ---- spv_enc_fc1_fwd ----------------------------------------------------------------------------------------------------------------
    ("fc1_fwd/null-x", "spv_enc_fc1_fwd", lambda: fc1_fwd(x=None), ERR_ARG, "spv_enc_fc1_fwd: null pointer"),
    ("fc1_fwd/null-x.X", "spv_enc_fc1_fwd", lambda: fc1_fwd(x=counts(X=None)), ERR_ARG, "spv_enc_fc1_fwd: null pointer"),
    ("fc1_fwd/null-W1_hi", "spv_enc_fc1_fwd", lambda: fc1_fwd(W1_hi=None), ERR_ARG, "spv_enc_fc1_fwd: null pointer"),
    ("fc1_fwd/null-library", "spv_enc_fc1_fwd", lambda: fc1_fwd(library=None), ERR_ARG, "spv_enc_fc1_fwd: null pointer"),
    ("fc1_fwd/cov-without-idx", "spv_enc_fc1_fwd", lambda: fc1_fwd(cov=P), ERR_ARG, "spv_enc_fc1_fwd: cov and cov_idx go together"),
    ("fc1_fwd/idx-without-cov", "spv_enc_fc1_fwd", lambda: fc1_fwd(cov_idx=P), ERR_ARG, "spv_enc_fc1_fwd: cov and cov_idx go together"),
    ("fc1_fwd/B-0", "spv_enc_fc1_fwd", lambda: fc1_fwd(B=0), ERR_ARG, "spv_enc_fc1_fwd: bad shape"),
    ("fc1_fwd/ldw-odd", "spv_enc_fc1_fwd", lambda: fc1_fwd(ldw=72), ERR_ARG, "spv_enc_fc1_fwd: bad shape"),
    ("fc1_fwd/ldw-short", "spv_enc_fc1_fwd", lambda: fc1_fwd(G=65), ERR_ARG, "spv_enc_fc1_fwd: bad shape"),
    ("fc1_fwd/nsplit-2", "spv_enc_fc1_fwd", lambda: fc1_fwd(nsplit=2), ERR_ARG, "spv_enc_fc1_fwd: nsplit must be 1 or 3"),
    ("fc1_fwd/nsplit-3-no-lo", "spv_enc_fc1_fwd", lambda: fc1_fwd(nsplit=3), ERR_ARG, "spv_enc_fc1_fwd: nsplit=3 needs W1_lo"),
    ("fc1_fwd/xb-no-library_all", "spv_enc_fc1_fwd", lambda: fc1_fwd(xb_all=P, ld_xb=64), ERR_ARG, "spv_enc_fc1_fwd: xb_all needs library_all and ld_xb >= round_up(G, 32)"),
    ("fc1_fwd/xb-ld-odd", "spv_enc_fc1_fwd", lambda: fc1_fwd(xb_all=P, ld_xb=68, library_all=P), ERR_ARG, "spv_enc_fc1_fwd: xb_all needs library_all and ld_xb >= round_up(G, 32)"),
    ("fc1_fwd/split-image-N1-128", "spv_enc_fc1_fwd", lambda: fc1_fwd_split(N1=128), ERR_ARG, FWD_SPLIT_ONLY_DMA),
    ("fc1_fwd/split-image-one-plane-pitch", "spv_enc_fc1_fwd", lambda: fc1_fwd_split(ld_xb=64), ERR_ARG, FWD_SPLIT_ONLY_DMA),
    ("fc1_fwd/split-misaligned-xb", "spv_enc_fc1_fwd", lambda: fc1_fwd_split(xb_all=Q), ERR_ARG, "spv_enc_fc1_fwd: images must be 16-byte aligned"),
    ("fc1_fwd/split-misaligned-W1_hi", "spv_enc_fc1_fwd", lambda: fc1_fwd_split(W1_hi=Q), ERR_ARG, "spv_enc_fc1_fwd: images must be 16-byte aligned"),
    ("fc1_fwd/split-misaligned-W1_lo", "spv_enc_fc1_fwd", lambda: fc1_fwd_split(W1_lo=Q), ERR_ARG, "spv_enc_fc1_fwd: images must be 16-byte aligned"),
    ("fc1_fwd/dtype-7", "spv_enc_fc1_fwd", lambda: fc1_fwd(x=counts(dtype=7)), ERR_ARG, "spv_enc_fc1_fwd: unknown count dtype"),
    ("fc1_fwd/2:null-and-shape", "spv_enc_fc1_fwd", lambda: fc1_fwd(bias=None, splits=0), ERR_ARG, "spv_enc_fc1_fwd: null pointer"),
    ("fc1_fwd/2:shape-and-nsplit", "spv_enc_fc1_fwd", lambda: fc1_fwd(N1=0, nsplit=2), ERR_ARG, "spv_enc_fc1_fwd: bad shape"),
    ("fc1_fwd/2:not-dma-and-misaligned", "spv_enc_fc1_fwd", lambda: fc1_fwd_split(N1=128, W1_lo=Q), ERR_ARG, FWD_SPLIT_ONLY_DMA),
    ("fc1_fwd/2:no-lo-and-misaligned", "spv_enc_fc1_fwd", lambda: fc1_fwd_split(W1_lo=None, xb_all=Q), ERR_ARG, "spv_enc_fc1_fwd: nsplit=3 needs W1_lo"),
    # ---- spv_enc_fc1_fwd_grouped --------------------------------------------------------------------------------------------------------
    ("fc1_fwd_grouped/null", "spv_enc_fc1_fwd_grouped", lambda: (None, 2), ERR_ARG, "spv_enc_fc1_fwd_grouped: bad arguments"),
    ("fc1_fwd_grouped/n-0", "spv_enc_fc1_fwd_grouped", lambda: (C.cast(_array(_abi().SpvFc1FwdArgs, [fc1_fwd()]), C.c_void_p), 0), ERR_ARG, "spv_enc_fc1_fwd_grouped: bad arguments"),
    ("fc1_fwd_grouped/first-null-W1_hi", "spv_enc_fc1_fwd_grouped", lambda: [fc1_fwd_split(W1_hi=None), fc1_fwd_split()], ERR_ARG, "spv_enc_fc1_fwd: null pointer"),
    ("fc1_fwd_grouped/first-misaligned-W1_lo", "spv_enc_fc1_fwd_grouped", lambda: [fc1_fwd_split(W1_lo=Q), fc1_fwd_split()], ERR_ARG, "spv_enc_fc1_fwd: images must be 16-byte aligned"),
    ("fc1_fwd_grouped/first-misaligned-xb", "spv_enc_fc1_fwd_grouped", lambda: [fc1_fwd_split(xb_all=Q), fc1_fwd_split()], ERR_ARG, "spv_enc_fc1_fwd: images must be 16-byte aligned"),
    ("fc1_fwd_grouped/one-group-nsplit-2", "spv_enc_fc1_fwd_grouped", lambda: [fc1_fwd(nsplit=2)], ERR_ARG, "spv_enc_fc1_fwd: nsplit must be 1 or 3"),
    ("fc1_fwd_grouped/2:first-shape-second-null", "spv_enc_fc1_fwd_grouped", lambda: [fc1_fwd_split(splits=0), fc1_fwd_split(h1=None)], ERR_ARG, "spv_enc_fc1_fwd: bad shape"),
    # ---- spv_enc_fc1_wgrad --------------------------------------------------------------------------------------------------------------
    ("fc1_wgrad/null-x", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(x=None), ERR_ARG, "spv_enc_fc1_wgrad: null pointer"),
    ("fc1_wgrad/null-dW", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(dW=None), ERR_ARG, "spv_enc_fc1_wgrad: null pointer"),
    ("fc1_wgrad/no-scale", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(dh_scale=None), ERR_ARG, "spv_enc_fc1_wgrad: nsplit=1 needs the dh image's scale record (spv_enc_fc1_bwd_prep)"),
    ("fc1_wgrad/ld_dh-short", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(ld_dh=128), ERR_ARG, "spv_enc_fc1_wgrad: bad shape"),
    ("fc1_wgrad/ldc-short", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(ldc=95), ERR_ARG, "spv_enc_fc1_wgrad: bad shape"),
    ("fc1_wgrad/nsplit-2", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(nsplit=2), ERR_ARG, "spv_enc_fc1_wgrad: nsplit must be 1 or 3"),
    ("fc1_wgrad/nsplit-3-no-lo", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(nsplit=3), ERR_ARG, "spv_enc_fc1_wgrad: nsplit=3 needs dh_lo"),
    ("fc1_wgrad/split-image-pitch", "spv_enc_fc1_wgrad", lambda: fc1_wgrad_split(ld_xb=192), ERR_ARG, WGRAD_SPLIT_ONLY_DMA),
    ("fc1_wgrad/split-image-rows_first", "spv_enc_fc1_wgrad", lambda: fc1_wgrad_split(rows_first=64), ERR_ARG, WGRAD_SPLIT_ONLY_DMA),
    ("fc1_wgrad/split-image-no-dW2", "spv_enc_fc1_wgrad", lambda: fc1_wgrad_split(dW2=None), ERR_ARG, WGRAD_SPLIT_ONLY_DMA),
    ("fc1_wgrad/split-misaligned-xb", "spv_enc_fc1_wgrad", lambda: fc1_wgrad_split(xb=Q), ERR_ARG, WGRAD_SPLIT_ONLY_DMA),
    ("fc1_wgrad/split-misaligned-dh_hi", "spv_enc_fc1_wgrad", lambda: fc1_wgrad_split(dh_hi=Q), ERR_ARG, WGRAD_SPLIT_ONLY_DMA),
    ("fc1_wgrad/split-misaligned-dh_lo", "spv_enc_fc1_wgrad", lambda: fc1_wgrad_split(dh_lo=Q), ERR_ARG, WGRAD_SPLIT_ONLY_DMA),
    ("fc1_wgrad/xb-ld-short", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(xb=P, ld_xb=96), ERR_ARG, "spv_enc_fc1_wgrad: xb needs nsplit 1 and ld_xb >= round_up(G, 64)"),
    ("fc1_wgrad/xb-ld-odd", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(xb=P, ld_xb=132), ERR_ARG, "spv_enc_fc1_wgrad: xb needs nsplit 1 and ld_xb >= round_up(G, 64)"),
    ("fc1_wgrad/dtype-7", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(x=counts(dtype=7)), ERR_ARG, "spv_enc_fc1_wgrad: unknown count dtype"),
    ("fc1_wgrad/2:null-and-shape", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(dh_hi=None, G=0), ERR_ARG, "spv_enc_fc1_wgrad: null pointer"),
    ("fc1_wgrad/2:no-scale-and-shape", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(dh_scale=None, B=0), ERR_ARG, "spv_enc_fc1_wgrad: nsplit=1 needs the dh image's scale record (spv_enc_fc1_bwd_prep)"),
    ("fc1_wgrad/2:shape-and-nsplit", "spv_enc_fc1_wgrad", lambda: fc1_wgrad(ld_dh=260, nsplit=0), ERR_ARG, "spv_enc_fc1_wgrad: bad shape"),
    # ---- spv_enc_fc1_bwd_prep -----------------------------------------------------------------------------------------------------------
    ("fc1_prep/null-dh1", "spv_enc_fc1_bwd_prep", lambda: fc1_prep(dh1=None), ERR_ARG, "spv_enc_fc1_bwd_prep: null pointer"),
    ("fc1_prep/null-db", "spv_enc_fc1_bwd_prep", lambda: fc1_prep(db=None), ERR_ARG, "spv_enc_fc1_bwd_prep: null pointer"),
    ("fc1_prep/Bp-short", "spv_enc_fc1_bwd_prep", lambda: fc1_prep(Bp=64), ERR_ARG, "spv_enc_fc1_bwd_prep: bad shape (Bp a multiple of 64)"),
    ("fc1_prep/Bp-odd", "spv_enc_fc1_bwd_prep", lambda: fc1_prep(Bp=112), ERR_ARG, "spv_enc_fc1_bwd_prep: bad shape (Bp a multiple of 64)"),
    ("fc1_prep/ld_img-short", "spv_enc_fc1_bwd_prep", lambda: fc1_prep(ld_img=255), ERR_ARG, "spv_enc_fc1_bwd_prep: bad shape (Bp a multiple of 64)"),
    ("fc1_prep/f16-no-scale_ws", "spv_enc_fc1_bwd_prep", lambda: fc1_prep(scale_ws=None), ERR_ARG, "spv_enc_fc1_bwd_prep: the f16 image (img_lo == NULL) needs scale_ws [2 + Bp / 16]"),
    ("fc1_prep/too-large", "spv_enc_fc1_bwd_prep", lambda: fc1_prep(Bp=64 * 16385), ERR_ARG, "spv_enc_fc1_bwd_prep: minibatch too large"),
    ("fc1_prep/2:null-and-shape", "spv_enc_fc1_bwd_prep", lambda: fc1_prep(part=None, N1=0), ERR_ARG, "spv_enc_fc1_bwd_prep: null pointer"),
    ("fc1_prep/2:shape-and-scale_ws", "spv_enc_fc1_bwd_prep", lambda: fc1_prep(B=0, scale_ws=None), ERR_ARG, "spv_enc_fc1_bwd_prep: bad shape (Bp a multiple of 64)"),
    # ---- spv_enc_fc1_bwd_grouped --------------------------------------------------------------------------------------------------------
    ("fc1_bwd_grouped/null", "spv_enc_fc1_bwd_grouped", lambda: (None, 2), ERR_ARG, "spv_enc_fc1_bwd_grouped: bad arguments"),
    ("fc1_bwd_grouped/n-negative", "spv_enc_fc1_bwd_grouped", lambda: (C.cast(_array(_abi().SpvFc1BwdArgs, [fc1_bwd_group()]), C.c_void_p), -1), ERR_ARG, "spv_enc_fc1_bwd_grouped: bad arguments"),
    ("fc1_bwd_grouped/first-null-dh1", "spv_enc_fc1_bwd_grouped", lambda: [fc1_bwd_group(dh1=None), fc1_bwd_group()], ERR_ARG, "spv_enc_fc1_bwd_prep: null pointer"),
    ("fc1_bwd_grouped/first-Bp-odd", "spv_enc_fc1_bwd_grouped", lambda: [fc1_bwd_group(Bp=96), fc1_bwd_group()], ERR_ARG, "spv_enc_fc1_bwd_prep: bad shape (Bp a multiple of 64)"),
    ("fc1_bwd_grouped/one-group-no-scale_ws", "spv_enc_fc1_bwd_grouped", lambda: [fc1_bwd_group(scale_ws=None)], ERR_ARG, "spv_enc_fc1_bwd_prep: the f16 image (img_lo == NULL) needs scale_ws [2 + Bp / 16]"),
    ("fc1_bwd_grouped/2:first-misaligned-and-Bp-short", "spv_enc_fc1_bwd_grouped", lambda: [fc1_bwd_group(xb=Q, Bp=0), fc1_bwd_group()], ERR_ARG, "spv_enc_fc1_bwd_prep: bad shape (Bp a multiple of 64)"),
    # ---- spv_gemm_bf16_fix --------------------------------------------------------------------------------------------------------------
    ("gemm_fix/null-A", "spv_gemm_bf16_fix", lambda: gemm_fix(A_hi=None), ERR_ARG, "spv_gemm_bf16: null pointer"),
    ("gemm_fix/null-C", "spv_gemm_bf16_fix", lambda: gemm_fix(C=None, fix=None), ERR_ARG, "spv_gemm_bf16: null pointer"),
    ("gemm_fix/not-dma-N-32", "spv_gemm_bf16_fix", lambda: gemm_fix(N=32), ERR_UNSUPPORTED, "spv_gemm_bf16_fix: only the LDS-DMA 320-column kernels sum their slabs in the launch"),
    ("gemm_fix/not-dma-plain-A", "spv_gemm_bf16_fix", lambda: gemm_fix(a_tiles=0), ERR_UNSUPPORTED, "spv_gemm_bf16_fix: only the LDS-DMA 320-column kernels sum their slabs in the launch"),
    ("gemm_fix/no-counters", "spv_gemm_bf16_fix", lambda: gemm_fix(fix=fixup(counters=None)), ERR_ARG, "spv_gemm_bf16_fix: bad fix-up description"),
    ("gemm_fix/n0-wide", "spv_gemm_bf16_fix", lambda: gemm_fix(fix=fixup(n0=321, ld0=321)), ERR_ARG, "spv_gemm_bf16_fix: bad fix-up description"),
    ("gemm_fix/ldc-odd", "spv_gemm_bf16_fix", lambda: gemm_fix(ldc=322), ERR_ARG, "spv_gemm_bf16_fix: bad fix-up description"),
    ("gemm_fix/second-range-overlaps", "spv_gemm_bf16_fix", lambda: gemm_fix(fix=fixup(dst1=P, ld1=32, c1=8, n1=32)), ERR_ARG, "spv_gemm_bf16_fix: bad fix-up description"),
    ("gemm_fix/misaligned-C", "spv_gemm_bf16_fix", lambda: gemm_fix(C=Q), ERR_ARG, "spv_gemm_bf16_fix: bad fix-up description"),
    ("gemm_fix/misaligned-A_hi", "spv_gemm_bf16_fix", lambda: gemm_fix(A_hi=Q), ERR_ARG, "spv_gemm_bf16_fix: operand planes must be 16-byte aligned"),
    ("gemm_fix/misaligned-B_hi", "spv_gemm_bf16_fix", lambda: gemm_fix(B_hi=Q), ERR_ARG, "spv_gemm_bf16_fix: operand planes must be 16-byte aligned"),
    ("gemm_fix/nsplit-3-misaligned-A_lo", "spv_gemm_bf16_fix", lambda: gemm_fix(nsplit=3, A_lo=Q, B_lo=P), ERR_ARG, "spv_gemm_bf16_fix: operand planes must be 16-byte aligned"),
    ("gemm_fix/nsplit-3-misaligned-B_lo", "spv_gemm_bf16_fix", lambda: gemm_fix(nsplit=3, A_lo=P, B_lo=Q), ERR_ARG, "spv_gemm_bf16_fix: operand planes must be 16-byte aligned"),
    ("gemm_fix/M-0", "spv_gemm_bf16_fix", lambda: gemm_fix(M=0, fix=None), ERR_ARG, "spv_gemm_bf16: bad shape"),
    ("gemm_fix/lda-odd", "spv_gemm_bf16_fix", lambda: gemm_fix(a_tiles=0, lda=68, fix=None), ERR_ARG, "spv_gemm_bf16: bad shape"),
    ("gemm_fix/nsplit-2", "spv_gemm_bf16_fix", lambda: gemm_fix(nsplit=2, fix=None), ERR_ARG, "spv_gemm_bf16: nsplit must be 1 or 3"),
    ("gemm_fix/nsplit-3-no-lo", "spv_gemm_bf16_fix", lambda: gemm_fix(nsplit=3, A_lo=P, fix=None), ERR_ARG, "spv_gemm_bf16: nsplit=3 needs lo images"),
    ("gemm_fix/B-narrow", "spv_gemm_bf16_fix", lambda: gemm_fix(N=40, ldb=64, fix=None), ERR_ARG, "spv_gemm_bf16: B image narrower than the N tiling"),
    ("gemm_fix/2:null-and-shape", "spv_gemm_bf16_fix", lambda: gemm_fix(B_hi=None, K=0), ERR_ARG, "spv_gemm_bf16: null pointer"),
    ("gemm_fix/2:not-dma-and-bad-fix", "spv_gemm_bf16_fix", lambda: gemm_fix(M=0, fix=fixup(dst0=None)), ERR_UNSUPPORTED, "spv_gemm_bf16_fix: only the LDS-DMA 320-column kernels sum their slabs in the launch"),
    ("gemm_fix/2:misaligned-C-and-A", "spv_gemm_bf16_fix", lambda: gemm_fix(C=Q, A_hi=Q), ERR_ARG, "spv_gemm_bf16_fix: bad fix-up description"),
    ("gemm_fix/2:misaligned-A-and-splits-0", "spv_gemm_bf16_fix", lambda: gemm_fix(A_hi=Q, splits=0), ERR_ARG, "spv_gemm_bf16_fix: operand planes must be 16-byte aligned"),
    ("gemm_fix/2:nsplit-2-with-fix", "spv_gemm_bf16_fix", lambda: gemm_fix(nsplit=2), ERR_UNSUPPORTED, "spv_gemm_bf16_fix: only the LDS-DMA 320-column kernels sum their slabs in the launch"),
    # ---- spv_gemm_bf16_grouped ----------------------------------------------------------------------------------------------------------
    ("gemm_grouped/null", "spv_gemm_bf16_grouped", lambda: (None, 2), ERR_ARG, "spv_gemm_bf16_grouped: bad arguments"),
    ("gemm_grouped/n-0", "spv_gemm_bf16_grouped", lambda: (_array(_abi().SpvGemmArgs, [gemm_group()]), 0), ERR_ARG, "spv_gemm_bf16_grouped: bad arguments"),
    ("gemm_grouped/first-null-A", "spv_gemm_bf16_grouped", lambda: [gemm_group(A_hi=None), gemm_group()], ERR_ARG, "spv_gemm_bf16: null pointer"),
    ("gemm_grouped/first-K-0", "spv_gemm_bf16_grouped", lambda: [gemm_group(K=0), gemm_group()], ERR_ARG, "spv_gemm_bf16: bad shape"),
    ("gemm_grouped/first-nsplit-3-no-lo", "spv_gemm_bf16_grouped", lambda: [gemm_group(nsplit=3), gemm_group()], ERR_ARG, "spv_gemm_bf16: nsplit=3 needs lo images"),
    ("gemm_grouped/2:first-misaligned-and-narrow-B", "spv_gemm_bf16_grouped", lambda: [gemm_group(A_hi=Q, ldb=64), gemm_group()], ERR_ARG, "spv_gemm_bf16: B image narrower than the N tiling"),
    # ---- spv_dec_heads_wgrad ------------------------------------------------------------------------------------------------------------
    ("heads_wgrad/null-tP", "spv_dec_heads_wgrad", lambda: heads_wgrad(tP=None), ERR_ARG, "spv_dec_heads_wgrad: null pointer"),
    ("heads_wgrad/null-slabS", "spv_dec_heads_wgrad", lambda: heads_wgrad(slabS=None), ERR_ARG, "spv_dec_heads_wgrad: null pointer"),
    ("heads_wgrad/Bp-odd", "spv_dec_heads_wgrad", lambda: heads_wgrad(Bp=96), ERR_ARG, HEADS_WGRAD_SHAPE),
    ("heads_wgrad/tiles-short", "spv_dec_heads_wgrad", lambda: heads_wgrad(G=257), ERR_ARG, HEADS_WGRAD_SHAPE),
    ("heads_wgrad/misaligned-tP", "spv_dec_heads_wgrad", lambda: heads_wgrad(tP=Q), ERR_ARG, "spv_dec_heads_wgrad: operands must be 16-byte aligned"),
    ("heads_wgrad/misaligned-tS", "spv_dec_heads_wgrad", lambda: heads_wgrad(tS=Q), ERR_ARG, "spv_dec_heads_wgrad: operands must be 16-byte aligned"),
    ("heads_wgrad/misaligned-Aps", "spv_dec_heads_wgrad", lambda: heads_wgrad(Aps=Q), ERR_ARG, "spv_dec_heads_wgrad: operands must be 16-byte aligned"),
    ("heads_wgrad/2:null-and-misaligned", "spv_dec_heads_wgrad", lambda: heads_wgrad(Aps=None, tS=Q), ERR_ARG, "spv_dec_heads_wgrad: null pointer"),
    ("heads_wgrad/2:shape-and-misaligned", "spv_dec_heads_wgrad", lambda: heads_wgrad(splits=0, tP=Q), ERR_ARG, HEADS_WGRAD_SHAPE),
    # ---- spv_dec_tables_grouped ---------------------------------------------------------------------------------------------------------
    ("tables_grouped/null", "spv_dec_tables_grouped", lambda: (None, 2), ERR_ARG, "spv_dec_tables_grouped: bad arguments"),
    ("tables_grouped/n-0", "spv_dec_tables_grouped", lambda: (_array(_abi().SpvDecGroup, [dec_group()]), 0), ERR_ARG, "spv_dec_tables_grouped: bad arguments"),
    ("tables_grouped/pair-null-px_r", "spv_dec_tables_grouped", lambda: [dec_group(), dec_group(px_r=None)], ERR_ARG, "spv_dec_tables_grouped: bad arguments"),
    ("tables_grouped/pair-Gp-short", "spv_dec_tables_grouped", lambda: [dec_group(p=dict(Gp=32)), dec_group()], ERR_ARG, "spv_dec_tables_grouped: bad arguments"),
    ("tables_grouped/one-group-null-cnt_tab", "spv_dec_tables_grouped", lambda: [dec_group(p=dict(cnt_tab=None))], ERR_ARG, "spv_dec_tables: bad arguments"),
    # ---- spv_dec_logits_grouped ---------------------------------------------------------------------------------------------------------
    ("logits_grouped/null", "spv_dec_logits_grouped", lambda: (None, 2), ERR_ARG, "spv_dec_logits_grouped: bad arguments"),
    ("logits_grouped/n-0", "spv_dec_logits_grouped", lambda: (_array(_abi().SpvDecGroup, [dec_group()]), 0), ERR_ARG, "spv_dec_logits_grouped: bad arguments"),
    ("logits_grouped/first-null-Am", "spv_dec_logits_grouped", lambda: [dec_group(Am_hi=None, p=dict(Gp=256)), dec_group(p=dict(Gp=256))], ERR_ARG, "spv_dec_logits: null pointer"),
    ("logits_grouped/first-null-out", "spv_dec_logits_grouped", lambda: [dec_group(p=dict(Gp=256, logits=None)), dec_group(p=dict(Gp=256))], ERR_ARG, "spv_dec_logits: null pointer"),
    ("logits_grouped/first-K-33", "spv_dec_logits_grouped", lambda: [dec_group(K=33, p=dict(Gp=256)), dec_group(p=dict(Gp=256))], ERR_ARG, "spv_dec_logits: bad shape"),
    ("logits_grouped/first-Gp-64", "spv_dec_logits_grouped", lambda: [dec_group(), dec_group(p=dict(Gp=256))], ERR_ARG, "spv_dec_logits: bad shape"),
    ("logits_grouped/first-nsplit-2", "spv_dec_logits_grouped", lambda: [dec_group(nsplit=2, p=dict(Gp=256)), dec_group(p=dict(Gp=256))], ERR_ARG, "spv_dec_logits: nsplit must be 1 or 3"),
    ("logits_grouped/first-nsplit-3-no-lo", "spv_dec_logits_grouped", lambda: [dec_group(nsplit=3, p=dict(Gp=256)), dec_group(p=dict(Gp=256))], ERR_ARG, "spv_dec_logits: nsplit=3 needs lo images"),
    ("logits_grouped/2:first-misaligned-and-K-0", "spv_dec_logits_grouped", lambda: [dec_group(Am_hi=Q, K=0, p=dict(Gp=256)), dec_group(p=dict(Gp=256))], ERR_ARG, "spv_dec_logits: bad shape"),
    # ---- spv_dec_lse, spv_dec_lse_grouped -----------------------------------------------------------------------------------------------
    ("lse/null-params", "spv_dec_lse", lambda: (None, P), ERR_ARG, "decoder: null params"),
    ("lse/zeroed-params", "spv_dec_lse", lambda: (C.pointer(_abi().SpvDecParams()), P), ERR_ARG, DEC_BP),
    ("lse/Bp-odd", "spv_dec_lse", lambda: (dec_p(Bp=192), P), ERR_ARG, DEC_BP),
    ("lse/Gp-short", "spv_dec_lse", lambda: (dec_p(G=65), P), ERR_ARG, DEC_BP),
    ("lse/2^30", "spv_dec_lse", lambda: (dec_p(Bp=1 << 20, Gp=1024), P), ERR_ARG, DEC_2_30),
    ("lse/2^29-split-words", "spv_dec_lse", lambda: (dec_p(Bp=1 << 19, Gp=1024, grads_f32=1), P), ERR_ARG, DEC_2_30),
    ("lse/splits-odd", "spv_dec_lse", lambda: (dec_p(genes_per_split=48), P), ERR_ARG, DEC_SPLITS),
    ("lse/splits-short", "spv_dec_lse", lambda: (dec_p(genes_per_split=32), P), ERR_ARG, DEC_SPLITS),
    ("lse/no-Aps_lo", "spv_dec_lse", lambda: (dec_p(Aps_lo=None), P), ERR_ARG, DEC_OPERANDS),
    ("lse/kslots-2", "spv_dec_lse", lambda: (dec_p(kslots=2), P), ERR_ARG, DEC_KSLOTS),
    ("lse/null-library", "spv_dec_lse", lambda: (dec_p(), None), ERR_ARG, "spv_dec_lse: null pointer"),
    ("lse/null-part_sum_s", "spv_dec_lse", lambda: (dec_p(part_sum_s=None), P), ERR_ARG, "spv_dec_lse: null pointer"),
    ("lse/2:shape-and-null", "spv_dec_lse", lambda: (dec_p(B=0), None), ERR_ARG, DEC_BP),
    ("lse/2:splits-and-kslots", "spv_dec_lse", lambda: (dec_p(gene_splits=0, kslots=3), P), ERR_ARG, DEC_SPLITS),
    ("lse_grouped/null", "spv_dec_lse_grouped", lambda: (None, 2), ERR_ARG, "spv_dec_lse_grouped: bad arguments"),
    ("lse_grouped/n-0", "spv_dec_lse_grouped", lambda: (_array(_abi().SpvDecGroup, [dec_group()]), 0), ERR_ARG, "spv_dec_lse_grouped: bad arguments"),
    ("lse_grouped/second-null-library", "spv_dec_lse_grouped", lambda: [dec_group(), dec_group(library=None)], ERR_ARG, "spv_dec_lse: null pointer"),
    ("lse_grouped/second-kslots-2", "spv_dec_lse_grouped", lambda: [dec_group(), dec_group(p=dict(kslots=2))], ERR_ARG, DEC_KSLOTS),
    ("lse_grouped/one-group-Bp-odd", "spv_dec_lse_grouped", lambda: [dec_group(p=dict(Bp=200))], ERR_ARG, DEC_BP),
    ("lse_grouped/2:first-null-second-shape", "spv_dec_lse_grouped", lambda: [dec_group(p=dict(a_s=None)), dec_group(p=dict(Gp=48))], ERR_ARG, "spv_dec_lse: null pointer"),
    ("lse_grouped/2:layouts-differ-and-second-null", "spv_dec_lse_grouped", lambda: [dec_group(p=dict(kslots=1)), dec_group(p=dict(lse_p=None))], ERR_ARG, "spv_dec_lse: null pointer"),
    # ---- spv_dec_nb_fwd, spv_dec_nb_fwd_grouped -----------------------------------------------------------------------------------------
    ("nb/null-params", "spv_dec_nb_fwd", lambda: (None, 1), ERR_ARG, "decoder: null params"),
    ("nb/Bp-odd", "spv_dec_nb_fwd", lambda: (dec_p(Bp=130), 0), ERR_ARG, DEC_BP),
    ("nb/no-Wps_hi", "spv_dec_nb_fwd", lambda: (dec_p(Wps_hi=None), 0), ERR_ARG, DEC_OPERANDS),
    ("nb/null-X", "spv_dec_nb_fwd", lambda: (dec_p(X=None), 0), ERR_ARG, "spv_dec_nb_fwd: null pointer"),
    ("nb/null-rec_part", "spv_dec_nb_fwd", lambda: (dec_p(rec_part=None), 1), ERR_ARG, "spv_dec_nb_fwd: null pointer"),
    ("nb/gene-tiles", "spv_dec_nb_fwd", lambda: (dec_p(n_gene_tiles=3), 0), ERR_ARG, "spv_dec_nb_fwd: n_gene_tiles must be Gp / 32"),
    ("nb/nb_splits-0", "spv_dec_nb_fwd", lambda: (dec_p(nb_splits=0), 0), ERR_ARG, NB_SPLITS),
    ("nb/nb-split-odd", "spv_dec_nb_fwd", lambda: (dec_p(nb_genes_per_split=80), 0), ERR_ARG, NB_SPLITS),
    ("nb/nb-split-192", "spv_dec_nb_fwd", lambda: (dec_p(nb_genes_per_split=192), 0), ERR_ARG, NB_SPLITS),
    ("nb/nb-splits-short", "spv_dec_nb_fwd", lambda: (dec_p(nb_genes_per_split=32), 0), ERR_ARG, NB_SPLITS),
    ("nb/train-no-dL", "spv_dec_nb_fwd", lambda: (dec_p(dL=None), 1), ERR_ARG, "spv_dec_nb_fwd: training outputs missing"),
    ("nb/train-no-dtheta_part", "spv_dec_nb_fwd", lambda: (dec_p(dtheta_part=None), 1), ERR_ARG, "spv_dec_nb_fwd: training outputs missing"),
    ("nb/2:null-and-tiles", "spv_dec_nb_fwd", lambda: (dec_p(w_row=None, n_gene_tiles=0), 0), ERR_ARG, "spv_dec_nb_fwd: null pointer"),
    ("nb/2:tiles-and-splits", "spv_dec_nb_fwd", lambda: (dec_p(n_gene_tiles=1, nb_splits=-1), 0), ERR_ARG, "spv_dec_nb_fwd: n_gene_tiles must be Gp / 32"),
    ("nb/2:splits-and-training", "spv_dec_nb_fwd", lambda: (dec_p(nb_genes_per_split=0, tP=None), 1), ERR_ARG, NB_SPLITS),
    ("nb_grouped/null", "spv_dec_nb_fwd_grouped", lambda: (None, 2, 1), ERR_ARG, "spv_dec_nb_fwd_grouped: bad arguments"),
    ("nb_grouped/n-0", "spv_dec_nb_fwd_grouped", lambda: (_array(_abi().SpvDecGroup, [dec_group()]), 0, 1), ERR_ARG, "spv_dec_nb_fwd_grouped: bad arguments"),
    ("nb_grouped/second-train-no-tS", "spv_dec_nb_fwd_grouped", lambda: [dec_group(), dec_group(p=dict(tS=None)), 1], ERR_ARG, "spv_dec_nb_fwd: training outputs missing"),
    ("nb_grouped/second-gene-tiles", "spv_dec_nb_fwd_grouped", lambda: [dec_group(), dec_group(p=dict(n_gene_tiles=4)), 0], ERR_ARG, "spv_dec_nb_fwd: n_gene_tiles must be Gp / 32"),
    ("nb_grouped/one-group-null-logits", "spv_dec_nb_fwd_grouped", lambda: [dec_group(p=dict(logits=None)), 0], ERR_ARG, "spv_dec_nb_fwd: null pointer"),
    ("nb_grouped/2:first-splits-second-null", "spv_dec_nb_fwd_grouped", lambda: [dec_group(p=dict(nb_splits=0)), dec_group(p=dict(X=None)), 0], ERR_ARG, NB_SPLITS),
    ("nb_grouped/2:variants-differ-and-second-misaligned-null", "spv_dec_nb_fwd_grouped", lambda: [dec_group(p=dict(X=Q, logits_f32=1)), dec_group(p=dict(a_p=None)), 0], ERR_ARG, "spv_dec_nb_fwd: null pointer"),
    # ---- spv_dec_heads_bwd, spv_dec_heads_bwd_grouped -----------------------------------------------------------------------------------
    ("heads_bwd/null-params", "spv_dec_heads_bwd", lambda: (None, P, P, P, P), ERR_ARG, "decoder: null params"),
    ("heads_bwd/splits-odd", "spv_dec_heads_bwd", lambda: (dec_p(genes_per_split=16), P, P, P, P), ERR_ARG, DEC_SPLITS),
    ("heads_bwd/null-Tp", "spv_dec_heads_bwd", lambda: (dec_p(), None, P, P, P), ERR_ARG, "spv_dec_heads_bwd: null pointer"),
    ("heads_bwd/null-dw_part", "spv_dec_heads_bwd", lambda: (dec_p(), P, P, P, None), ERR_ARG, "spv_dec_heads_bwd: null pointer"),
    ("heads_bwd/null-tS", "spv_dec_heads_bwd", lambda: (dec_p(tS=None), P, P, P, P), ERR_ARG, "spv_dec_heads_bwd: null pointer"),
    ("heads_bwd/gene-tiles", "spv_dec_heads_bwd", lambda: (dec_p(n_gene_tiles=1), P, P, P, P), ERR_ARG, "spv_dec_heads_bwd: n_gene_tiles must be Gp / 32"),
    ("heads_bwd/wide-layout", "spv_dec_heads_bwd", lambda: (dec_p(kslots=1), P, P, P, P), ERR_UNSUPPORTED, "spv_dec_heads_bwd: narrow operand layout only (kslots = 0)"),
    ("heads_bwd/2:null-and-wide", "spv_dec_heads_bwd", lambda: (dec_p(kslots=1), P, None, P, P), ERR_ARG, "spv_dec_heads_bwd: null pointer"),
    ("heads_bwd/2:tiles-and-wide", "spv_dec_heads_bwd", lambda: (dec_p(kslots=1, n_gene_tiles=0), P, P, P, P), ERR_ARG, "spv_dec_heads_bwd: n_gene_tiles must be Gp / 32"),
    ("heads_bwd_grouped/null", "spv_dec_heads_bwd_grouped", lambda: (None, 2), ERR_ARG, "spv_dec_heads_bwd_grouped: bad arguments"),
    ("heads_bwd_grouped/n-0", "spv_dec_heads_bwd_grouped", lambda: (_array(_abi().SpvDecGroup, [dec_group()]), 0), ERR_ARG, "spv_dec_heads_bwd_grouped: bad arguments"),
    ("heads_bwd_grouped/second-null-dz_part", "spv_dec_heads_bwd_grouped", lambda: [dec_group(), dec_group(dz_part=None)], ERR_ARG, "spv_dec_heads_bwd: null pointer"),
    ("heads_bwd_grouped/second-wide", "spv_dec_heads_bwd_grouped", lambda: [dec_group(), dec_group(p=dict(kslots=1))], ERR_UNSUPPORTED, "spv_dec_heads_bwd: narrow operand layout only (kslots = 0)"),
    ("heads_bwd_grouped/one-group-gene-tiles", "spv_dec_heads_bwd_grouped", lambda: [dec_group(p=dict(n_gene_tiles=7))], ERR_ARG, "spv_dec_heads_bwd: n_gene_tiles must be Gp / 32"),
    ("heads_bwd_grouped/2:first-split-words-second-null", "spv_dec_heads_bwd_grouped", lambda: [dec_group(p=dict(grads_f32=1)), dec_group(Ts=None)], ERR_ARG, "spv_dec_heads_bwd: null pointer"),
    # ---- spv_dec_expected, spv_dec_sample -----------------------------------------------------------------------------------------------
    ("expected/null-params", "spv_dec_expected", lambda: (None, expected_args()), ERR_ARG, "decoder: null params"),
    ("expected/kslots-2", "spv_dec_expected", lambda: (dec_p(kslots=2), expected_args()), ERR_ARG, DEC_KSLOTS),
    ("expected/null-args", "spv_dec_expected", lambda: (dec_p(), None), ERR_ARG, "spv_dec_expected: null arguments"),
    ("expected/null-out", "spv_dec_expected", lambda: (dec_p(), expected_args(out=None)), ERR_ARG, "spv_dec_expected: null pointer"),
    ("expected/null-a_p", "spv_dec_expected", lambda: (dec_p(a_p=None), expected_args()), ERR_ARG, "spv_dec_expected: null pointer"),
    ("expected/K-48", "spv_dec_expected", lambda: (dec_p(), expected_args(K=48)), ERR_ARG, "spv_dec_expected: K must be a multiple of 32, at most 320"),
    ("expected/K-352", "spv_dec_expected", lambda: (dec_p(), expected_args(K=352)), ERR_ARG, "spv_dec_expected: K must be a multiple of 32, at most 320"),
    ("expected/nsplit-0", "spv_dec_expected", lambda: (dec_p(), expected_args(nsplit=0)), ERR_ARG, "spv_dec_expected: nsplit must be 1 or 3"),
    ("expected/nsplit-3-no-lo", "spv_dec_expected", lambda: (dec_p(), expected_args(nsplit=3, Am_lo=P)), ERR_ARG, "spv_dec_expected: nsplit=3 needs lo images"),
    ("expected/misaligned-Am_hi", "spv_dec_expected", lambda: (dec_p(), expected_args(Am_hi=Q)), ERR_ARG, "spv_dec_expected: operand images must be 16-byte aligned"),
    ("expected/misaligned-Wm_hi", "spv_dec_expected", lambda: (dec_p(), expected_args(Wm_hi=Q)), ERR_ARG, "spv_dec_expected: operand images must be 16-byte aligned"),
    ("expected/misaligned-Am_lo", "spv_dec_expected", lambda: (dec_p(), expected_args(nsplit=3, Am_lo=Q, Wm_lo=P)), ERR_ARG, "spv_dec_expected: operand images must be 16-byte aligned"),
    ("expected/misaligned-unused-Wm_lo", "spv_dec_expected", lambda: (dec_p(), expected_args(Wm_lo=Q)), ERR_ARG, "spv_dec_expected: operand images must be 16-byte aligned"),
    ("expected/n_genes-0", "spv_dec_expected", lambda: (dec_p(), expected_args(n_genes=0)), ERR_ARG, "spv_dec_expected: n_genes must be positive (and at most G without a gene list)"),
    ("expected/n_genes-65-no-list", "spv_dec_expected", lambda: (dec_p(), expected_args(n_genes=65, ld_out=65)), ERR_ARG, "spv_dec_expected: n_genes must be positive (and at most G without a gene list)"),
    ("expected/what-4", "spv_dec_expected", lambda: (dec_p(), expected_args(what=4)), ERR_ARG, "spv_dec_expected: what must be 0 (mixture), 1 (private), 2 (shared) or 3 (mixing weight)"),
    ("expected/ld_out-short", "spv_dec_expected", lambda: (dec_p(), expected_args(ld_out=63)), ERR_ARG, "spv_dec_expected: ld_out < n_genes"),
    ("expected/2:null-and-misaligned", "spv_dec_expected", lambda: (dec_p(), expected_args(Wm_hi=None, Am_hi=Q)), ERR_ARG, "spv_dec_expected: null pointer"),
    ("expected/2:K-and-misaligned", "spv_dec_expected", lambda: (dec_p(), expected_args(K=0, Am_hi=Q)), ERR_ARG, "spv_dec_expected: K must be a multiple of 32, at most 320"),
    ("expected/2:misaligned-and-n_genes", "spv_dec_expected", lambda: (dec_p(), expected_args(Wm_hi=Q, n_genes=-1)), ERR_ARG, "spv_dec_expected: operand images must be 16-byte aligned"),
    ("sample/null-args", "spv_dec_sample", lambda: (dec_p(), None), ERR_ARG, "spv_dec_sample: null arguments"),
    ("sample/null-Am_hi", "spv_dec_sample", lambda: (dec_p(), sample_args(Am_hi=None)), ERR_ARG, "spv_dec_sample: null pointer"),
    ("sample/K-0", "spv_dec_sample", lambda: (dec_p(), sample_args(K=0)), ERR_ARG, "spv_dec_sample: K must be a multiple of 32, at most 320"),
    ("sample/nsplit-2", "spv_dec_sample", lambda: (dec_p(), sample_args(nsplit=2)), ERR_ARG, "spv_dec_sample: nsplit must be 1 or 3"),
    ("sample/nsplit-3-no-lo", "spv_dec_sample", lambda: (dec_p(), sample_args(nsplit=3, Wm_lo=P)), ERR_ARG, "spv_dec_sample: nsplit=3 needs lo images"),
    ("sample/misaligned-Wm_hi", "spv_dec_sample", lambda: (dec_p(), sample_args(Wm_hi=Q)), ERR_ARG, "spv_dec_sample: operand images must be 16-byte aligned"),
    ("sample/misaligned-Wm_lo", "spv_dec_sample", lambda: (dec_p(), sample_args(nsplit=3, Am_lo=P, Wm_lo=Q)), ERR_ARG, "spv_dec_sample: operand images must be 16-byte aligned"),
    ("sample/n_genes-0", "spv_dec_sample", lambda: (dec_p(), sample_args(n_genes=0)), ERR_ARG, "spv_dec_sample: n_genes must be positive (and at most G without a gene list)"),
    ("sample/null-theta", "spv_dec_sample", lambda: (dec_p(), sample_args(theta=None)), ERR_ARG, "spv_dec_sample: null pointer"),
    ("sample/ld_gene-0", "spv_dec_sample", lambda: (dec_p(), sample_args(ld_gene=0)), ERR_ARG, "spv_dec_sample: ld_gene < 1"),
    ("sample/ld_out-short", "spv_dec_sample", lambda: (dec_p(), sample_args(ld_gene=2, ld_out=126)), ERR_ARG, "spv_dec_sample: ld_out < (n_genes - 1) * ld_gene + 1"),
    ("sample/2:misaligned-and-null-theta", "spv_dec_sample", lambda: (dec_p(), sample_args(Am_hi=Q, theta=None)), ERR_ARG, "spv_dec_sample: operand images must be 16-byte aligned"),
    ("sample/2:theta-and-ld_gene", "spv_dec_sample", lambda: (dec_p(), sample_args(theta=None, ld_gene=0)), ERR_ARG, "spv_dec_sample: null pointer"),
    # ---- spv_linear_dgrad, spv_linear_wgrad, spv_linear_bwd -----------------------------------------------------------------------------
    ("linear_dgrad/null-batch", "spv_linear_dgrad", lambda: (None,), ERR_ARG, "spv_linear_dgrad: bad batch"),
    ("linear_dgrad/nprob-9", "spv_linear_dgrad", lambda: (linear(nprob=9),), ERR_ARG, "spv_linear_dgrad: bad batch"),
    ("linear_dgrad/B-0", "spv_linear_dgrad", lambda: (linear(B=0),), ERR_ARG, "spv_linear_dgrad: bad batch"),
    ("linear_dgrad/drop_p-1", "spv_linear_dgrad", lambda: (linear(drop_p=1.0),), ERR_ARG, "spv_linear_dgrad: dropout probability outside [0,1)"),
    ("linear_dgrad/K-0", "spv_linear_dgrad", lambda: (linear(probs={1: dict(K=0)}),), ERR_ARG, "spv_linear_dgrad: bad problem"),
    ("linear_dgrad/null-W", "spv_linear_dgrad", lambda: (linear(probs={0: dict(W=None)}),), ERR_ARG, "spv_linear_dgrad: bad problem"),
    ("linear_dgrad/null-dX", "spv_linear_dgrad", lambda: (linear(probs={1: dict(dX=None)}),), ERR_ARG, "spv_linear_dgrad: null pointer"),
    ("linear_dgrad/relu-null-Y", "spv_linear_dgrad", lambda: (linear(prob=dict(Y=None)),), ERR_ARG, "spv_linear_dgrad: null pointer"),
    ("linear_dgrad/dropout-null-Y", "spv_linear_dgrad", lambda: (linear(relu=0, drop_p=0.5, prob=dict(Y=None)),), ERR_ARG, "spv_linear_dgrad: null pointer"),
    ("linear_dgrad/2:problem-and-null", "spv_linear_dgrad", lambda: (linear(probs={0: dict(dY=None), 1: dict(N=0)}),), ERR_ARG, "spv_linear_dgrad: bad problem"),
    ("linear_wgrad/null-batch", "spv_linear_wgrad", lambda: (None, P, WPART), ERR_ARG, "spv_linear_wgrad: bad batch"),
    ("linear_wgrad/drop_p-negative", "spv_linear_wgrad", lambda: (linear(drop_p=-0.5), P, WPART), ERR_ARG, "spv_linear_wgrad: dropout probability outside [0,1)"),
    ("linear_wgrad/N-0", "spv_linear_wgrad", lambda: (linear(probs={0: dict(N=0)}), P, WPART), ERR_ARG, "spv_linear_wgrad: bad problem"),
    ("linear_wgrad/null-dW", "spv_linear_wgrad", lambda: (linear(probs={1: dict(dW=None)}), P, WPART), ERR_ARG, "spv_linear_wgrad: null pointer"),
    ("linear_wgrad/null-X", "spv_linear_wgrad", lambda: (linear(probs={0: dict(X=None)}), P, WPART), ERR_ARG, "spv_linear_wgrad: null pointer"),
    ("linear_wgrad/relu-null-Y", "spv_linear_wgrad", lambda: (linear(probs={1: dict(Y=None)}), P, WPART), ERR_ARG, "spv_linear_wgrad: null pointer"),
    ("linear_wgrad/no-workspace", "spv_linear_wgrad", lambda: (linear(), None, WPART), ERR_ARG, "spv_linear_wgrad: workspace missing"),
    ("linear_wgrad/workspace-one-short", "spv_linear_wgrad", lambda: (linear(), P, WPART - 1), ERR_ARG, "spv_linear_wgrad: workspace too small"),
    ("linear_wgrad/2:null-and-no-workspace", "spv_linear_wgrad", lambda: (linear(prob=dict(dY=None)), None, 0), ERR_ARG, "spv_linear_wgrad: null pointer"),
    ("linear_wgrad/2:no-workspace-and-size-0", "spv_linear_wgrad", lambda: (linear(), None, 0), ERR_ARG, "spv_linear_wgrad: workspace missing"),
    ("linear_bwd/nothing", "spv_linear_bwd", lambda: (None, None, None, 0, None), ERR_ARG, "spv_linear_bwd: nothing to do"),
    ("linear_bwd/d-nprob-0", "spv_linear_bwd", lambda: (linear(nprob=0), None, None, 0, None), ERR_ARG, "spv_linear_bwd: bad batch"),
    ("linear_bwd/d-drop_p", "spv_linear_bwd", lambda: (linear(drop_p=1.5), None, None, 0, None), ERR_ARG, "spv_linear_bwd: dropout probability outside [0,1)"),
    ("linear_bwd/d-bad-problem", "spv_linear_bwd", lambda: (linear(probs={1: dict(W=None)}), None, None, 0, None), ERR_ARG, "spv_linear_bwd: bad problem"),
    ("linear_bwd/d-null-dY", "spv_linear_bwd", lambda: (linear(probs={0: dict(dY=None)}), None, None, 0, None), ERR_ARG, "spv_linear_bwd: null pointer"),
    ("linear_bwd/d-relu-null-Y", "spv_linear_bwd", lambda: (linear(prob=dict(Y=None)), linear(), P, WPART, None), ERR_ARG, "spv_linear_bwd: null pointer"),
    ("linear_bwd/w-B-negative", "spv_linear_bwd", lambda: (None, linear(B=-1), P, WPART, None), ERR_ARG, "spv_linear_bwd: bad batch"),
    ("linear_bwd/w-bad-problem", "spv_linear_bwd", lambda: (linear(), linear(probs={0: dict(K=-1)}), P, WPART, None), ERR_ARG, "spv_linear_bwd: bad problem"),
    ("linear_bwd/w-null-dW", "spv_linear_bwd", lambda: (linear(), linear(probs={1: dict(dW=None)}), P, WPART, None), ERR_ARG, "spv_linear_bwd: null pointer"),
    ("linear_bwd/w-accumulate", "spv_linear_bwd", lambda: (linear(), linear(accumulate=1), P, WPART, None), ERR_ARG, "spv_linear_bwd: accumulate belongs to the input-gradient batch"),
    ("linear_bwd/w-no-workspace", "spv_linear_bwd", lambda: (None, linear(), None, WPART, None), ERR_ARG, "spv_linear_bwd: workspace missing"),
    ("linear_bwd/w-workspace-one-short", "spv_linear_bwd", lambda: (linear(), linear(), P, WPART - 1, None), ERR_ARG, "spv_linear_bwd: workspace too small"),
    ("linear_bwd/B-differs", "spv_linear_bwd", lambda: (linear(B=299), linear(), P, WPART, None), ERR_ARG, "spv_linear_bwd: the two batches disagree in B / relu / drop_p"),
    ("linear_bwd/relu-differs", "spv_linear_bwd", lambda: (linear(relu=0), linear(), P, WPART, None), ERR_ARG, "spv_linear_bwd: the two batches disagree in B / relu / drop_p"),
    ("linear_bwd/pending-nprob-0", "spv_linear_bwd", lambda: (linear(), None, None, 0, pending(nprob=0)), ERR_ARG, "spv_linear_bwd: bad pending record"),
    ("linear_bwd/pending-null-wpart", "spv_linear_bwd", lambda: (linear(), None, None, 0, pending(wpart=None)), ERR_ARG, "spv_linear_bwd: bad pending record"),
    ("linear_bwd/pending-null-dW", "spv_linear_bwd", lambda: (linear(), None, None, 0, pending(prob=dict(dW=None))), ERR_ARG, "spv_linear_bwd: bad pending problem"),
    ("linear_bwd/pending-stride-short", "spv_linear_bwd", lambda: (linear(), None, None, 0, pending(prob_stride=16 * 24 * 17 - 1)), ERR_ARG, "spv_linear_bwd: pending problem stride too small"),
    ("linear_bwd/pending-overlaps-wpart", "spv_linear_bwd", lambda: (None, linear(), P, WPART, pending(wpart=P + 4 * (WPART - 1))), ERR_ARG, "spv_linear_bwd: wpart overlaps the pending workspace"),
    ("linear_bwd/pending-alone-bad", "spv_linear_bwd", lambda: (None, None, None, 0, pending(nprob=9)), ERR_ARG, "spv_linear_reduce_pending: bad pending record"),
    ("linear_bwd/2:d-batch-and-w-null", "spv_linear_bwd", lambda: (linear(B=0), linear(prob=dict(dW=None)), P, WPART, None), ERR_ARG, "spv_linear_bwd: bad batch"),
    ("linear_bwd/2:d-null-and-w-problem", "spv_linear_bwd", lambda: (linear(prob=dict(dX=None)), linear(prob=dict(N=0)), P, WPART, None), ERR_ARG, "spv_linear_bwd: null pointer"),
    ("linear_bwd/2:w-null-and-accumulate", "spv_linear_bwd", lambda: (None, linear(accumulate=1, prob=dict(X=None)), P, WPART, None), ERR_ARG, "spv_linear_bwd: null pointer"),
    ("linear_bwd/2:w-accumulate-and-no-workspace", "spv_linear_bwd", lambda: (None, linear(accumulate=1), None, 0, None), ERR_ARG, "spv_linear_bwd: accumulate belongs to the input-gradient batch"),
    ("linear_bwd/2:w-workspace-and-B-differs", "spv_linear_bwd", lambda: (linear(B=64), linear(), P, 1, None), ERR_ARG, "spv_linear_bwd: workspace too small"),
    ("linear_bwd/2:B-differs-and-pending", "spv_linear_bwd", lambda: (linear(B=64), linear(), P, WPART, pending(nprob=0)), ERR_ARG, "spv_linear_bwd: the two batches disagree in B / relu / drop_p"),
]


def test_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


def test_baselines_are_the_shapes_the_dma_kernels_take(lib):
    """the misaligned-pointer cases of the LDS-DMA paths say something only if alignment is the ONE thing wrong with them"""
    a = fc1_fwd_split()
    assert lib.spv_enc_fc1_fwd_uses_dma(a["B"], a["G"], a["N1"], 3, 1, a["ldw"], a["ld_xb"]) == 1
    w = fc1_wgrad_split()
    assert lib.spv_enc_fc1_wgrad_split_uses_dma(w["B"], w["G"], w["N1"], w["ld_dh"], w["ld_xb"]) == 1
    for nsplit in (1, 3):
        g = gemm()
        assert lib.spv_gemm_bf16_uses_dma(g["a_kmajor"], g["M"], g["N"], g["K"], nsplit, g["a_tiles"], g["ldb"]) == 1


@pytest.mark.parametrize("name,entry,make,rc,text", CASES, ids=[c[0] for c in CASES])
def test_rejection(lib, name, entry, make, rc, text):
    got_rc, got_text = _call(lib, entry, make())
    assert (got_rc, got_text) == (rc, text)
