"""GPU: the decoder-preparation kernels one by one through the C ABI -- spv_zsplit_fwd / _bwd, spv_bn_fold_fwd / _bwd (with
zstats_bwd_kernel), spv_trunk_fold_fwd / _bwd (with trunk_zstats_kernel) and the statistics producer (dec_ops._zstats_batch through
spv_linear_wgrad) -- against the float64 definition of tests/_fold_reference.py.

Slicing and operand images are exact: compared bit for bit.  Every other output is held to the bound DERIVED in the module docstring of
tests/_fold_reference.py (roundings counted from csrc/spv_small.h times 2^-24 times the running-error form of the output); no tolerance is
picked here.  tests/test_fold_reference_cpu.py shows that a float32 transcription stays inside those bounds and that on the standard
cases they are at most 1e-3 of the output's largest value.  Unless a test is about the statistics producer, zsum / zz (and stat = (mean,
var) for the backward calls) are float64 values rounded once, so each kernel is judged on its own arithmetic.

Every output buffer carries a margin filled with a sentinel, and whatever the header says is never written must still hold it.
Shapes: the grids of tests/_fold_reference.py (the smallest that reach each code path: partial gene blocks, one to five 256-gene blocks,
K across the 4-lane / 16-row / 32-column tile edges, the wide layout's second tile, one and two 64-cell blocks)."""
import ctypes as C

import pytest
import torch

from tests import _fold_reference as R

pytestmark = pytest.mark.gpu

SENT = -7.5
SENT16 = 0x5A5A
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _f(dev, n, margin=64):
    return torch.full((n + margin,), SENT, dtype=torch.float32, device=dev)


def _h(dev, n, margin=64):
    return torch.full((n + margin,), SENT16, dtype=torch.int16, device=dev)


def _io(dev, t):
    """an in/out buffer: ``t`` in front, the sentinel margin behind"""
    b = _f(dev, t.numel())
    b[:t.numel()] = t.reshape(-1).to(dev)
    return b


def _up(dev, t):
    return t.contiguous().to(dev)


def _untouched(buf, n, what):
    tail = buf[n:].cpu()
    assert bool((tail == (SENT if buf.dtype == torch.float32 else SENT16)).all()), f"{what}: written past its extent"


def _close(name, got, ref, bound, where):
    got = got.detach().cpu().double().reshape(ref.shape)
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all()), f"{name} {where}: not finite"
    over = err > bound
    if bool(over.any()):
        i = int(torch.argmax((err - bound).flatten()))
        raise AssertionError(f"{name} {where}: {int(over.sum())} of {over.numel()} over the bound; worst at flat index {i}: "
                             f"got {got.flatten()[i]:.9g} ref {ref.flatten()[i]:.9g} error {err.flatten()[i]:.3e} bound {bound.flatten()[i]:.3e}")


def _where(c, training):
    return f"(K {c['K']}, G {c['G']}, B {c['B']}, {c['kind']}, {'train' if training else 'eval'})"


def _chunks(xs, n):
    return [xs[i:i + n] for i in range(0, len(xs), n)]


# ==== latent slicing and the operand images: exact ============================================================================================
ZS_SHAPES = [(1, 1, 0), (3, 6, 0), (15, 31, 0), (16, 32, 1), (31, 63, 1)]


@pytest.mark.parametrize("ngroups", [1, 2])
@pytest.mark.parametrize("n_p,n_s,wide", ZS_SHAPES)
@pytest.mark.parametrize("B", [1, 5, 130])
def test_zsplit_slicing_and_images_are_exact(dev, B, n_p, n_s, wide, ngroups):
    from spvipes_amd import _abi
    from spvipes_amd._abi import SpvZsplitArgs, ptr, round_up, stream_ptr
    Bp, nt = round_up(B, 128), n_p + n_s
    KP, KS = (32, 64) if wide else (16, 32)
    KPS = KP + KS
    am_col, am_cols = 8, round_up(nt + 1, 8) + 8
    ld_am = am_col + am_cols + 8   # (columns before and behind the tail belong to someone else)
    gen = torch.Generator().manual_seed(97 * B + 7 * n_p + n_s)
    priv = [torch.randn(B, n_p, generator=gen) for _ in range(ngroups)]
    poe = [torch.randn(B, n_s, generator=gen) for _ in range(ngroups)]
    dpriv, dpoe = [_up(dev, t) for t in priv], [_up(dev, t) for t in poe]

    def run(mode):
        za = SpvZsplitArgs()
        za.B, za.n_p, za.n_s, za.ngroups, za.kslots = B, n_p, n_s, ngroups, wide
        za.ld_am, za.am_col, za.am_cols, za.Bp = ld_am, am_col, am_cols, Bp
        out = []
        for g in range(ngroups):
            o = dict(zcat=_f(dev, B * nt), am_hi=_h(dev, Bp * ld_am), am_lo=_h(dev, Bp * ld_am), aps_hi=_h(dev, Bp * KPS), aps_lo=_h(dev, Bp * KPS))
            za.priv[g], za.poe[g], za.zcat[g] = ptr(dpriv[g]), ptr(dpoe[g]), ptr(o["zcat"])
            if mode != "plain":
                za.am_hi[g], za.aps_hi[g] = ptr(o["am_hi"]), ptr(o["aps_hi"])
                if mode == "pack":
                    za.am_lo[g], za.aps_lo[g] = ptr(o["am_lo"]), ptr(o["aps_lo"])
            out.append(o)
        _abi.call("spv_zsplit_fwd", C.byref(za), stream_ptr())
        torch.cuda.synchronize()
        return out

    res = {m: run(m) for m in ("pack", "plain", "hi_only")}
    for g in range(ngroups):
        zc = R.zcat_of(priv[g], poe[g])
        # the index map of the A6 quirk, spelled out: z_private = Z[:, n_s : n_s + n_p], z_shared = Z[:, :n_s] of Z = [private | poe]
        Z = torch.cat([priv[g], poe[g]], 1)
        for c in range(nt):
            assert torch.equal(zc[:, c], Z[:, n_s + c] if c < n_p else Z[:, c - n_p])
        am = torch.zeros(Bp, am_cols)
        am[:B, :nt], am[:B, nt] = zc, 1.0
        aps = torch.zeros(Bp, KPS)
        aps[:B, :n_p], aps[:B, n_p], aps[:B, KP:KP + n_s], aps[:B, KP + n_s] = zc[:, :n_p], 1.0, zc[:, n_p:], 1.0
        am_w, aps_w = R.split_bf16(am), R.split_bf16(aps)
        for mode, r in res.items():
            o = r[g]
            got = o["zcat"][:B * nt].cpu().view(B, nt)
            assert torch.equal(got.view(torch.int32), zc.view(torch.int32)), f"zcat ({mode})"
            _untouched(o["zcat"], B * nt, f"zcat ({mode})")
            for half, (name, exp, ld, c0, nc) in enumerate((("am_hi", am_w[0], ld_am, am_col, am_cols), ("am_lo", am_w[1], ld_am, am_col, am_cols),
                                                            ("aps_hi", aps_w[0], KPS, 0, KPS), ("aps_lo", aps_w[1], KPS, 0, KPS))):
                buf = o[name].cpu()
                written = mode == "pack" or (mode == "hi_only" and name.endswith("_hi"))
                if not written:   # an image that was not asked for: nothing may have been written through it
                    assert bool((buf == SENT16).all()), f"{name} ({mode}) written though absent"
                    continue
                img = buf[:Bp * ld].view(Bp, ld)
                assert torch.equal(img[:, c0:c0 + nc], exp), f"{name} ({mode}): words differ from split_bf16 of [z | 1 | 0]"
                assert bool((img[:, :c0] == SENT16).all()) and bool((img[:, c0 + nc:] == SENT16).all()), f"{name} ({mode}): columns outside the tail"
                assert bool((buf[Bp * ld:] == SENT16).all()), f"{name} ({mode}): past the image"

    # backward: the exact inverse permutation (autograd of the definition: every column of Z is used once, so no sum is formed)
    za = SpvZsplitArgs()
    za.B, za.n_p, za.n_s, za.ngroups = B, n_p, n_s, ngroups
    outs = []
    for g in range(ngroups):
        dzc = torch.randn(B, nt, generator=gen)
        o = dict(dzc=dzc, d=_up(dev, dzc), dp=_f(dev, B * n_p), dq=_f(dev, B * n_s))
        za.d_zcat[g], za.d_priv[g], za.d_poe[g] = ptr(o["d"]), ptr(o["dp"]), ptr(o["dq"])
        outs.append(o)
    _abi.call("spv_zsplit_bwd", C.byref(za), stream_ptr())
    torch.cuda.synchronize()
    for g, o in enumerate(outs):
        p, q = priv[g].clone().requires_grad_(True), poe[g].clone().requires_grad_(True)
        gp, gq = torch.autograd.grad(R.zcat_of(p, q), (p, q), o["dzc"])
        assert torch.equal(o["dp"][:B * n_p].cpu().view(B, n_p), gp) and torch.equal(o["dq"][:B * n_s].cpu().view(B, n_s), gq)
        _untouched(o["dp"], B * n_p, "d_priv"); _untouched(o["dq"], B * n_s, "d_poe")


# ==== the regressor fold =========================================================================================================================
def _slot(K, wide):
    """(ld_img, col_off, slot) of a problem's image slot: the product's two slots where K fits them, else the smallest legal one"""
    if wide:
        return (96, 32, 64) if K < 64 else (96, 24, 72)
    if K == 32:
        return (48, 8, 40)
    if K >= 16 or K % 2 == 0:
        return (48, 16, 32)
    return (48, 0, 16)


def _fold_header(B, training, wide):
    from spvipes_amd import dec_ops
    from spvipes_amd._abi import DEC_NARROW, DEC_WIDE
    return dec_ops._fold_batch(B, training, R.MOMENTUM, DEC_WIDE if wide else DEC_NARROW)


def _stat_f32(ref):
    return torch.stack([ref["mean0"], ref["var"]], 1).float()


def _fold_fwd(dev, cases, B, training, wide, stats=None):
    from spvipes_amd import _abi
    from spvipes_amd._abi import ptr, round_up, stream_ptr
    fb = _fold_header(B, training, wide)
    fb.nprob = len(cases)
    hold = []
    for i, c in enumerate(cases):
        G, K = c["G"], c["K"]
        Gp = round_up(G, 256)
        ld, off, slot = _slot(K, wide)
        zsum, zz = stats[i] if stats is not None else R.stats_f32(c["z"])
        t = dict(W=_up(dev, c["W"]), gamma=_up(dev, c["gamma"]), beta=_up(dev, c["beta"]), zsum=_up(dev, zsum), zz=_up(dev, zz),
                 rm=_io(dev, c["rm"]), rv=_io(dev, c["rv"]), stat=_f(dev, 2 * G), hi=_h(dev, Gp * ld), lo=_h(dev, Gp * ld), Gp=Gp, slot=(ld, off, slot))
        q = fb.p[i]
        q.W, q.gamma, q.beta, q.running_mean, q.running_var = ptr(t["W"]), ptr(t["gamma"]), ptr(t["beta"]), ptr(t["rm"]), ptr(t["rv"])
        q.zsum, q.zz, q.stat = ptr(t["zsum"]), ptr(t["zz"]), ptr(t["stat"])
        q.img_hi, q.img_lo, q.ld_img, q.col_off, q.slot = ptr(t["hi"]), ptr(t["lo"]), ld, off, slot
        q.G, q.Gp, q.K = G, Gp, K
        hold.append(t)
    _abi.call("spv_bn_fold_fwd", C.byref(fb), stream_ptr())
    torch.cuda.synchronize()
    return hold


def _check_fold_fwd(c, t, training, ref=None):
    G, K, Gp = c["G"], c["K"], t["Gp"]
    ld, off, slot = t["slot"]
    where = _where(c, training)
    ref = ref if ref is not None else R.reference(c, training)
    bnd = R.forward_bounds(c, ref, training, image=True)
    stat = t["stat"][:2 * G].cpu().view(G, 2)
    _close("stat mean", stat[:, 0], ref["mean0"], bnd["mean0"], where)
    _close("stat var", stat[:, 1], ref["var"], bnd["var"], where)
    assert bool((stat[:, 1] >= 0).all()), f"negative variance {where}"
    _close("running_mean", t["rm"][:G], ref["rm"], bnd["rm"], where)
    _close("running_var", t["rv"][:G], ref["rv"], bnd["rv"], where)
    for k in ("stat", "rm", "rv"):
        _untouched(t[k], 2 * G if k == "stat" else G, k + where)
    hi, lo = t["hi"].cpu(), t["lo"].cpu()
    for name, buf in (("img_hi", hi), ("img_lo", lo)):
        img = buf[:Gp * ld].view(Gp, ld)
        assert bool((buf[Gp * ld:] == SENT16).all()) and bool((img[:, :off] == SENT16).all()) and bool((img[:, off + slot:] == SENT16).all()), \
            f"{name} {where}: written outside its slot"
    H, L = hi[:Gp * ld].view(Gp, ld)[:, off:off + slot], lo[:Gp * ld].view(Gp, ld)[:, off:off + slot]
    vh, vl = R.bf16_value(H), R.bf16_value(L)
    val = vh + vl
    _close("image W'", val[:G, :K], ref["Wf"], bnd["Wf"], where)
    _close("image c", val[:G, K], ref["cf"], bnd["cf"], where)
    assert bool((H[G:] == 0).all()) and bool((L[G:] == 0).all()), f"image rows G..Gp not zero {where}"
    assert bool((H[:, K + 1:] == 0).all()) and bool((L[:, K + 1:] == 0).all()), f"image slots above K + 1 not zero {where}"
    assert bool((vl.abs() <= R.bf16_ulp(H) / 2).all()), f"|lo| above half an ulp of hi {where}"
    # hi = bf16(hi + lo), compared as values (-0 = +0 at gamma = 0).  The one exception a correct split has: v - hi just under half an ulp
    # rounds, as lo, UP to exactly half an ulp; hi + lo is then the tie between hi and its neighbour, which round-to-even may give to the
    # neighbour (tests/test_fold_reference_cpu.py: test_split_bf16_transcription shows it happens only there).
    tie = vl.abs() == R.bf16_ulp(H) / 2
    assert bool(((val.float().to(torch.bfloat16).double() == vh) | tie).all()), f"hi is not bf16(hi + lo) {where}"
    return stat


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B", R.FWD_B)
@pytest.mark.parametrize("wide", [False, True])
def test_fold_forward_against_float64(dev, wide, B, training):
    cases = [R.standard_case(K, G, b) for (K, G, b) in R.fwd_cases(wide) if b == B]
    assert cases
    for chunk in _chunks(cases, 8):
        for c, t in zip(chunk, _fold_fwd(dev, chunk, B, training, wide)):
            _check_fold_fwd(c, t, training)


@pytest.mark.parametrize("training", [True, False])
def test_fold_forward_batch_of_unequal_problems(dev, training):
    """(G, K) = (1, 3), (300, 31), (65, 16), (257, 1) in one launch: the grid is sized for the largest, the others' workgroups return early"""
    cases = [R.standard_case(K, G, 37) for (G, K) in R.MIXED_BATCH]
    for c, t in zip(cases, _fold_fwd(dev, cases, 37, training, False)):
        _check_fold_fwd(c, t, training)


def _ld_dw(K, mode):
    """K + 1 (dense), or the operand slab's pitch: 48 where K + 1 fits it, else the wide layout's 96"""
    return K + 1 if mode == 0 else (48 if K + 1 <= 48 else 96)


def _fold_bwd(dev, cases, refs, B, training, wide, ld_mode, fused=None):
    """``fused`` = per problem (zcat buffer, d zcat buffer, nt, zcol, out_priv, out_poe, n_p, n_s): z and d z are column blocks of the two
    [B][nt] matrices (and with out_priv set the finished columns go to the latent gradients)"""
    from spvipes_amd import _abi
    from spvipes_amd._abi import ptr, stream_ptr
    fb = _fold_header(B, training, wide)
    fb.nprob = len(cases)
    hold = []
    for i, (c, ref) in enumerate(zip(cases, refs)):
        G, K = c["G"], c["K"]
        nblk, nred, ld = (G + 255) // 256, K + K * K, _ld_dw(K, ld_mode)
        zsum, zz = R.stats_f32(c["z"])
        g = torch.full((G, ld), NAN)   # (the padding columns of d W' are nobody's: a read of them poisons the result)
        g[:, :K + 1] = c["dWeff"]
        t = dict(W=_up(dev, c["W"]), gamma=_up(dev, c["gamma"]), beta=_up(dev, c["beta"]), rm=_up(dev, c["rm"]), rv=_up(dev, c["rv"]),
                 zsum=_up(dev, zsum), zz=_up(dev, zz), stat=_up(dev, _stat_f32(ref)), g=_up(dev, g),
                 dW=_f(dev, G * K), dgamma=_f(dev, G), dbeta=_f(dev, G), red=_f(dev, (nblk + 1) * nred), nblk=nblk)
        q = fb.p[i]
        q.W, q.gamma, q.beta, q.running_mean, q.running_var = ptr(t["W"]), ptr(t["gamma"]), ptr(t["beta"]), ptr(t["rm"]), ptr(t["rv"])
        q.zsum, q.zz, q.stat, q.dWeff, q.ld_dw = ptr(t["zsum"]), ptr(t["zz"]), ptr(t["stat"]), ptr(t["g"]), ld
        q.dW, q.dgamma, q.dbeta, q.red_part = ptr(t["dW"]), ptr(t["dgamma"]), ptr(t["dbeta"]), ptr(t["red"])
        q.G, q.Gp, q.K = G, G, K
        if fused is None:
            t["z"], t["dz"] = _up(dev, c["z"]), _io(dev, c["dz0"])
            q.z, q.ldz, q.dz, q.lddz = ptr(t["z"]), K, ptr(t["dz"]), K
        else:
            zcat, dzcat, nt, zcol, op, oq, n_p, n_s = fused[i]
            q.z, q.ldz, q.dz, q.lddz = zcat.data_ptr() + 4 * zcol, nt, dzcat.data_ptr() + 4 * zcol, nt
            if op is not None:
                q.zcol, q.out_priv, q.out_poe, q.n_p, q.n_s = zcol, ptr(op), ptr(oq), n_p, n_s
        hold.append(t)
    _abi.call("spv_bn_fold_bwd", C.byref(fb), stream_ptr())
    torch.cuda.synchronize()
    return hold


def _check_fold_bwd(c, t, ref, training):
    G, K, B = c["G"], c["K"], c["B"]
    where = _where(c, training)
    bnd = R.backward_bounds(c, ref, training)
    _close("dW", t["dW"][:G * K], ref["dW"], bnd["dW"], where)
    _close("dgamma", t["dgamma"][:G], ref["dgamma"], bnd["dgamma"], where)
    assert torch.equal(t["dbeta"][:G].cpu(), c["dWeff"][:, K].contiguous()), f"dbeta is not the copy of d c {where}"
    _close("dbeta", t["dbeta"][:G], ref["dbeta"], torch.zeros(G, dtype=torch.float64), where)
    _untouched(t["dW"], G * K, "dW" + where); _untouched(t["dgamma"], G, "dgamma" + where); _untouched(t["dbeta"], G, "dbeta" + where)
    nblk, nred = t["nblk"], K + K * K
    if training:
        row = t["red"][nblk * nred:(nblk + 1) * nred]
        _close("red d zbar", row[:K], ref["dzbar"], bnd["dzbar"], where)
        _close("red d C", row[K:], ref["dC"], bnd["dC"], where)
        _untouched(t["red"], (nblk + 1) * nred, "red_part" + where)
        if "dz" in t:
            _close("dz", t["dz"][:B * K], ref["dz_acc"], bnd["dz_acc"], where)
            _untouched(t["dz"], B * K, "dz" + where)
    else:   # eval mode writes dW, dgamma, dbeta and nothing else
        _untouched(t["red"], 0, "red_part (eval)" + where)
        assert torch.equal(t["dz"][:B * K].cpu().view(B, K), c["dz0"]), f"dz changed in eval mode {where}"
        _untouched(t["dz"], B * K, "dz" + where)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B", R.BWD_B)
@pytest.mark.parametrize("wide", [False, True])
def test_fold_backward_against_autograd(dev, wide, B, training):
    cases = [R.standard_case(K, G, b) for (K, G, b) in R.bwd_cases(wide) if b == B]
    assert cases
    for chunk in _chunks(cases, 8):
        refs = [R.reference(c, training, backward=True) for c in chunk]
        for ld_mode in (0, 1):
            for c, t, ref in zip(chunk, _fold_bwd(dev, chunk, refs, B, training, wide, ld_mode), refs):
                _check_fold_bwd(c, t, ref, training)


@pytest.mark.parametrize("n_p,n_s,wide", [(3, 6, 0), (15, 31, 0), (31, 63, 1)])
@pytest.mark.parametrize("B", [5, 130])
def test_fold_backward_fused_slicing_has_the_unfused_bits(dev, B, n_p, n_s, wide):
    """zcol / out_priv / out_poe on the two problems of each of two groups: the latent gradients carry the bits of the unfused call followed
    by spv_zsplit_bwd, and d zcat itself is only read"""
    from spvipes_amd import _abi
    from spvipes_amd._abi import SpvZsplitArgs, ptr, stream_ptr
    nt, G = n_p + n_s, 300
    gen = torch.Generator().manual_seed(5 * B + n_p)
    cases, refs, lay = [], [], []
    for g in range(2):
        zcat, dz0 = torch.randn(B, nt, generator=gen), torch.randn(B, nt, generator=gen)
        for (zcol, K) in ((0, n_p), (n_p, n_s)):
            c = R.make_case(K, G + g, B, salt=1 + g)
            c["z"], c["dz0"] = zcat[:, zcol:zcol + K].contiguous(), dz0[:, zcol:zcol + K].contiguous()
            cases.append(c); refs.append(R.reference(c, True, backward=True)); lay.append((g, zcat, dz0, zcol))

    def run(fuse):
        zc = {g: _up(dev, z) for (g, z, _, col) in lay if col == 0}
        dzc = {g: _io(dev, d) for (g, _, d, col) in lay if col == 0}
        front = {g: (_f(dev, B * n_p + 64), _f(dev, B * n_s + 64)) for g in zc}   # (a margin in FRONT of the latent gradients as well)
        op, oq = {g: front[g][0][64:] for g in zc}, {g: front[g][1][64:] for g in zc}
        fused = [(zc[g], dzc[g], nt, col, op[g] if fuse else None, oq[g] if fuse else None, n_p, n_s) for (g, _, _, col) in lay]
        hold = _fold_bwd(dev, cases, refs, B, True, bool(wide), 0, fused=fused)
        for g in zc:
            assert bool((front[g][0][:64] == SENT).all()) and bool((front[g][1][:64] == SENT).all()), "written in front of the latent gradients"
        return dzc, op, oq, hold

    dzc_u, op_u, oq_u, hold_u = run(False)
    za = SpvZsplitArgs()
    za.B, za.n_p, za.n_s, za.ngroups = B, n_p, n_s, 2
    for g in range(2):
        za.d_zcat[g], za.d_priv[g], za.d_poe[g] = ptr(dzc_u[g]), ptr(op_u[g]), ptr(oq_u[g])
    _abi.call("spv_zsplit_bwd", C.byref(za), stream_ptr())
    torch.cuda.synchronize()
    dzc_f, op_f, oq_f, hold_f = run(True)
    for g in range(2):
        assert torch.equal(op_f[g].cpu().view(torch.int32), op_u[g].cpu().view(torch.int32)), f"d private_log_z, group {g}"
        assert torch.equal(oq_f[g].cpu().view(torch.int32), oq_u[g].cpu().view(torch.int32)), f"d poe_log_z, group {g}"
        _untouched(op_f[g], B * n_p, "out_priv"); _untouched(oq_f[g], B * n_s, "out_poe")
        dz0 = [d for (gg, _, d, col) in lay if gg == g and col == 0][0]
        assert torch.equal(dzc_f[g][:B * nt].cpu().view(B, nt), dz0), "the fused call wrote into d zcat"
    # and the unfused d zcat is right: the accumulated d z of each problem, in its column block
    for c, ref, (g, _, _, col) in zip(cases, refs, lay):
        bnd = R.backward_bounds(c, ref, True)
        got = dzc_u[g][:B * nt].view(B, nt)[:, col:col + c["K"]]
        _close("dz (column block)", got, ref["dz_acc"], bnd["dz_acc"], _where(c, True))
    for c, t, ref in zip(cases, hold_f, refs):
        _check_fold_bwd(c, t, ref, True)


# ==== the mixing trunk's fold ===================================================================================================================
def _trunk(dev, cases, refs, B, training, use_bias, use_dbias):
    from spvipes_amd import _abi
    from spvipes_amd._abi import SpvTrunkBatch, ptr, stream_ptr
    tb = SpvTrunkBatch()
    tb.nprob, tb.B, tb.training, tb.eps, tb.momentum = len(cases), B, int(training), 1e-3, R.MOMENTUM
    hold = []
    for i, (c, ref) in enumerate(zip(cases, refs)):
        N, K = c["G"], c["K"]
        nred, nb = K + K * K, (N + 63) // 64
        zsum, zz = R.stats_f32(c["z"])
        t = dict(W=_up(dev, c["W"]), bias=_up(dev, c["bias"]), gamma=_up(dev, c["gamma"]), beta=_up(dev, c["beta"]), zsum=_up(dev, zsum), zz=_up(dev, zz),
                 rm=_io(dev, c["rm"]), rv=_io(dev, c["rv"]), Wf=_f(dev, N * K), cf=_f(dev, N), stat=_f(dev, 2 * N), stat_in=_up(dev, _stat_f32(ref)),
                 dWf=_up(dev, c["dWeff"][:, :K]), dcf=_up(dev, c["dWeff"][:, K]), dW=_f(dev, N * K), dbias=_f(dev, N), dgamma=_f(dev, N), dbeta=_f(dev, N),
                 dred=_f(dev, nb * nred), z=_up(dev, c["z"]), dz=_io(dev, c["dz0"]), nb=nb)
        q = tb.p[i]
        q.W, q.bias, q.gamma, q.beta = ptr(t["W"]), ptr(t["bias"]) if use_bias else None, ptr(t["gamma"]), ptr(t["beta"])
        q.running_mean, q.running_var, q.zsum, q.zz = ptr(t["rm"]), ptr(t["rv"]), ptr(t["zsum"]), ptr(t["zz"])
        q.Wf, q.cf, q.stat, q.N, q.K = ptr(t["Wf"]), ptr(t["cf"]), ptr(t["stat"]), N, K
        hold.append(t)
    _abi.call("spv_trunk_fold_fwd", C.byref(tb), stream_ptr())
    for i, t in enumerate(hold):   # the backward call reads stat: the float64 value rounded once, as for the regressors
        q = tb.p[i]
        q.stat = ptr(t["stat_in"])
        q.dWf, q.dcf, q.dW, q.dbias, q.dgamma, q.dbeta = ptr(t["dWf"]), ptr(t["dcf"]), ptr(t["dW"]), ptr(t["dbias"]) if use_dbias else None, ptr(t["dgamma"]), ptr(t["dbeta"])
        q.dred, q.z, q.ldz, q.dz, q.lddz = ptr(t["dred"]), ptr(t["z"]), t["z"].shape[1], ptr(t["dz"]), t["z"].shape[1]
    _abi.call("spv_trunk_fold_bwd", C.byref(tb), stream_ptr())
    torch.cuda.synchronize()
    return hold


def _check_trunk(c, t, ref, training, use_bias, use_dbias):
    N, K, B = c["G"], c["K"], c["B"]
    where = _where(c, training) + f" bias {use_bias} dbias {use_dbias}"
    fb = R.forward_bounds(c, ref, training, use_bias=use_bias, image=False)
    stat = t["stat"][:2 * N].cpu().view(N, 2)
    _close("stat mean0", stat[:, 0], ref["mean0"], fb["mean0"], where)
    _close("stat var", stat[:, 1], ref["var"], fb["var"], where)
    assert bool((stat[:, 1] >= 0).all()), f"negative variance {where}"
    _close("running_mean", t["rm"][:N], ref["rm"], fb["rm"], where)
    _close("running_var", t["rv"][:N], ref["rv"], fb["rv"], where)
    _close("W'", t["Wf"][:N * K], ref["Wf"], fb["Wf"], where)
    _close("c'", t["cf"][:N], ref["cf"], fb["cf"], where)
    bb = R.backward_bounds(c, ref, training, use_bias=use_bias)
    _close("dW", t["dW"][:N * K], ref["dW"], bb["dW"], where)
    _close("dgamma", t["dgamma"][:N], ref["dgamma"], bb["dgamma"], where)
    assert torch.equal(t["dbeta"][:N].cpu(), c["dWeff"][:, K].contiguous()), f"dbeta is not the copy of d c' {where}"
    if use_dbias:
        # (without a bias the gradient with respect to one that is zero: the same formula, gc * inv in eval mode and 0 in training)
        dbias_ref = ref["dbias"] if use_bias else (torch.zeros(N, dtype=torch.float64) if training else c["dWeff"][:, K].double() * ref["inv"])
        if training:
            assert bool((t["dbias"][:N].cpu() == 0).all()), f"training-mode d bias is not exactly zero {where}"
        _close("dbias", t["dbias"][:N], dbias_ref, bb["dbias"], where)
        _untouched(t["dbias"], N, "dbias" + where)
    else:
        _untouched(t["dbias"], 0, "dbias (absent)" + where)
    for k, n in (("stat", 2 * N), ("rm", N), ("rv", N), ("Wf", N * K), ("cf", N), ("dW", N * K), ("dgamma", N), ("dbeta", N)):
        _untouched(t[k], n, k + where)
    nred = K + K * K
    if training:
        part = t["dred"][:t["nb"] * nred].cpu().double().view(t["nb"], nred).sum(0)   # (the block partials, summed here in float64)
        _close("dred d zbar", part[:K], ref["dzbar"], bb["dzbar"], where)
        _close("dred d C", part[K:], ref["dC"], bb["dC"], where)
        _untouched(t["dred"], t["nb"] * nred, "dred" + where)
        _close("dz", t["dz"][:B * K], ref["dz_acc"], bb["dz_acc"], where)
    else:
        _untouched(t["dred"], 0, "dred (eval)" + where)
        assert torch.equal(t["dz"][:B * K].cpu().view(B, K), c["dz0"]), f"dz changed in eval mode {where}"
    _untouched(t["dz"], B * K, "dz" + where)


@pytest.mark.parametrize("use_dbias", [True, False])
@pytest.mark.parametrize("use_bias", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B", R.TRUNK_B)
def test_trunk_fold_forward_and_backward(dev, B, training, use_bias, use_dbias):
    cases = [R.standard_case(K, N, b, trunk=True) for (K, N, b) in R.trunk_cases() if b == B]
    assert len(cases) >= 3
    launches = [[cases[0]], [cases[-1]]] + _chunks(cases, 2)   # one problem, and two problems of unequal N (and K)
    assert any(len(l) == 2 and l[0]["G"] != l[1]["G"] for l in launches)
    for chunk in launches:
        refs = [R.reference(c, training, use_bias=use_bias, backward=True) for c in chunk]
        for c, t, ref in zip(chunk, _trunk(dev, chunk, refs, B, training, use_bias, use_dbias), refs):
            _check_trunk(c, t, ref, training, use_bias, use_dbias)


# ==== the statistics producer =====================================================================================================================
class _Ws:
    def __init__(self, dev):
        self.dev = dev

    def get(self, name, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.dev)


@pytest.mark.parametrize("n_p,n_s", [(3, 6), (15, 31)])
@pytest.mark.parametrize("B", R.STATS_B)
def test_statistics_producer_against_float64(dev, B, n_p, n_s):
    """zsum / zz as the step forms them: dec_ops._zstats_batch through spv_linear_wgrad (private, shared and trunk blocks of two groups);
    B = 1100 takes the 16-slice path, the others the direct one"""
    from spvipes_amd import dec_ops, nn_ops
    nt = n_p + n_s
    gen = torch.Generator().manual_seed(B + n_p)
    z = [torch.randn(B, nt, generator=gen) + 0.5 * torch.randn(1, nt, generator=gen) for _ in range(2)]
    zcat = [_up(dev, t) for t in z]
    blocks = ((0, n_p), (n_p, n_s))
    zsum = [[_f(dev, n) for (_, n) in blocks] for _ in range(2)]
    zz = [[_f(dev, n * n) for (_, n) in blocks] for _ in range(2)]
    zsum_t, zz_t = [_f(dev, nt) for _ in range(2)], [_f(dev, nt * nt) for _ in range(2)]
    b = dec_ops._zstats_batch(B, n_p, n_s, zcat, zsum, zz, trunk=(zsum_t, zz_t))
    nn_ops._wgrad(b, _Ws(dev))
    torch.cuda.synchronize()
    for g in range(2):
        for (off, n), s, q in list(zip(blocks, zsum[g], zz[g])) + [((0, nt), zsum_t[g], zz_t[g])]:
            zb = z[g][:, off:off + n].double()
            bs, bq = R.stats_bounds(zb)
            where = f"(B {B}, group {g}, columns {off}..{off + n})"
            _close("zsum", s[:n], zb.sum(0), bs, where)
            _close("zz", q[:n * n], zb.T @ zb, bq, where)
            _untouched(s, n, "zsum" + where); _untouched(q, n * n, "zz" + where)


# ==== degenerate and ill-conditioned inputs: the same assertions, the bound moves with the inputs ==================================================
def _inv_errors(c, stat, ref, bnd):
    """relative error of gamma / sqrt(var + eps) formed (in float64) from the kernel's variance; its bound; and the same for float32 torch
    BatchNorm1d of z W^T on the CPU, the library yardstick"""
    var_k = stat[:, 1].double()
    gam = c["gamma"].double()
    inv_ref = ref["inv"]
    nz = inv_ref != 0
    rel = lambda inv: ((inv - inv_ref).abs()[nz] / inv_ref.abs()[nz]).max().item()
    bn = torch.nn.BatchNorm1d(c["G"], eps=1e-3, momentum=1.0)
    bn.train()
    with torch.no_grad():
        bn(c["z"] @ c["W"].T)
    B = c["B"]
    var32 = bn.running_var.double() * (B - 1) / B
    bound = (bnd["var"] / (2 * (ref["var"] + R.EPS)))[nz].max().item()
    return rel(gam / torch.sqrt(var_k + R.EPS)), bound, rel(gam / torch.sqrt(var32 + R.EPS))


def _fold_both(dev, c, wide):
    ref = R.reference(c, True, backward=True)
    t = _fold_fwd(dev, [c], c["B"], True, wide)[0]
    stat = _check_fold_fwd(c, t, True, ref=ref)
    tb = _fold_bwd(dev, [c], [ref], c["B"], True, wide, 0)[0]
    _check_fold_bwd(c, tb, ref, True)
    return stat, ref


@pytest.mark.parametrize("kind", R.KINDS_DEGENERATE)
def test_degenerate_and_ill_conditioned_inputs(dev, kind):
    for (K, G, B, wide) in ((15, 300, 1100, False), (31, 65, 37, False), (47, 257, 130, True)):
        c = R.make_case(K, G, B, kind=kind)
        stat, ref = _fold_both(dev, c, wide)
        if kind == "equal_rows":   # every variance is zero: exactly, or within the bound (checked above), never negative or NaN
            assert bool((stat[:, 1] >= 0).all()) and bool(torch.isfinite(stat).all())
        if kind in ("off3", "off30"):
            e, b, y = _inv_errors(c, stat, ref, R.forward_bounds(c, ref, True))
            print(f"fold accuracy [{kind}] K {K} B {B}: kernel rel. error of gamma/sqrt(var+eps) {e:.2e}, bound {b:.2e}, float32 torch BatchNorm {y:.2e}")
    c = R.make_case(33, 65, 130, kind=kind, trunk=True)
    for use_bias in (True, False):
        ref = R.reference(c, True, use_bias=use_bias, backward=True)
        t = _trunk(dev, [c], [ref], 130, True, use_bias, True)[0]
        _check_trunk(c, t, ref, True, use_bias, True)


def test_fold_accuracy_table(dev):
    """printed, for DESIGN.md: the relative error of gamma / sqrt(var + eps) against offset / spread of the latents (B 1100, K 15, G 300);
    the assertions are the same derived bounds"""
    print("\noffset/spread  offset  spread  kernel      bound       float32 torch BatchNorm")
    for mean, spread in ((0.0, 1.0), (1.0, 1.0), (3.0, 1.0), (10.0, 1.0), (1.0, 0.05), (1.5, 0.05), (3.0, 0.05), (5.0, 0.05), (10.0, 0.05), (30.0, 0.05)):
        c = R.make_case(15, 300, 1100, kind=f"off:{mean}:{spread}")
        ref = R.reference(c, True)
        t = _fold_fwd(dev, [c], 1100, True, False)[0]
        stat = _check_fold_fwd(c, t, True, ref=ref)
        e, b, y = _inv_errors(c, stat, ref, R.forward_bounds(c, ref, True))
        print(f"{mean / spread:13.0f}  {mean:6.2f}  {spread:6.2f}  {e:.2e}    {b:.2e}    {y:.2e}")
