"""GPU: the mixing-head weights take their Adam step inside their slab-sum launch (spv_reduce_slabs_adam), the optimiser launch
skips them (spv_adam_step_images, skip ranges), and a training step armed that way is the step it was, bit for bit."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, WD = 5e-3, 0.9, 0.999, 0.01, 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()  # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _words(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _adam_images(p, g, m, v, images, skip, counter, t_dev):
    from spvipes_amd import _abi
    imgs = (_abi.SpvAdamImage * len(images))(*images) if images else None
    rng = (_abi.SpvAdamRange * len(skip))(*[_abi.SpvAdamRange(b, c) for b, c in skip]) if skip else None
    _abi.call("spv_adam_step_images", _abi.ptr(p), _abi.ptr(g), _abi.ptr(m), _abi.ptr(v), p.numel(), LR, B1, B2, EPS, WD, 1.0, 1.0, 1.0,
              imgs, len(images), rng, len(skip), _abi.ptr(counter), _abi.ptr(t_dev), B1, B2, _abi.stream_ptr())


def _image(dst, begin, count, cols, row_off, col_off, fmt, scale):
    from spvipes_amd import _abi
    d = _abi.SpvAdamImage()
    d.begin, d.count, d.cols, d.row_off, d.col_off, d.fmt, d.ld, d.dst, d.scale = begin, count, cols, row_off, col_off, fmt, dst.shape[1], _abi.ptr(dst), scale
    return d


# ld_src = 320 throughout (the decoder's K_M pitch), so a problem at col_off = 291 has at most 29 columns: the (64, 1) shape is the
# b_m problem and takes both offsets, the matrix shapes take col_off = 0.  (5, 291): less than one workgroup, odd columns; (130, 291):
# several workgroups, rows that end inside a wave; (33, 292): columns a multiple of 4 (where spv_reduce_slabs takes its 16-byte path).
CASES = [(5, 291, 0), (130, 291, 0), (33, 292, 0), (64, 1, 0), (64, 1, 291)]


@pytest.mark.parametrize("rows,cols,col_off", CASES)
@pytest.mark.parametrize("nslabs", [1, 3, 4, 8])
def test_fused_launch_equals_slab_sum_then_adam_word_for_word(dev, nslabs, rows, cols, col_off):
    """spv_reduce_slabs_adam against spv_reduce_slabs followed by spv_adam_step_images on copies of the same buffers: gradient, p, m, v
    and the image agree word for word, over two consecutive steps (the second with non-zero moments), for t_dev 0 and 7, without an
    image and with a bf16 / an f16 one.  The parameter sits at flat offset 20: a 4-element but not a 16-element boundary."""
    from spvipes_amd import _abi
    from spvipes_amd._abi import SpvReduceAdamBatch, SpvReduceBatch, ptr, stream_ptr
    from spvipes_amd.dec_ops import _add_red
    gen = torch.Generator(device=dev).manual_seed(1000 * nslabs + rows + col_off)
    ld, off, count = 320, 20, rows * cols
    n = off + (count + 3) // 4 * 4 + 12
    alpha = torch.tensor(0.37, device=dev)
    for t0 in (0, 7):
        for fmt in (None, _abi.IMAGE_BF16, _abi.IMAGE_F16):
            p0 = torch.randn(n, generator=gen, device=dev)
            bufs = [dict(p=p0.clone(), g=torch.randn(n, generator=gen, device=dev), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev),
                         img=torch.full((rows + 3, cols + 8), 0x1234, dtype=torch.int16, device=dev), t=torch.tensor(t0, dtype=torch.int64, device=dev))
                    for _ in range(2)]
            bufs[1]["g"].copy_(bufs[0]["g"])
            fused, ref = bufs
            scale = 256.0 if fmt == _abi.IMAGE_F16 else 1.0
            for step in range(2):
                src = torch.randn(nslabs, rows, ld, generator=gen, device=dev)
                # fused
                ba = SpvReduceAdamBatch()
                rb = SpvReduceBatch()
                rb.nprob = 0
                _add_red(rb, src, nslabs, rows * ld, ld, rows, cols, fused["g"][off:off + count], cols, col_off=col_off, alpha=alpha)
                ba.nprob, q = 1, ba.p[0]
                q.r = rb.p[0]
                q.p, q.m, q.v = fused["p"].data_ptr() + 4 * off, fused["m"].data_ptr() + 4 * off, fused["v"].data_ptr() + 4 * off
                if fmt is not None:
                    q.img = _image(fused["img"], 0, count, cols, 2, 3, fmt, scale)
                _abi.call("spv_reduce_slabs_adam", C.byref(ba), LR, B1, B2, EPS, WD, 1.0, 1.0, 1.0, ptr(fused["t"]), B1, B2, stream_ptr())
                # reference: the two launches of today's step
                rb2 = SpvReduceBatch()
                rb2.nprob = 0
                _add_red(rb2, src, nslabs, rows * ld, ld, rows, cols, ref["g"][off:off + count], cols, col_off=col_off, alpha=alpha)
                _abi.call("spv_reduce_slabs", C.byref(rb2), stream_ptr())
                images = [_image(ref["img"], off, count, cols, 2, 3, fmt, scale)] if fmt is not None else []
                _adam_images(ref["p"], ref["g"], ref["m"], ref["v"], images, [], None, ref["t"])
                for b in bufs:
                    b["t"] += 1
                sl = slice(off, off + count)
                what = (nslabs, rows, cols, col_off, t0, fmt, step)
                for k in ("g", "p", "m", "v"):
                    assert torch.equal(_words(fused[k][sl]), _words(ref[k][sl])), (k, what)
                assert torch.equal(fused["img"], ref["img"]), ("image", what)
                if fmt is not None:
                    assert not bool((ref["img"][2:2 + rows, 3:3 + cols] == 0x1234).all()), "the image block was written"
                # the fused launch touches nothing beside the parameter
                for k in ("p", "m", "v"):
                    outside = torch.cat([fused[k][:off], fused[k][off + count:]])
                    want = torch.cat([p0[:off], p0[off + count:]]) if k == "p" else torch.zeros_like(outside)
                    assert torch.equal(outside, want), (k, what)
                assert int(fused["t"]) == t0 + step + 1, "t_dev is only read by the launch"
                assert bool(fused["m"][sl].abs().sum() > 0) and bool(fused["v"][sl].abs().sum() > 0)


@pytest.mark.parametrize("skip", [[], [(4 * 1031 - 1028, 1028)], [(0, 12), (2000, 1000), (4 * 1031 - 24, 24)]])
def test_adam_skip_ranges(dev, skip):
    """spv_adam_step_images with 0, 1 and 3 skipped ranges over n = 4 * 1031 elements (ranges touching both ends of the buffer, one
    inside an imaged parameter): word-equal to the unmasked call outside the ranges, p / m / v / image untouched inside."""
    from spvipes_amd import _abi
    n = 4 * 1031
    gen = torch.Generator(device=dev).manual_seed(len(skip))
    init = dict(p=torch.randn(n, generator=gen, device=dev), m=torch.randn(n, generator=gen, device=dev) * 0.1,
                v=torch.rand(n, generator=gen, device=dev) * 0.01)
    g = torch.randn(n, generator=gen, device=dev)
    ib, ic, icols = 1996, 1100, 11   # an imaged parameter: elements 1996 .. 3095, of which 2000 .. 2999 lie in the middle skipped range
    out = []
    for ranges in ([], skip):
        b = {k: t.clone() for k, t in init.items()}
        b["img"] = torch.full((ic // icols + 2, icols + 5), 0x1234, dtype=torch.int16, device=dev)
        b["ctr"], b["t"] = torch.tensor(5, dtype=torch.int64, device=dev), torch.tensor(3, dtype=torch.int64, device=dev)
        _adam_images(b["p"], g, b["m"], b["v"], [_image(b["img"], ib, ic, icols, 1, 2, _abi.IMAGE_BF16, 1.0)], ranges, b["ctr"], b["t"])
        out.append(b)
    full, masked = out
    inside = torch.zeros(n, dtype=torch.bool, device=dev)
    for b0, c in skip:
        inside[b0:b0 + c] = True
    assert int(inside.sum()) == sum(c for _b, c in skip)
    for k in ("p", "m", "v"):
        assert torch.equal(_words(masked[k])[~inside], _words(full[k])[~inside]), k
        assert torch.equal(_words(masked[k])[inside], _words(init[k])[inside]), k
        assert not torch.equal(full[k], init[k])
    img_in = torch.zeros_like(full["img"], dtype=torch.bool)
    flat_in = inside[ib:ib + ic].view(ic // icols, icols)
    img_in[1:1 + ic // icols, 2:2 + icols] = flat_in
    assert torch.equal(masked["img"][~img_in], full["img"][~img_in])
    assert bool((masked["img"][img_in] == 0x1234).all())
    assert int(masked["ctr"]) == 6 and int(masked["t"]) == 3, "the step counter advances once, t_dev is only read"
    if not skip:
        assert torch.equal(masked["img"], full["img"])


def test_skip_ranges_are_validated(dev):
    from spvipes_amd import _abi
    n = 64
    z = [torch.zeros(n, device=dev) for _ in range(4)]
    for bad in ([(2, 4)], [(0, 6)], [(8, 8), (4, 4)], [(0, 8), (4, 8)], [(60, 8)], [(4 * i, 4) for i in range(0, 2 * (_abi.ADAM_MAX_SKIP + 1), 2)]):
        with pytest.raises(_abi.SpvError):
            _adam_images(*z, [], bad, None, None)
    _adam_images(*z, [], [(0, 8), (56, 8)], None, None)


@pytest.mark.parametrize("B", [128, 256])
@pytest.mark.parametrize("graph", [False, True])
def test_trainer_steps_are_bit_identical_with_the_fused_launch(dev, monkeypatch, B, graph):
    """Three optimiser steps of a tiny bf16 model (G = 301 / 260, H = 32, device RNG on), switch on / off: parameters, Adam moments,
    the flat gradient buffer, the dec_Wm images and every loss are identical; eagerly a step with optimizer_step=False in between
    leaves the parameters alone and gives the same loss either way.  The small-step threshold is lowered to 50 000 elements for the
    test, so that B = 128 takes the small-step pair path on one stream -- where the fused launch is NOT used (nothing to overlap; lab
    notes Y) -- and B = 256 the large-step path, where it is; which path a run took is asserted from its launches.  G = 301: W_m
    (301 rows) and b_m (301) both end off a 4-element boundary, so the skipped range covers their padding and is merged across it."""
    from spvipes_amd import _abi, ops
    from spvipes_amd.data import MinibatchSampler, make_synthetic_group
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd import train
    from spvipes_amd.train import Trainer
    monkeypatch.setattr(ops, "SMALL_STEP_ELEMS", 50_000)
    Gs = (301, 260)
    groups = [make_synthetic_group(g, 512, Gs[g], dev) for g in range(2)]
    calls, FusedWmAdamRanges = [], []
    real_call = _abi.call
    real_ranges = train.FusedWmAdam.ranges
    monkeypatch.setattr(train.FusedWmAdam, "ranges", lambda self: (FusedWmAdamRanges.append(real_ranges(self)), FusedWmAdamRanges[-1])[1])
    monkeypatch.setattr(_abi, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])

    def run(on):
        calls.clear()
        FusedWmAdamRanges.clear()
        monkeypatch.setattr(Trainer, "FUSED_WM_ADAM", on)
        torch.manual_seed(0)
        module = spVIPESmodule({0: Gs[0], 1: Gs[1]}, use_labels=True, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision="bf16").to(dev)
        trainer = Trainer(module, [g.counts for g in groups], labels=[g.labels for g in groups], lr=LR)
        assert trainer.DEVICE_RNG
        module.train()
        batches = list(MinibatchSampler([512, 512], B, dev, seed=0).epoch())[:2] * 2
        if graph:
            trainer.capture(batches[0], warmup=1)
        losses, frozen = [], None
        for i, rows in enumerate(batches[:3]):
            losses.append(float(trainer.step(rows, kl_weight=1.0).loss.detach()))
            if i == 0 and not graph:
                before = trainer.fp.flat.clone()
                losses.append(float(trainer.step(batches[3], kl_weight=1.0, optimizer_step=False).loss.detach()))
                frozen = torch.equal(before, trainer.fp.flat)
        torch.cuda.synchronize()
        assert frozen in (None, True), "optimizer_step=False changed a parameter"
        assert trainer.opt.t == 3 and int(trainer.opt.t_dev) == 3
        n_fused, n_pair = calls.count("spv_reduce_slabs_adam"), calls.count("spv_gemm_bf16_grouped")
        skips = FusedWmAdamRanges[:]
        heads = [(d.mixture.linear.weight.numel(), d.mixture.linear.bias.numel()) for d in (module.decoders[g] for g in range(2))]
        assert heads[0][0] % 4 and heads[0][1] % 4, "group 0's W_m and b_m end off a 4-element boundary"
        sizes = sorted((w + 3) // 4 * 4 + (b_ + 3) // 4 * 4 for w, b_ in heads)
        imgs = [img.clone() for _ws, key, img, _p, _t in trainer._img_specs if key == "dec_Wm"]
        assert len(imgs) == 2
        sd = {k: v.detach().clone() for k, v in module.state_dict().items()}
        return losses, sd, trainer.opt.m.clone(), trainer.opt.v.clone(), trainer.fp.grad.clone(), imgs, n_fused, n_pair, skips, sizes

    a, b = run(True), run(False)
    small = B == 128
    for r in (a, b):   # the path each run took: pair grids (spv_gemm_bf16_grouped) in the small step and only there
        assert (r[7] > 0) == small, (B, r[7])
    want_fused = 0 if small else (1 if graph else 3)
    assert a[6] == want_fused and b[6] == 0, "once per armed backward pass on the large-step path; never on one stream or with the switch off"
    if want_fused:   # per group ONE range: W_m with its padding, merged with b_m and its padding
        for rng in a[8]:
            assert sorted(c for _b, c in rng) == a[9] and all(b0 % 4 == 0 for b0, _c in rng), (rng, a[9])
        assert len(a[8]) == want_fused
    else:
        assert all(rng == [] for rng in a[8])
    assert a[0] == b[0], (a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    for i, what in ((2, "m"), (3, "v"), (4, "grad")):
        assert torch.equal(_words(a[i]), _words(b[i])), what
    for x, y in zip(a[5], b[5]):
        assert torch.equal(x, y), "dec_Wm image"
