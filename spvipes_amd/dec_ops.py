"""The whole decoder side of the step for BOTH groups as one autograd node: latent slicing, BatchNorm
folding of the two factor regressors, mixing trunk, operand packing, logits GEMM, softmax statistics,
NB-mixture likelihood -- and the hand-written backward of all of it.

Reference arithmetic replaced (file:line into /root/reference/src/spVIPES):
    module/spVIPESmodule.py:733-759 (generative), nn/networks.py:314-325 (LinearDecoderSPVIPE.forward),
    module/spVIPESmodule.py:817-824 (reconstruction term of loss)

Launches per step (2 groups): 10 small batched kernels + per group {5 packs, tables, logits GEMM, lse x2,
likelihood} forward; backward per group {softmax fix, 6 GEMMs} + 8 small batched kernels.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _abi
from ._abi import (DEC_CELLS_PER_WG, DEC_NARROW, NB_CMAX, TRUNK_KMAX, SpvBnBatch, SpvDecExpectedArgs, SpvDecExpectedStatsArgs, SpvDecGroup, SpvDecSampleArgs, SpvDecSampleStatsArgs, SpvDecParams, SpvFoldBatch, SpvGemmArgs, SpvReduceBatch, SpvTrunkBatch, SpvZsplitArgs,
                   ptr, round_up, stream_ptr)
from .nn_ops import _add_lin, _first_ws, _fptr, _lin_batch, _linear_bwd, _reduce_pending, _wgrad, grad_out
from . import ops as _ops
from .ops import N_HIDDEN_MIX, GroupCounts, Workspace, _bf16_image, _gemm_slabs, _gene_splits, _nb_cell_tiles, _nb_splits, _pack, fork, group_streams, join

N_DEC_PARAMS = 13  # Wp, gamma_p, beta_p, Ws, gamma_s, beta_s, Wa, ba, gamma_a, beta_a, Wm, bm, px_r
KMP = 320


def _cont(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself if it is contiguous fp32, else such a copy"""
    return t if (t.is_contiguous() and t.dtype == torch.float32) else t.contiguous().float()


def _theta(par) -> torch.Tensor:
    """theta = exp(px_r) of a decoder parameter set (module/spVIPESmodule.py:758)"""
    return torch.exp(_cont(par[12]))


def dec_slots(decoder):
    """the K-slot layout (_abi.DecSlots) a decoder's regressor operand images use: chosen per module (spVIPESmodule decoder_slots)"""
    return getattr(decoder, "dec_slots", DEC_NARROW)


def _slab_cols(KP: int, KS: int):
    """the split-K GEMMs' column problems of the two regressor heads: (column offset in the operand image, columns, head, first column
    of the head): 16 / 32 columns in the narrow layout; the wide layout's 64-column shared head as two 32-column problems (the
    32-column GEMM configuration; the 320-column kernels never see these)"""
    return [(0, KP, 0, 0)] + [(KP + c, 32, 1, c) for c in range(0, KS, 32)]


def decoder_params(dec, px_r) -> List[torch.Tensor]:
    fp, fs, tr, mx = dec.factor_regressor_private, dec.factor_regressor_shared, dec.sigmoid_decoder, dec.mixture
    return [fp.linear.weight, fp.bn.weight, fp.bn.bias, fs.linear.weight, fs.bn.weight, fs.bn.bias,
            tr.linear.weight, tr.linear.bias, tr.bn.weight, tr.bn.bias, mx.linear.weight, mx.linear.bias, px_r]


def _add_red(b: SpvReduceBatch, src: torch.Tensor, nslabs: int, slab_stride: int, ld_src: int, rows: int, cols: int, dst: torch.Tensor,
             ld_dst: int, *, col_off: int = 0, dst_col: int = 0, accumulate: bool = False, alpha=None, exp_scale=None) -> None:
    """one problem of spv_reduce_slabs: dst[r][dst_col + c] (+)= alpha * exp(exp_scale[c]) * sum_s src[s][r][col_off + c]"""
    q = b.p[b.nprob]
    q.src, q.slab_stride, q.ld_src, q.nslabs, q.col_off, q.rows, q.cols = ptr(src), slab_stride, ld_src, nslabs, col_off, rows, cols
    q.dst, q.ld_dst, q.accumulate = dst.data_ptr() + 4 * dst_col, ld_dst, int(accumulate)
    q.alpha, q.exp_scale = ptr(alpha), ptr(exp_scale)
    b.nprob += 1


def _add_heads_red(red: SpvReduceBatch, st: "_DecoderBwd", slabs, dWp: torch.Tensor, dWs: torch.Tensor, sl, alpha) -> None:
    """one group's regressor weight-gradient slabs d [W'_p | c_p], d [W'_s | c_s] (``st.gemm_bc()``) into dWp [G][KP] / dWs [G][KS]"""
    G, KP, KS, KPS = st.G, sl.KP, sl.KS, sl.KPS
    if sl.kslots:   # wide: [(slab, columns, head, first column of the head)] of 32-column problems
        for slab, n, hd, c0 in slabs:
            _add_red(red, slab, st.csp_n, G * n, n, G, n, (dWp, dWs)[hd], (KP, KS)[hd], dst_col=c0, alpha=alpha)
    elif st.fused_heads:   # spv_dec_heads_bwd's slabs: [Gp][48] for both heads, private columns first
        _add_red(red, slabs[0], st.csp_n, st.Gp * KPS, KPS, G, KP, dWp, KP, alpha=alpha)
        _add_red(red, slabs[1], st.csp_n, st.Gp * KPS, KPS, G, KS, dWs, KS, col_off=KP, alpha=alpha)
    else:   # the GEMM slabs [G][16] / [G][32]
        _add_red(red, slabs[0], st.csp_n, G * KP, KP, G, KP, dWp, KP, alpha=alpha)
        _add_red(red, slabs[1], st.csp_n, G * KS, KS, G, KS, dWs, KS, alpha=alpha)


def _run_red(b: SpvReduceBatch) -> None:
    if b.nprob:
        _abi.call("spv_reduce_slabs", C.byref(b), stream_ptr())


def _reduce_adam(b: SpvReduceBatch, params, targets) -> bool:
    """``b``'s problems (problem i sums the gradient of params[i] into targets[i]) as one spv_reduce_slabs_adam launch, where a step
    has armed it (ops.WM_ADAM) and every problem qualifies; False: nothing was launched and the caller runs the plain sum"""
    fa = _ops.WM_ADAM
    if fa is None or not b.nprob or b.nprob != len(params) or b.nprob > _abi.SPV_MAXRA or len(fa.taken) + b.nprob > _abi.ADAM_MAX_SKIP:
        return False   # (the optimiser launch skips at most ADAM_MAX_SKIP ranges: counted before neighbours are merged)
    ba = _abi.SpvReduceAdamBatch()
    ba.nprob = b.nprob
    for i in range(b.nprob):
        q, r = ba.p[i], b.p[i]
        if r.nslabs > 8 or r.accumulate or r.exp_scale or r.ld_dst != r.cols or not fa.fill(q, params[i], targets[i]):
            return False
        q.r = r
    fa.launch(ba, params)
    return True


# ---- one function per argument block: every site that launches with a block gets it from here and sets no field of it itself ----
def _zsplit_args(B: int, Bp: int, n_p: int, n_s: int, n_m: int, sl, lat, zcat, Am_img, Aps_img) -> SpvZsplitArgs:
    """spv_zsplit_fwd's block: per group ``lat`` = (private, poe) latents (contiguous fp32: the caller holds them) into ``zcat`` and, packed
    by the same launch, into the (hi, lo) operand images"""
    za = SpvZsplitArgs()
    za.B, za.n_p, za.n_s, za.ngroups, za.kslots = B, n_p, n_s, len(lat), sl.kslots
    za.ld_am, za.am_col, za.am_cols, za.Bp = KMP, n_m, KMP - n_m, Bp
    for g, (pz, qz) in enumerate(lat):
        za.priv[g], za.poe[g], za.zcat[g] = ptr(pz), ptr(qz), ptr(zcat[g])
        za.am_hi[g], za.am_lo[g], za.aps_hi[g], za.aps_lo[g] = ptr(Am_img[g][0]), ptr(Am_img[g][1]), ptr(Aps_img[g][0]), ptr(Aps_img[g][1])
    return za


def _zstats_batch(B: int, n_p: int, n_s: int, zcat, zsum, zz, trunk=None):
    """the z statistics of the BatchNorm fold as spv_linear_wgrad problems: per group the column sums ``zsum[g][k]`` and z^T z ``zz[g][k]`` of
    the private / shared columns of ``zcat[g]``; ``trunk`` = (zsum_t, zz_t): also those of all its columns (spv_trunk_fold_fwd)"""
    nt = n_p + n_s
    b = _lin_batch(B)
    for g, z in enumerate(zcat):
        for k, (off, n) in enumerate(((0, n_p), (n_p, n_s))):
            _add_lin(b, N=n, K=n, W=ptr(zz[g][k]), X=_fptr(z, off), ldx=nt, dY=_fptr(z, off), lddy=nt, dW=ptr(zz[g][k]), db=ptr(zsum[g][k]))
        if trunk is not None:
            _add_lin(b, N=nt, K=nt, W=ptr(trunk[1][g]), X=ptr(z), ldx=nt, dY=ptr(z), lddy=nt, dW=ptr(trunk[1][g]), db=ptr(trunk[0][g]))
    return b


def _fold_batch(B: int, training: bool, momentum: float, sl) -> SpvFoldBatch:
    fb = SpvFoldBatch()
    fb.nprob, fb.B, fb.training, fb.eps, fb.momentum, fb.kslots = 0, B, int(training), 1e-3, momentum, sl.kslots
    return fb


def _add_fold(fb: SpvFoldBatch, decoder, par, n_p: int, n_s: int, zcat, zsum, zz, fstat, Wps, G: int, Gp: int, sl) -> None:
    """the two regressors of one decoder as problems of spv_bn_fold_fwd: private into columns 0.. of the (hi, lo) image ``Wps``, shared into KP.."""
    for k, (reg, W, gam, bet, off, slot, n, zoff) in enumerate(((decoder.factor_regressor_private, par[0], par[1], par[2], 0, sl.KP, n_p, 0),
                                                                (decoder.factor_regressor_shared, par[3], par[4], par[5], sl.KP, sl.KS, n_s, n_p))):
        q = fb.p[fb.nprob]
        q.W, q.gamma, q.beta, q.running_mean, q.running_var = ptr(W), ptr(gam), ptr(bet), ptr(reg.bn.running_mean), ptr(reg.bn.running_var)
        q.zsum, q.zz, q.z, q.ldz, q.stat = ptr(zsum[k]), ptr(zz[k]), _fptr(zcat, zoff), n_p + n_s, ptr(fstat[k])
        q.img_hi, q.img_lo, q.ld_img, q.col_off, q.slot = ptr(Wps[0]), ptr(Wps[1]), sl.KPS, off, slot
        q.G, q.Gp, q.K = G, Gp, n
        fb.nprob += 1


def _trunk_bn_batch(B: int, training: bool, momentum: float, decoders, par, pre_a, m, tstat, parts, n_m: int, Am_img=None, Bp: int = 0,
                    grads=None) -> SpvBnBatch:
    """the mixing trunks' BatchNorm + rectifier (spv_bn_fwd / spv_bn_bwd), one problem per decoder.  ``Am_img``: per group the (hi, lo) logits
    operand image m is also written into; ``grads`` = (dY, dX, dgamma, dbeta) per-group lists: the backward's fields"""
    bn = SpvBnBatch()
    bn.nprob, bn.B, bn.training, bn.relu, bn.eps, bn.momentum = len(decoders), B, int(training), 1, 1e-3, momentum
    for g, dec in enumerate(decoders):
        tb = dec.sigmoid_decoder.bn
        q = bn.p[g]
        q.X, q.ldx, q.Y, q.ldy, q.gamma, q.beta = ptr(pre_a[g]), n_m, ptr(m[g]), n_m, ptr(par[g][8]), ptr(par[g][9])
        q.running_mean, q.running_var, q.stats, q.N = ptr(tb.running_mean), ptr(tb.running_var), ptr(tstat[g]), n_m
        q.part = ptr(parts[g])
        if Am_img is not None:  # m straight into the logits operand image
            q.img_hi, q.img_lo, q.ld_img, q.img_rows = ptr(Am_img[g][0]), ptr(Am_img[g][1]), KMP, Bp
        if grads is not None:
            q.dY, q.lddy, q.dX, q.lddx, q.dgamma, q.dbeta = ptr(grads[0][g]), n_m, ptr(grads[1][g]), n_m, ptr(grads[2][g]), ptr(grads[3][g])
    return bn


def _trunk_batch(B: int, training: bool, decoders, Wa, par, zsum_t, zz_t, Wf, cf, tstat, n_m: int, nt: int, bwd=None) -> SpvTrunkBatch:
    """spv_trunk_fold_fwd's block, one problem per decoder (``Wa``: its contiguous trunk weights, held by the caller); ``bwd``: per group
    (dWf, dcf, dW, dbias, dgamma, dbeta, dred, z, dz), the further fields of spv_trunk_fold_bwd"""
    tb_ = SpvTrunkBatch()
    tb_.nprob, tb_.B, tb_.training, tb_.eps, tb_.momentum = len(decoders), B, int(training), 1e-3, 0.01
    for g, dec in enumerate(decoders):
        bnm = dec.sigmoid_decoder.bn
        q = tb_.p[g]
        q.W, q.bias, q.gamma, q.beta = ptr(Wa[g]), ptr(par[g][7]), ptr(par[g][8]), ptr(par[g][9])
        q.running_mean, q.running_var = ptr(bnm.running_mean), ptr(bnm.running_var)
        q.zsum, q.zz, q.Wf, q.cf, q.stat, q.N, q.K = ptr(zsum_t[g]), ptr(zz_t[g]), ptr(Wf[g]), ptr(cf[g]), ptr(tstat[g]), n_m, nt
        if bwd is not None:
            q.dWf, q.dcf, q.dW, q.dbias, q.dgamma, q.dbeta, q.dred, q.z, q.dz = (ptr(t) for t in bwd[g])
            q.ldz, q.lddz = nt, nt
    return tb_


def _dec_params(wsg: Workspace, pre: str, B: int, G: int, Bp: int, Gp: int, mlo: bool, sl, logits, Wps, Aps, *, cst=None, tabs=(None, None),
                w_row=None, nb=None, grads=None, grads_f32: bool = False, split_Bp: Optional[int] = None) -> SpvDecParams:
    """one group's spv_dec_params over the workspace arrays named ``pre`` + ...; the read-outs pass none of ``cst`` (the counts), ``tabs``
    (gene_tab, cnt_tab), ``w_row``, ``nb`` = (nb_splits, nb_genes_per_split, nb_cell_tiles: the likelihood kernel's partial rows) and
    ``grads`` = (dtheta_part, dL, tP, tS).  ``split_Bp``: the padded row count whose gene split the softmax statistics take (default: ``Bp``'s
    own) -- the split fixes the order in which spv_dec_lse adds up a row's denominator, so rows gathered out of a minibatch of another
    size keep that minibatch's values bit for bit"""
    splits, per = _gene_splits(split_Bp or Bp, Gp)
    nbs, nbper, nbtiles = nb if nb is not None else (1, 32, 0)
    vec = lambda nme: ptr(wsg.get(pre + nme, (Bp,), torch.float32))
    part = lambda nme: ptr(wsg.get(pre + nme, (splits, Bp), torch.float32))
    nbpart = lambda nme: ptr(wsg.get(pre + nme, (nbs, Bp), torch.float32)) if nb is not None else None
    dth, dL, tP, tS = grads if grads is not None else (None,) * 4
    counts = dict(X=cst.X, ldx=cst.ld, rows=cst.rows, col_off=cst.col_off, count_is_u16=int(cst.dtype == _abi.SPV_COUNT_U16)) if cst is not None else {}
    return SpvDecParams(
        B=B, G=G, Bp=Bp, Gp=Gp, logits=ptr(logits), n_gene_tiles=Gp // 32, logits_f32=int(mlo),
        Wps_hi=ptr(Wps[0]), Wps_lo=ptr(Wps[1]), Aps_hi=ptr(Aps[0]), Aps_lo=ptr(Aps[1]), gene_tab=ptr(tabs[0]), cnt_tab=ptr(tabs[1]),
        lse_p=vec("lse_p"), lse_s=vec("lse_s"), a_p=vec("a_p"), a_s=vec("a_s"), w_row=ptr(w_row), gene_splits=splits, genes_per_split=per,
        part_max_p=part("pmp"), part_sum_p=part("psp"), part_max_s=part("pms"), part_sum_s=part("pss"),
        rec_part=nbpart("rec"), tp_part=nbpart("tp"), ts_part=nbpart("ts"),
        dtheta_part=ptr(dth), dL=ptr(dL), tP=ptr(tP), tS=ptr(tS), grads_f32=int(grads_f32), nb_splits=nbs, nb_genes_per_split=nbper,
        nb_cell_tiles=nbtiles, kslots=sl.kslots, **counts,
    )


class _DecOperands:
    """one group's decoder operand set as ``spv_dec_lse`` leaves it (the inputs of spv_dec_materialize and spv_dec_expected)"""
    __slots__ = ("p", "B", "G", "Bp", "Gp", "Am", "Wm", "par", "keep")


class _DecFront:
    """What the decoder's front end (the ``_front_*`` stages below) leaves for one call over NG groups: one or two in
    ``DecoderFused.forward``, whose backward reads it by name, one in a read-out.  Everything after the sizes is a per-group list."""
    __slots__ = ("dev", "B", "Bp", "Gs", "Gps", "n_p", "n_s", "n_m", "sl", "mlo",   # sizes, K-slot layout, lo planes (fp32 mode)
                 "lat", "zcat", "Am", "Aps",       # contiguous (private, poe) latents; [z_private | z_shared]; (hi, lo) logits / regressor operand images
                 "zsum", "zz", "zsum_t", "zz_t",   # z statistics per head [private, shared]; of all of zcat's columns (folded trunk only, else None)
                 "Wps", "fstat", "fb", "Wm",       # folded regressor image (hi, lo), its statistics per head, the spv_fold_batch; [W_m | b_m] image (hi, lo)
                 "m", "tstat", "pre_a", "Wf", "cf")   # trunk output and statistics; pre-activation (unfolded trunk) or folded weights (folded), else None

    def __init__(self, dev, B: int, Gs, n_p: int, n_s: int, n_m: int, sl, mlo: bool):
        if n_p + 1 > sl.KP or n_s + 1 > sl.KS:
            raise _abi.SpvError(f"decoder kernels support n_private <= {sl.KP - 1} and n_shared <= {sl.KS - 1}")
        if n_m + n_p + n_s + 1 > KMP:
            raise _abi.SpvError("mixture input wider than 320 columns is not supported")
        self.dev, self.B, self.Gs, self.n_p, self.n_s, self.n_m, self.sl, self.mlo = dev, B, list(Gs), n_p, n_s, n_m, sl, mlo
        self.Bp, self.Gps = round_up(B, DEC_CELLS_PER_WG), [round_up(G, 256) for G in Gs]   # 256: the logits GEMM runs 256-gene workgroup tiles
        self.zsum_t = self.zz_t = self.pre_a = self.Wf = self.cf = None   # (what a call does not make stays None)

    def new(self, *shape) -> torch.Tensor:
        return torch.empty(*shape, dtype=torch.float32, device=self.dev)


# ---- the front end's stages over per-group lists (``ws``: one workspace per group), on the caller's current stream.  DecoderFused.forward
# names its workspace arrays "dec_", _prepare_decoder "mat_": a read-out may run between a step's forward and its backward, which reads them ----
def _front_latents(r: _DecFront, lat, ws, pre: str) -> None:
    """latent slicing: zcat = [z_private | z_shared] and, from the same launch, the packed operand images of these latents"""
    NG, nt = len(lat), r.n_p + r.n_s
    r.zcat = [r.new(r.B, nt) for _ in range(NG)]
    r.Am, r.Aps = [_bf16_image(ws[g], pre + "Am", r.Bp, KMP, r.mlo) for g in range(NG)], [_bf16_image(ws[g], pre + "Aps", r.Bp, r.sl.KPS, True) for g in range(NG)]
    r.lat = [(_cont(pz), _cont(qz)) for pz, qz in lat]
    za = _zsplit_args(r.B, r.Bp, r.n_p, r.n_s, r.n_m, r.sl, r.lat, r.zcat, r.Am, r.Aps)
    _abi.call("spv_zsplit_fwd", C.byref(za), stream_ptr())


def _front_zstats(r: _DecFront, training: bool, trunk_fold: bool, ws) -> None:
    """batch statistics of z (column sums and z^T z) for the BatchNorm fold; ``trunk_fold``: the mixing trunk's BatchNorm is folded too
    (spv_trunk_fold_fwd) and needs those of ALL of zcat's columns, cross terms included.  Launched in training mode only"""
    NG, n_p, n_s, nt = len(r.zcat), r.n_p, r.n_s, r.n_p + r.n_s
    r.zsum, r.zz = [[r.new(n_p), r.new(n_s)] for _ in range(NG)], [[r.new(n_p, n_p), r.new(n_s, n_s)] for _ in range(NG)]
    if trunk_fold:
        r.zsum_t, r.zz_t = [r.new(nt) for _ in range(NG)], [r.new(nt, nt) for _ in range(NG)]
    if training:
        _wgrad(_zstats_batch(r.B, n_p, n_s, r.zcat, r.zsum, r.zz, (r.zsum_t, r.zz_t) if trunk_fold else None), _first_ws(ws))


def _front_fold(r: _DecFront, decoders, par, training: bool, momentum: float, ws, pre: str) -> None:
    """the regressors' BatchNorm folded into the packed [Gp][KPS] operand image: builds the block (kept as ``r.fb``: the backward completes it);
    ``_run_fold`` launches it where the caller says.  ``momentum`` 0 leaves the running statistics alone"""
    NG = len(r.zcat)
    r.Wps = [_bf16_image(ws[g], pre + "Wps", r.Gps[g], r.sl.KPS, True) for g in range(NG)]
    r.fstat, r.fb = [[r.new(r.Gs[g], 2), r.new(r.Gs[g], 2)] for g in range(NG)], _fold_batch(r.B, training, momentum, r.sl)
    for g in range(NG):
        _add_fold(r.fb, decoders[g], par[g], r.n_p, r.n_s, r.zcat[g], r.zsum[g], r.zz[g], r.fstat[g], r.Wps[g], r.Gs[g], r.Gps[g], r.sl)


def _run_fold(r: _DecFront) -> None:
    _abi.call("spv_bn_fold_fwd", C.byref(r.fb), stream_ptr())


def _front_wm(r: _DecFront, g: int, par_g, wsg: Workspace, pre: str, reuse: bool):
    """group ``g``'s [W_m | b_m] logits operand image -> (hi, lo), for ``r.Wm`` (per group: the step packs it between the group's other
    side-stream launches).  ``reuse``: skip the pack where the workspace holds the image of these very parameters (Adam has just rewritten it)"""
    Wm_hi, Wm_lo = _bf16_image(wsg, pre + "Wm", r.Gps[g], KMP, r.mlo)
    if not reuse or Wm_lo is not None or wsg.fresh.get(pre + "Wm") != _ops.image_token(par_g[10], par_g[11]):
        _pack(_cont(par_g[10]), Wm_hi, Wm_lo, extra_col=_cont(par_g[11]))
    return Wm_hi, Wm_lo


def _front_trunk(r: _DecFront, decoders, par, training: bool, trunk_fold: bool, momentum: float, ws, part_name: str) -> None:
    """mixing trunk: m = relu(BN(zcat Wa^T + ba)) into ``r.m`` / ``r.tstat`` (the caller's allocations, as is ``r.pre_a`` where it wants that
    ahead of them) AND into the logits operand image.  ``trunk_fold``: the BatchNorm folded into the layer (batch mean / variance of a linear
    map of z from zbar and cov(z)): one affine map + rectifier, no statistics / finalise / normalise launches -- the same mathematics with
    other roundings, so a caller stays with its form.  ``momentum``, ``part_name`` (the BatchNorm partials' workspace array): the unfolded form's"""
    NG, B, n_m, nt = len(r.zcat), r.B, r.n_m, r.n_p + r.n_s
    if trunk_fold:
        r.Wf, r.cf = [r.new(n_m, nt) for _ in range(NG)], [r.new(n_m) for _ in range(NG)]
        wa_c = [_cont(par[g][6]) for g in range(NG)]
        tb_ = _trunk_batch(B, training, decoders, wa_c, par, r.zsum_t, r.zz_t, r.Wf, r.cf, r.tstat, n_m, nt)
        _abi.call("spv_trunk_fold_fwd", C.byref(tb_), stream_ptr())
        b = _lin_batch(B, relu=True)
        for g in range(NG):
            _add_lin(b, N=n_m, K=nt, W=ptr(r.Wf[g]), bias=ptr(r.cf[g]), X=ptr(r.zcat[g]), ldx=nt, Y=ptr(r.m[g]), ldy=n_m,
                     img=(ptr(r.Am[g][0]), ptr(r.Am[g][1]), KMP, r.Bp))
        _abi.call("spv_linear_fwd", C.byref(b), stream_ptr())
        return
    r.pre_a = r.pre_a or [r.new(B, n_m) for _ in range(NG)]
    b = _lin_batch(B)
    for g in range(NG):
        _add_lin(b, N=n_m, K=nt, W=ptr(par[g][6]), bias=ptr(par[g][7]), X=ptr(r.zcat[g]), ldx=nt, Y=ptr(r.pre_a[g]), ldy=n_m)
    _abi.call("spv_linear_fwd", C.byref(b), stream_ptr())
    parts = [ws[g].get(part_name, (-(-B // _abi.BN_ROWS), n_m, 2), torch.float32) for g in range(NG)]
    bn = _trunk_bn_batch(B, training, momentum, decoders, par, r.pre_a, r.m, r.tstat, parts, n_m, r.Am, r.Bp)
    _abi.call("spv_bn_fwd", C.byref(bn), stream_ptr())


class _DecoderBwd:
    """One group's decoder backward launches, as separately schedulable stages (none depends on the upstream gradient of
    the loss: that scalar is applied later by spv_reduce_slabs):
      softmax()  the softmax fix in place on tP / tS; in bf16 mode it also yields the latent gradient of the two rate heads
      gemm_d()   d A_m = dL W_m (contraction over genes): feeds the trunk backward          -- needs only dL
      gemm_bc()  d [W'_p | c_p], d [W'_s | c_s] (contractions over cells): feed the BatchNorm-fold backward -- after softmax()
      gemm_a()   d W_m = dL^T A_m: feeds only the optimiser                                   -- needs only dL
      gemm_ef()  fp32 mode only: the latent gradient of the rate heads as two GEMMs           -- after softmax()
    (Measured: issuing these from the forward pass right after the group's likelihood kernel, staggered so that the other
    group's VALU-bound likelihood kernel runs beside these memory-bound kernels, changes nothing.)"""

    def __init__(self, g: int, P, S, Wps_g, wsg, B: int, Bp: int, G: int, Gp: int, nsplit: int, grads_f32: bool, pair: bool = False, sl=DEC_NARROW):
        self.g, self.P, self.S, self.Wps_g, self.wsg = g, P, S, Wps_g, wsg
        self.B, self.Bp, self.G, self.Gp, self.nsplit, self.grads_f32 = B, Bp, G, Gp, nsplit, grads_f32
        self.sl = sl
        # the wide layout (sl.kslots = 1) runs the in-place softmax fix and the split-K GEMMs: the fused one-pass backward kernels are
        # built for the narrow layout only
        wide = sl.kslots != 0
        self.fused_dz = bool(_ops.FUSED_DZ and not wide)
        self.dz_part = wsg.get("dec_dz_part", (P.gene_splits, Bp, sl.KPS), torch.float32) if self.fused_dz else None
        self.T = T = Gp // 32
        bt = Bp // 32
        # K splits (fp32 slabs, reduced in order by spv_reduce_slabs).  The 320-column GEMMs (d A_m, d W_m) get ~1 workgroup
        # per CU: every extra split adds a [M, 320] fp32 slab to write and to re-read (at C2 8 -> 4 and 4 -> 2 splits:
        # -0.05 ms per step, same-box A/B); the narrow ones (16 / 32 columns) stream their [B,G] operand with ~2 per CU
        self.ksp_m, self.ksp_n = max(1, min(T // 8, -(-256 // max(Bp // 64, 1)))), max(1, min(T // 8, -(-512 // max(Bp // 128, 1))))
        self.csp_m, self.csp_n = max(1, min(bt // 8, -(-256 // max(Gp // 64, 1)))), max(1, min(bt // 8, -(-512 // max(Gp // 128, 1))))
        # bf16 mode: one streaming kernel for both regressor weight gradients (csrc/spv_dec_gemm.h)
        self.heads_dma = bool(nsplit == 1 and not grads_f32 and Bp % 64 == 0 and not wide)
        if self.heads_dma:
            mt, kt = -(-G // 128), Bp // 64   # 128-gene workgroup tiles, two workgroups per CU
            self.csp_n = max(1, min(512 // mt if mt <= 512 else 1, max(kt // 4, 1)))
        # bf16 mode: the regressor weight gradients come out of the softmax-fix pass itself (spv_dec_heads_bwd), one partial slab per
        # 128-cell workgroup row
        self.fused_heads = bool(self.fused_dz and self.heads_dma and Bp % DEC_CELLS_PER_WG == 0)
        # "fp32" mode (split-bf16 gradient words, round 4): the same one-pass kernel on the hi / lo planes -- no in-place fix of the four
        # planes and no register-staged weight-gradient GEMMs re-reading them
        if grads_f32 and nsplit == 3 and self.fused_dz and Bp % DEC_CELLS_PER_WG == 0:
            self.fused_heads = True
        if self.fused_heads:
            self.csp_n = Bp // DEC_CELLS_PER_WG
            self.dw_part = wsg.get("dec_dW48", (self.csp_n, Gp, sl.KPS), torch.float32)   # [d W'_p | d W'_s] rows over the padded genes
        # bf16 mode: the two 320-column GEMMs run the LDS-DMA 128 x 320 kernels, which want their own split counts
        # (d A_m of the two groups of a ``pair`` run side by side, K splits sized so that they share one round of workgroups; d W_m one
        # after the other on the side stream)
        self.ksp_m = self._splits(False, B, G, self.ksp_m, 128 if pair else 256)
        self.csp_m = self._splits(True, G, Bp, self.csp_m)

    def _operand(self, key: str):
        """(hi, lo) operand image of dL / tP / tS: the bf16 tile array itself, or its hi / lo planes in fp32 mode"""
        if not self.grads_f32:
            return self.S[key], None
        t = self.S[key]   # [2 Bp][Gp]: hi plane, lo plane
        return t[:self.Bp], t[self.Bp:]

    def softmax(self):
        if self.fused_heads:
            _abi.call("spv_dec_heads_bwd", C.byref(self.P), ptr(self.S["Tp"]), ptr(self.S["Ts"]), ptr(self.dz_part), ptr(self.dw_part), stream_ptr())
            return
        _abi.call("spv_dec_softmax_bwd", C.byref(self.P), ptr(self.S["Tp"]), ptr(self.S["Ts"]), ptr(self.dz_part), stream_ptr())

    @staticmethod
    def _dma_splits(M: int, K: int, cus: int = 256) -> int:
        """K splits for the LDS-DMA 128 x 320 kernels (csrc/spv_dec_gemm.h): the count that minimises
        rounds-of-``cus``-workgroups x (64-deep steps per split + ~4 steps of prologue / slab store).  ``cus`` = 128 for a launch that
        runs beside its twin of the other group on a second stream (one workgroup per CU: the pair then shares ONE round)."""
        mt, kt = -(-M // 128), -(-K // 64)
        best, best_cost = 1, None
        for s_ in range(1, 17):
            if s_ > 1 and kt // s_ < 4:
                break
            cost = -(-(mt * s_) // cus) * (-(-kt // s_) + 4)
            if best_cost is None or cost < best_cost:
                best, best_cost = s_, cost
        return best

    def _splits(self, a_kmajor: bool, M: int, K: int, default: int, cus: int = 256) -> int:
        if _abi.load().spv_gemm_bf16_uses_dma(int(a_kmajor), M, KMP, K, self.nsplit, self.T, KMP):
            return self._dma_splits(M, K, cus)
        return default

    def gemm_d(self):
        (Wm_hi, Wm_lo), (dL_hi, dL_lo) = self.S["Wm"], self._operand("dL")
        return _gemm_slabs(False, dL_hi, dL_lo, self.Gp, Wm_hi, Wm_lo, KMP, self.B, KMP, self.G, self.nsplit,
                           self.ksp_m, self.wsg, "dec_dAm", a_tiles=self.T)

    def gemm_bc(self):
        if self.fused_heads:   # already produced by softmax() (spv_dec_heads_bwd): hand the partial slabs to the reduction
            return self.dw_part, self.dw_part   # (one 48-column slab: the reductions below pick their columns)
        (Aps_hi, Aps_lo), (tP_hi, tP_lo), (tS_hi, tS_lo) = self.S["Aps"], self._operand("tP"), self._operand("tS")
        KP, KS, KPS = self.sl.KP, self.sl.KS, self.sl.KPS
        if self.heads_dma:   # bf16 mode: both heads in one LDS-DMA streaming pass (csrc/spv_dec_gemm.h)
            b = self.wsg.get("dec_dWp", (self.csp_n, self.G, KP), torch.float32)
            c = self.wsg.get("dec_dWs", (self.csp_n, self.G, KS), torch.float32)
            _abi.call("spv_dec_heads_wgrad", ptr(tP_hi), ptr(tS_hi), self.T, ptr(Aps_hi), self.G, self.Bp, self.csp_n, ptr(b), ptr(c), stream_ptr())
            return b, c
        if self.sl.kslots:   # wide: [(slab, columns, head, first column of the head)] of 32-column problems
            return [(_gemm_slabs(True, (tP_hi, tS_hi)[hd], (tP_lo, tS_lo)[hd], self.Gp, Aps_hi, Aps_lo, KPS, self.G, n, self.Bp, self.nsplit, self.csp_n,
                                 self.wsg, f"dec_dW{off}", b_col_off=off, a_tiles=self.T), n, hd, c0) for off, n, hd, c0 in _slab_cols(KP, KS)]
        b = _gemm_slabs(True, tP_hi, tP_lo, self.Gp, Aps_hi, Aps_lo, KPS, self.G, KP, self.Bp, self.nsplit, self.csp_n, self.wsg, "dec_dWp", a_tiles=self.T)
        c = _gemm_slabs(True, tS_hi, tS_lo, self.Gp, Aps_hi, Aps_lo, KPS, self.G, KS, self.Bp, self.nsplit, self.csp_n, self.wsg, "dec_dWs",
                        b_col_off=KP, a_tiles=self.T)
        return b, c

    def gemm_a(self):
        (Am_hi, Am_lo), (dL_hi, dL_lo) = self.S["Am"], self._operand("dL")
        return _gemm_slabs(True, dL_hi, dL_lo, self.Gp, Am_hi, Am_lo, KMP, self.G, KMP, self.Bp, self.nsplit,
                           self.csp_m, self.wsg, "dec_dWm", a_tiles=self.T)

    def gemm_args(self, which: str, a: "SpvGemmArgs") -> torch.Tensor:
        """fill ``a`` with the spv_gemm_bf16 arguments of gemm_d ("d") / gemm_a ("a") for spv_gemm_bf16_grouped; returns the slab tensor"""
        (dL_hi, dL_lo) = self._operand("dL")
        if which == "d":
            (B_hi, B_lo), kmaj, M, K, splits, name = self.S["Wm"], 0, self.B, self.G, self.ksp_m, "dec_dAm"
        else:
            (B_hi, B_lo), kmaj, M, K, splits, name = self.S["Am"], 1, self.G, self.Bp, self.csp_m, "dec_dWm"
        out = self.wsg.get(name, (splits, M, KMP), torch.float32)
        a.a_kmajor, a.A_hi, a.A_lo, a.lda = kmaj, ptr(dL_hi), ptr(dL_lo), self.Gp
        a.B_hi, a.B_lo, a.ldb, a.C, a.ldc = ptr(B_hi), ptr(B_lo) if B_lo is not None else None, KMP, ptr(out), KMP
        a.M, a.N, a.K, a.nsplit, a.splits, a.a_tiles, a.slab_stride = M, KMP, K, self.nsplit, splits, self.T, M * KMP
        return out

    def gemm_ef(self):
        (tP_hi, tP_lo), (tS_hi, tS_lo) = self._operand("tP"), self._operand("tS")
        KP, KS, KPS = self.sl.KP, self.sl.KS, self.sl.KPS
        if self.sl.kslots:   # wide: [(slab, columns, head, first column of the head)] of 32-column problems
            return [(_gemm_slabs(False, (tP_hi, tS_hi)[hd], (tP_lo, tS_lo)[hd], self.Gp, self.Wps_g[0], self.Wps_g[1], KPS, self.B, n, self.G, self.nsplit,
                                 self.ksp_n, self.wsg, f"dec_dA{off}", b_col_off=off, a_tiles=self.T), n, hd, c0) for off, n, hd, c0 in _slab_cols(KP, KS)]
        e = _gemm_slabs(False, tP_hi, tP_lo, self.Gp, self.Wps_g[0], self.Wps_g[1], KPS, self.B, KP, self.G, self.nsplit, self.ksp_n, self.wsg, "dec_dAp", a_tiles=self.T)
        f = _gemm_slabs(False, tS_hi, tS_lo, self.Gp, self.Wps_g[0], self.Wps_g[1], KPS, self.B, KS, self.G, self.nsplit, self.ksp_n, self.wsg, "dec_dAs",
                        b_col_off=KP, a_tiles=self.T)
        return e, f


def _trunk_bwd(r: _DecFront, decoders, par, training: bool, ws, pg, dAm, d_zcat):
    """DecoderFused.backward's trunk tail (BatchNorm + relu, Linear) from ``dAm`` = d m, in the form the forward took.  ``pg``: per group and
    parameter (kernel target, autograd return); ``d_zcat``: per group the gradient reaching zcat so far, which both tails add to.  Returns
    its temporaries: the caller holds them to the end of the pass, so that no later array of the pass takes their memory"""
    NG, B, n_m, nt, new = len(r.zcat), r.B, r.n_m, r.n_p + r.n_s, r.new
    dWa, dba, d_gam_a, d_bet_a = ([pg[g][j][0] for g in range(NG)] for j in (6, 7, 8, 9))
    if r.Wf is not None:
        # folded trunk (spv_trunk_fold_fwd): the layer is relu(zcat W'^T + c'); its input gradient and the gradients of (W', c') come from the
        # rectifier-masked linear kernels, spv_trunk_fold_bwd takes (d W', d c') back to W_a / gamma / beta and adds the part of d zcat that
        # flows through the batch statistics -- the three BatchNorm-backward launches are gone from this chain
        dWf, dcf = [new(n_m, nt) for _ in range(NG)], [new(n_m) for _ in range(NG)]
        dred = [new(-(-n_m // 64), nt + nt * nt) for _ in range(NG)]
        bw, bd = _lin_batch(B, relu=True), _lin_batch(B, relu=True, accumulate=True)
        for g in range(NG):
            _add_lin(bw, N=n_m, K=nt, W=ptr(r.Wf[g]), X=ptr(r.zcat[g]), ldx=nt, Y=ptr(r.m[g]), ldy=n_m, dY=ptr(dAm[g]), lddy=n_m, dW=ptr(dWf[g]), db=ptr(dcf[g]))
            _add_lin(bd, N=n_m, K=nt, W=ptr(r.Wf[g]), Y=ptr(r.m[g]), ldy=n_m, dY=ptr(dAm[g]), lddy=n_m, dX=ptr(d_zcat[g]), lddx=nt)
        if _ops.LINEAR_BWD:   # one launch; spv_trunk_fold_bwd reads the summed d W', so the slice sum stays on the chain
            _reduce_pending(_linear_bwd(bd, bw, _first_ws(ws), "wgrad_part_trunk"))
        else:
            _abi.call("spv_linear_dgrad", C.byref(bd), stream_ptr())
            _wgrad(bw, _first_ws(ws))
        wa_c = [par[g][6] if par[g][6].is_contiguous() else par[g][6].contiguous() for g in range(NG)]
        tb_ = _trunk_batch(B, training, decoders, wa_c, par, r.zsum_t, r.zz_t, r.Wf, r.cf, r.tstat, n_m, nt,
                           bwd=list(zip(dWf, dcf, dWa, dba, d_gam_a, d_bet_a, dred, r.zcat, d_zcat)))
        _abi.call("spv_trunk_fold_bwd", C.byref(tb_), stream_ptr())
        return dWf, dcf, dred, wa_c
    d_pre = [new(B, n_m) for _ in range(NG)]
    parts = [ws[g].get("trunk_bn_part", (-(-B // _abi.BN_ROWS), n_m, 2), torch.float32) for g in range(NG)]
    bn = _trunk_bn_batch(B, training, 0.01, decoders, par, r.pre_a, r.m, r.tstat, parts, n_m, grads=(dAm, d_pre, d_gam_a, d_bet_a))
    _abi.call("spv_bn_bwd", C.byref(bn), stream_ptr())
    bw, bd = _lin_batch(B), _lin_batch(B, accumulate=True)
    for g in range(NG):
        _add_lin(bw, N=n_m, K=nt, W=ptr(par[g][6]), X=ptr(r.zcat[g]), ldx=nt, dY=ptr(d_pre[g]), lddy=n_m, dW=ptr(dWa[g]), db=ptr(dba[g]))
        _add_lin(bd, N=n_m, K=nt, W=ptr(par[g][6]), dY=ptr(d_pre[g]), lddy=n_m, dX=ptr(d_zcat[g]), lddx=nt)
    if _ops.LINEAR_BWD:
        _reduce_pending(_linear_bwd(bd, bw, _first_ws(ws), "wgrad_part_trunk"))
    else:
        _wgrad(bw, _first_ws(ws))
        _abi.call("spv_linear_dgrad", C.byref(bd), stream_ptr())
    return d_pre


def _fold_bwd(r: _DecFront, training: bool, ws, pg, dWp, dWs, d_zcat, joins):
    """BatchNorm-fold backward (+ the z statistics it used) from the folded weights' gradients ``dWp`` / ``dWs``, then the latent slicing
    backward -> (d private, d poe) per group.  It completes the block the forward built and kept (``r.fb``), so that the two launches
    cannot disagree on the forward's half; ``joins()`` runs once the block is complete, ahead of the launch (the schedule's waits)"""
    NG, B, n_p, n_s, nt, sl = len(r.zcat), r.B, r.n_p, r.n_s, r.n_p + r.n_s, r.sl
    d_priv, d_poe = [r.new(B, n_p) for _ in range(NG)], [r.new(B, n_s) for _ in range(NG)]
    for g in range(NG):
        for k, (dweff, ld, n, zoff) in enumerate(((dWp[g], sl.KP, n_p, 0), (dWs[g], sl.KS, n_s, n_p))):
            q = r.fb.p[2 * g + k]   # (_add_fold's order)
            q.dWeff, q.ld_dw, q.dz, q.lddz = ptr(dweff), ld, _fptr(d_zcat[g], zoff), nt
            q.dW, q.dgamma, q.dbeta = (ptr(pg[g][3 * k + j][0]) for j in range(3))   # parameters 0-2: private W, gamma, beta; 3-5: shared
            q.red_part = ptr(ws[g].get(f"fold_red_{k}", (-(-r.Gs[g] // 256) + 1, n + n * n), torch.float32))
            if training:   # the latent-slicing backward rides in the same kernel (spv_fold_prob.out_priv)
                q.zcol, q.out_priv, q.out_poe, q.n_p, q.n_s = zoff, ptr(d_priv[g]), ptr(d_poe[g]), n_p, n_s
    joins()
    _abi.call("spv_bn_fold_bwd", C.byref(r.fb), stream_ptr())
    if not training:   # (training: already done by the z-statistics kernel of spv_bn_fold_bwd)
        za = SpvZsplitArgs()
        za.B, za.n_p, za.n_s, za.ngroups = B, n_p, n_s, NG
        for g in range(NG):
            za.d_zcat[g], za.d_priv[g], za.d_poe[g] = ptr(d_zcat[g]), ptr(d_priv[g]), ptr(d_poe[g])
        _abi.call("spv_zsplit_bwd", C.byref(za), stream_ptr())
    return d_priv, d_poe


class DecoderFused(torch.autograd.Function):
    """inputs : per group (private_log_z [B,n_p], poe_log_z [B,n_s]), per group its 13 parameters, then n_kl KL
             vectors [B] (module/spVIPESmodule.py:841-868) that the loss adds with weight kl_weight / B
    outputs: (loss, sum_g sum_b w_b rec_gb, rec_0 [B][, rec_1 [B]])   -- all but loss detached; one or two groups per call
    ``w_pad``: the per-cell weights of the reconstruction term, length >= Bp, zero beyond B.
    ``klw``  : 0-dim fp32 device tensor (read at run time: a captured graph sees later updates)."""

    @staticmethod
    def forward(ctx, counts: Sequence[GroupCounts], rows, B: int, decoders, library: Sequence[torch.Tensor], w_pad: torch.Tensor,
                training: bool, nsplit: int, ws: Sequence[Workspace], klw: torch.Tensor, n_kl: int, *tensors):
        NG = len(counts)   # one or two groups per call (the batched kernels carry two slots; spVIPESmodule.loss chunks more)
        if NG not in (1, 2):
            raise _abi.SpvError("DecoderFused takes one or two groups per call")
        ctx.set_materialize_grads(False)
        lat = [(tensors[2 * g], tensors[2 * g + 1]) for g in range(NG)]
        par = [tensors[2 * NG + g * N_DEC_PARAMS: 2 * NG + (g + 1) * N_DEC_PARAMS] for g in range(NG)]
        kls = [_cont(t) for t in tensors[2 * NG + NG * N_DEC_PARAMS:]]
        if len(kls) != n_kl or n_kl > 4:
            raise _abi.SpvError("DecoderFused: expected n_kl <= 4 KL vectors after the parameters")
        dev = lat[0][0].device
        n_p, n_s, n_m, mlo = lat[0][0].shape[1], lat[0][1].shape[1], par[0][6].shape[0], nsplit == 3
        sl = dec_slots(decoders[0])
        if any(dec_slots(d) != sl for d in decoders):
            raise _abi.SpvError("DecoderFused: the decoders of one call must share their operand layout")
        need_grad = any(ctx.needs_input_grad)  # (grad mode is off inside Function.forward)
        r = _DecFront(dev, B, [c.G for c in counts], n_p, n_s, n_m, sl, mlo)
        Bp, Gs, Gps, new = r.Bp, r.Gs, r.Gps, r.new
        # ---- 1.-3. latent slicing, the z statistics, the regressors' BatchNorm fold (built here, launched on the side stream below) ----
        _front_latents(r, lat, ws, "dec_")
        trunk_fold = bool(_ops.TRUNK_FOLD and n_p + n_s <= TRUNK_KMAX and n_m <= 256)
        _front_zstats(r, training, trunk_fold, ws)
        _front_fold(r, decoders, par, training, 0.01, ws, "dec_")
        # the schedule of this call AND of its backward pass (ops.DecSchedule): decided here, once
        grads_f32 = bool(need_grad and mlo)
        sched = _ops.dec_schedule(B, Gs, NG, grads_f32)
        pair = sched.pair   # both groups' per-group launches as one grid per kernel (ops.DEC_PAIR)
        # The fold, the mixture-weight images and the (count, gene) tables depend on nothing the trunk (step 4) computes:
        # they run beside it on a side stream and are joined before the per-group section.
        side = group_streams(dev, 3, sched.serial)[2]
        side.wait_stream(torch.cuda.current_stream(dev))
        r.Wm, tabs = [], []
        with torch.cuda.stream(side):
            _run_fold(r)
            for g in range(NG):
                r.Wm.append(_front_wm(r, g, par[g], ws[g], "dec_", reuse=True))
                gene_tab = ws[g].get("dec_gene_tab", (Gps[g], 4), torch.float32)
                cnt_tab = ws[g].get("dec_cnt_tab", (NB_CMAX, Gps[g], 2), torch.float32)
                if not pair:
                    _abi.call("spv_dec_tables", ptr(_cont(par[g][12])), Gs[g], Gps[g], ptr(gene_tab), ptr(cnt_tab), stream_ptr())
                tabs.append((gene_tab, cnt_tab))
            if pair:   # one grid for both groups' tables
                tg = (SpvDecGroup * NG)()
                px_keep = [_cont(par[g][12]) for g in range(NG)]
                for g in range(NG):
                    tg[g].px_r, tg[g].p.G, tg[g].p.Gp, tg[g].p.gene_tab, tg[g].p.cnt_tab = ptr(px_keep[g]), Gs[g], Gps[g], ptr(tabs[g][0]), ptr(tabs[g][1])
                _abi.call("spv_dec_tables_grouped", tg, NG, stream_ptr())
        # ---- 4. mixing trunk: m = relu(BN(zcat Wa^T + ba)) -------------------------------------------
        r.m, r.tstat = [new(B, n_m) for _ in range(NG)], [new(n_m, 2) for _ in range(NG)]
        _front_trunk(r, [decoders[g] for g in range(NG)], par, training, trunk_fold, 0.01, ws, "trunk_bn_part")
        # ---- 5. per group: operand images, tables, logits GEMM, softmax statistics, likelihood ------
        if w_pad.numel() < Bp or w_pad.dtype != torch.float32 or not w_pad.is_contiguous():
            raise _abi.SpvError("DecoderFused: w_pad must be contiguous fp32 of length >= round_up(B, 128)")
        # bf16 mode: one bf16 array per gradient; fp32 mode: a bf16 hi plane followed by a bf16 lo plane ([2 Bp][Gp] rows):
        # the two operand images the split-bf16 GEMMs consume, written directly by the likelihood kernel
        gdt, gname, gplanes = (torch.int16, "split", 2) if grads_f32 else (torch.int16, "bf16", 1)
        P, saved_g = [], []
        rec = [new(B) for _ in range(NG)]  # (allocated before the fork: every temporary belongs to the main stream)
        red = SpvReduceBatch()
        red.nprob = 0
        torch.cuda.current_stream(dev).wait_stream(side)
        streams = group_streams(dev, NG, sched.serial) if not pair else [torch.cuda.current_stream(dev)] * NG
        fork(streams)
        dgrp = (SpvDecGroup * NG)() if pair else None
        lib_keep = []
        for g in range(NG):
          with torch.cuda.stream(streams[g]):
              G, Gp, wsg = Gs[g], Gps[g], ws[g]
              Wm_hi, Wm_lo = r.Wm[g]
              (Am_hi, Am_lo), (Aps_hi, Aps_lo) = r.Am[g], r.Aps[g]
              logits = wsg.get("dec_logits_" + ("f32" if mlo else "f16"), (Bp, Gp), torch.float32 if mlo else torch.float16)
              lse_first = g % 2 == 1  # group 1 runs its (VALU-bound) softmax statistics beside group 0's logits GEMM
              run_logits = lambda: _abi.call("spv_dec_logits", ptr(Am_hi), ptr(Am_lo), ptr(Wm_hi), ptr(Wm_lo), KMP, Bp, Gp, nsplit, ptr(logits), int(mlo), stream_ptr())
              if not lse_first and not pair:
                  run_logits()
              nbs, nbper = _nb_splits(Gp, Bp)
              nbpart = lambda nme: wsg.get(nme, (nbs, Bp), torch.float32)
              if need_grad:
                  dL = wsg.get("dec_dL_" + gname, (gplanes * Bp, Gp), gdt, zero=True)
                  tP = wsg.get("dec_tP_" + gname, (gplanes * Bp, Gp), gdt, zero=True)
                  tS = wsg.get("dec_tS_" + gname, (gplanes * Bp, Gp), gdt, zero=True)
                  dth = wsg.get("dec_dtheta", (Bp // 64, Gp), torch.float32, zero=True)
                  Tp, Ts = wsg.get("dec_Tp", (Bp,), torch.float32), wsg.get("dec_Ts", (Bp,), torch.float32)
              else:
                  dL = tP = tS = dth = Tp = Ts = None
              p = _dec_params(wsg, "dec_", B, G, Bp, Gp, mlo, sl, logits, r.Wps[g], r.Aps[g], cst=counts[g].c_struct(rows[g]), tabs=tabs[g], w_row=w_pad,
                              nb=(nbs, nbper, _nb_cell_tiles(Bp, Gp)), grads=(dth, dL, tP, tS), grads_f32=grads_f32)
              if pair:
                  lib_keep.append(_cont(library[g].flatten()))
                  q = dgrp[g]
                  q.p, q.library = p, ptr(lib_keep[-1])
                  q.Am_hi, q.Am_lo, q.Wm_hi, q.Wm_lo, q.K, q.nsplit = ptr(Am_hi), ptr(Am_lo), ptr(Wm_hi), ptr(Wm_lo), KMP, nsplit
              else:
                  _abi.call("spv_dec_lse", C.byref(p), ptr(_cont(library[g].flatten())), stream_ptr())
                  if lse_first:
                      run_logits()
                  _abi.call("spv_dec_nb_fwd", C.byref(p), int(need_grad), stream_ptr())
              _add_red(red, nbpart("dec_rec"), nbs, Bp, Bp, 1, B, rec[g], B)
              if need_grad:
                  _add_red(red, nbpart("dec_tp"), nbs, Bp, Bp, 1, Bp, Tp, Bp)
                  _add_red(red, nbpart("dec_ts"), nbs, Bp, Bp, 1, Bp, Ts, Bp)
              P.append(p)
              if need_grad:
                  saved_g.append(dict(Wm=(Wm_hi, Wm_lo), Am=(Am_hi, Am_lo), Aps=(Aps_hi, Aps_lo), dL=dL, tP=tP, tS=tS, dth=dth, Tp=Tp, Ts=Ts))
        join(streams)
        if pair:   # logits GEMM, softmax statistics and likelihood of both groups: one grid each
            _abi.call("spv_dec_logits_grouped", dgrp, NG, stream_ptr())
            _abi.call("spv_dec_lse_grouped", dgrp, NG, stream_ptr())
            _abi.call("spv_dec_nb_fwd_grouped", dgrp, NG, int(need_grad), stream_ptr())
        _run_red(red)
        loss, rec_sum, gkl = new(()), new(()), new(B)
        klp = (C.c_void_p * 4)(*[ptr(k) for k in kls], *([None] * (4 - n_kl)))
        _abi.call("spv_loss_assemble", ptr(rec[0]), ptr(rec[1]) if NG > 1 else None, ptr(w_pad), klp, n_kl, B, ptr(klw), ptr(loss), ptr(rec_sum), ptr(gkl), stream_ptr())
        if need_grad:
            ctx.P, ctx.saved_g, ctx.ws, ctx.decoders, ctx.training, ctx.nsplit = P, saved_g, ws, decoders, training, nsplit
            ctx.NG, ctx.front, ctx.sched = NG, r, sched
            ctx.grads_f32, ctx.done, ctx.gkl, ctx.n_kl = grads_f32, False, gkl, n_kl
            ctx.save_for_backward(*tensors[:2 * NG + NG * N_DEC_PARAMS])
        ctx.mark_non_differentiable(rec_sum, *rec)
        return (loss, rec_sum, *rec)

    @staticmethod
    def backward(ctx, g_loss, *_g_rec):
        if ctx.done:
            raise _abi.SpvError("DecoderFused.backward may run once per forward (gradient buffers are consumed in place)")
        ctx.done = True
        NG, tensors = ctx.NG, ctx.saved_tensors
        par = [tensors[2 * NG + g * N_DEC_PARAMS: 2 * NG + (g + 1) * N_DEC_PARAMS] for g in range(NG)]
        r, ws, nsplit, training = ctx.front, ctx.ws, ctx.nsplit, ctx.training
        B, Bp, Gs, Gps, n_p, n_s, n_m, sl, dev, new = r.B, r.Bp, r.Gs, r.Gps, r.n_p, r.n_s, r.n_m, r.sl, r.dev, r.new
        nt, KM = n_p + n_s, n_m + n_p + n_s + 1
        if g_loss is None:
            raise _abi.SpvError("DecoderFused.backward: the loss output received no gradient")
        g_loss = g_loss if (g_loss.dtype == torch.float32 and g_loss.is_contiguous()) else g_loss.float().contiguous()
        pg = [[grad_out(par[g][j]) for j in range(N_DEC_PARAMS)] for g in range(NG)]  # (kernel target, autograd return) per parameter
        red, red2 = SpvReduceBatch(), SpvReduceBatch()
        red.nprob = red2.nprob = 0
        DEC_KP, DEC_KS, DEC_KPS = sl.KP, sl.KS, sl.KPS
        dWp, dWs = [new(Gs[g], DEC_KP) for g in range(NG)], [new(Gs[g], DEC_KS) for g in range(NG)]
        dAm, d_zcat = [new(B, n_m) for _ in range(NG)], [new(B, nt) for _ in range(NG)]
        # ---- schedule ---------------------------------------------------------------------------------------------
        # The d A_m GEMMs go first, group g's on group stream g: the critical chain (trunk / fold / PoE / encoder backward) needs only
        # d A_m up to the point where the latent gradient of the rate heads joins (red2).  The HBM-bound one-pass softmax / heads
        # kernels run on the side stream, then the regressor weight-gradient reductions (first needed by the BatchNorm-fold backward,
        # which sits behind the ~15 small launches of the trunk backward) and the mixture-weight GEMMs (which feed only the
        # optimiser), beside the trunk / PoE / encoder-tail backward chain; the side stream is joined at the end of the backward
        # pass (train.Trainer, DEFER_JOIN) or before returning.  Everything the switches and the step shape decide was fixed by
        # the forward pass (ctx.sched): nothing here asks ops for it again.
        sched = ctx.sched
        cur = torch.cuda.current_stream(dev)
        streams = group_streams(dev, NG, sched.serial)
        side = group_streams(dev, 3, sched.serial)[2]
        stages = [_DecoderBwd(g, ctx.P[g], ctx.saved_g[g], r.Wps[g], ws[g], B, Bp, Gs[g], Gps[g], nsplit, ctx.grads_f32, pair=(NG == 2), sl=sl) for g in range(NG)]
        d_slabs, ef_slabs = [None] * NG, [None] * NG
        # without a second stream, or where the softmax fix does not yield the latent gradient (wide layout, ops.FUSED_DZ off), the
        # softmax kernels stay ahead of the d A_m GEMMs on the group streams
        da_first = side is not cur and all(st.fused_dz for st in stages)
        sm_done = None
        wm_late = bool(sched.wm_late and side is not cur)
        # ops.DEC_PAIR: the per-group launches (d A_m GEMMs, one-pass backward, d W_m GEMMs) as one grid per kernel
        pair = bool(sched.pair and all(st.fused_heads and not st.grads_f32 for st in stages))

        def pair_gemm(which):
            ga = (SpvGemmArgs * NG)()
            outs = [stages[g].gemm_args(which, ga[g]) for g in range(NG)]
            _abi.call("spv_gemm_bf16_grouped", ga, NG, stream_ptr())
            return outs

        def pair_heads_bwd():
            hg = (SpvDecGroup * NG)()
            for g in range(NG):
                st = stages[g]
                hg[g].p, hg[g].Tp, hg[g].Ts, hg[g].dz_part, hg[g].dw_part = st.P, ptr(st.S["Tp"]), ptr(st.S["Ts"]), ptr(st.dz_part), ptr(st.dw_part)
            _abi.call("spv_dec_heads_bwd_grouped", hg, NG, stream_ptr())

        if pair:
            streams = [cur] * NG
            if not da_first:   # (single stream: the one-pass backward first, as the per-group schedule orders it)
                pair_heads_bwd()
            d_slabs = pair_gemm("d")
        fork(streams)
        for g in range(0 if pair else NG):
            with torch.cuda.stream(streams[g]):
                if not da_first:
                    stages[g].softmax()
                d_slabs[g] = stages[g].gemm_d()
                if not stages[g].fused_dz:
                    ef_slabs[g] = stages[g].gemm_ef()
        join(streams)
        side.wait_stream(cur)   # (before the reductions: the side work needs none of them)
        if da_first:
            with torch.cuda.stream(side):
                if pair:
                    pair_heads_bwd()
                else:
                    for st in stages:
                        st.softmax()
                sm_done = torch.cuda.Event()
                sm_done.record(side)
        # slab sums, scaled by the upstream gradient, straight into their consumers' buffers
        al = g_loss
        for g in range(NG):
            st, G, Gp = stages[g], Gs[g], Gps[g]
            _add_red(red, d_slabs[g], st.ksp_m, B * KMP, KMP, B, n_m, dAm[g], n_m, alpha=al)                          # d m (trunk output)
            # gradient reaching zcat directly: through the logits GEMM (columns n_m..) and the two regressors
            _add_red(red, d_slabs[g], st.ksp_m, B * KMP, KMP, B, nt, d_zcat[g], nt, col_off=n_m, alpha=al)
            if st.fused_dz:
                _add_red(red2, st.dz_part, st.P.gene_splits, Bp * DEC_KPS, DEC_KPS, B, n_p, d_zcat[g], nt, accumulate=True, alpha=al)
                _add_red(red2, st.dz_part, st.P.gene_splits, Bp * DEC_KPS, DEC_KPS, B, n_s, d_zcat[g], nt, col_off=DEC_KP, dst_col=n_p, accumulate=True, alpha=al)
            elif sl.kslots:   # wide: 32-column slabs; head hd's columns c0 .. c0 + 31 go to d zcat columns (0 | n_p) + c0 ..
                for slab, n, hd, c0 in ef_slabs[g]:
                    cols = min(n, (n_p, n_s)[hd] - c0)
                    if cols > 0:
                        _add_red(red2, slab, st.ksp_n, B * n, n, B, cols, d_zcat[g], nt, dst_col=(0, n_p)[hd] + c0, accumulate=True, alpha=al)
            else:
                _add_red(red2, ef_slabs[g][0], st.ksp_n, B * DEC_KP, DEC_KP, B, n_p, d_zcat[g], nt, accumulate=True, alpha=al)
                _add_red(red2, ef_slabs[g][1], st.ksp_n, B * DEC_KS, DEC_KS, B, n_s, d_zcat[g], nt, dst_col=n_p, accumulate=True, alpha=al)
            # d px_r = exp(px_r) * d theta (theta = exp(px_r): module/spVIPESmodule.py:758)
            _add_red(red, ctx.saved_g[g]["dth"], -(-(Bp // 64) // _nb_cell_tiles(Bp, Gp)), Gp, Gp, 1, G, pg[g][12][0], G, alpha=al, exp_scale=par[g][12])
        gk = None
        if ctx.n_kl:  # d loss / d kl_i[b] = g * kl_weight / B for every KL vector: rides in the second reduction launch
            gk = new(B)
            _add_red(red2, ctx.gkl, 1, B, B, 1, B, gk, B, alpha=g_loss)
        _run_red(red)
        if not da_first:
            _run_red(red2)
        # side stream: the regressor weight gradients (the main stream picks them up with an event before
        # spv_bn_fold_bwd), then the mixture-weight gradients (2 x [G, K_M] from dL^T A_m, the largest GEMMs of the backward
        # pass, which feed nothing but the optimiser)
        bc_done = None
        with torch.cuda.stream(side):
            red_bc = SpvReduceBatch()
            red_bc.nprob = 0
            for g in range(NG):
                _add_heads_red(red_bc, stages[g], stages[g].gemm_bc(), dWp[g], dWs[g], sl, g_loss)
            _run_red(red_bc)
            if side is not cur:
                bc_done = torch.cuda.Event()
                bc_done.record(side)

        def issue_wm(after=None):
            with torch.cuda.stream(side):
                if after is not None:
                    side.wait_event(after)
                red3 = SpvReduceBatch()
                red3.nprob = 0
                wm_slabs = pair_gemm("a") if pair else None
                for g in range(NG):
                    st, G = stages[g], Gs[g]
                    a = wm_slabs[g] if pair else st.gemm_a()
                    _add_red(red3, a, st.csp_m, G * KMP, KMP, G, KM - 1, pg[g][10][0], KM - 1, alpha=g_loss)                 # d W_m
                    _add_red(red3, a, st.csp_m, G * KMP, KMP, G, 1, pg[g][11][0], 1, col_off=KM - 1, alpha=g_loss)           # d b_m
                # Nothing but the optimiser reads these gradients, and nothing launched after this point in the step reads W_m, b_m or
                # their image (the logits GEMM and the d A_m GEMMs, their only readers, are behind side.wait_stream(cur) above): in a step
                # that ends with the optimiser the same launch takes their Adam step (train.FusedWmAdam) -- in large
                # steps.  A small step (sched.pair: pair grids, everything on the caller's stream) would overlap the launch with nothing and
                # only save the optimiser's 4-byte re-read of the gradient, for a one-element-per-thread kernel in place of the optimiser's
                # 16-byte one: measured slower at C1 (lab notes Y), so the plain sum stays there.  (SPV_SERIAL_STREAMS=1, the per-kernel
                # profiling mode of a large step, keeps the fused launch: the profile then shows the kernels the step runs.)
                if sched.pair or not _reduce_adam(red3, [par[g][j] for g in range(NG) for j in (10, 11)],
                                                   [pg[g][j][0] for g in range(NG) for j in (10, 11)]):
                    _run_red(red3)
            if _ops.DEFER_JOIN:
                _ops.defer(side, [g_loss])
            else:
                cur.wait_stream(side)

        # WM_LATE: the mixture-weight GEMMs are held back until the main stream reaches the BatchNorm-fold backward: they then run beside
        # the ~25 tiny launches of the fold / PoE / encoder-tail backward, where the GPU is otherwise almost idle, instead of beside the
        # trunk backward, which they slow down
        if not wm_late:
            issue_wm()
        held = _trunk_bwd(r, [ctx.decoders[g] for g in range(NG)], par, training, ws, pg, dAm, d_zcat)   # noqa: F841  (see _trunk_bwd)

        def joins():   # what the main stream picks up between building the BatchNorm-fold backward's block and launching it
            if da_first:   # the rate heads' latent gradient (softmax fix on the side stream) joins d_zcat here
                cur.wait_event(sm_done)
                _run_red(red2)
            if bc_done is not None:
                cur.wait_event(bc_done)
            if wm_late:
                ev = torch.cuda.Event()
                ev.record(cur)
                issue_wm(ev)

        d_priv, d_poe = _fold_bwd(r, training, ws, pg, dWp, dWs, d_zcat, joins)
        grads = [t for g in range(NG) for t in (d_priv[g], d_poe[g])] + [pg[g][j][1] for g in range(NG) for j in range(N_DEC_PARAMS)]
        return (None,) * 11 + tuple(grads) + (gk,) * ctx.n_kl


@torch.no_grad()
def _prepare_decoder(decoder, px_r: torch.Tensor, private_log_z: torch.Tensor, poe_log_z: torch.Tensor, library: torch.Tensor,
                     training: bool, nsplit: int, ws: Workspace, par=None, *, logits: bool, split_rows: Optional[int] = None) -> _DecOperands:
    """ONE group's decoder operands outside autograd: the front end of ``DecoderFused.forward`` (the ``_front_*`` stages) over a
    workspace of its own names ("mat_"), with momentum 0 (batch statistics in training mode, WITHOUT touching the running statistics)
    and always the unfolded mixing trunk (whose roundings define the read-outs' values); then the tiled logits GEMM (``logits``: only
    spv_dec_materialize reads that array) and the softmax statistics over all G genes (spv_dec_lse).  Shared by every read-out.
    ``split_rows``: the size of the minibatch whose gene split spv_dec_lse takes (``_dec_params``: ``split_Bp``); None = this call's
    own row count."""
    par = list(par) if par is not None else decoder_params(decoder, px_r)   # (``par``: spVIPESmodule._decoder_operands' covariate-extended set)
    pz, qz = _cont(private_log_z), _cont(poe_log_z)
    B, G, n_m, mlo = pz.shape[0], par[0].shape[0], par[6].shape[0], nsplit == 3
    r = _DecFront(private_log_z.device, B, [G], pz.shape[1], qz.shape[1], n_m, dec_slots(decoder), mlo)
    _front_latents(r, [(pz, qz)], [ws], "mat_")
    _front_zstats(r, training, False, [ws])
    _front_fold(r, [decoder], [par], training, 0.0, [ws], "mat_")
    _run_fold(r)
    r.Wm = [_front_wm(r, 0, par, ws, "mat_", reuse=False)]
    r.pre_a, r.m, r.tstat = [r.new(B, n_m)], [r.new(B, n_m)], [r.new(n_m, 2)]
    _front_trunk(r, [decoder], [par], training, False, 0.0, [ws], "mat_bn_part")
    Bp, Gp, (Am_hi, Am_lo), (Wm_hi, Wm_lo) = r.Bp, r.Gps[0], r.Am[0], r.Wm[0]
    tiled = None
    if logits:
        tiled = ws.get("mat_logits_" + ("f32" if mlo else "f16"), (Bp, Gp), torch.float32 if mlo else torch.float16)
        _abi.call("spv_dec_logits", ptr(Am_hi), ptr(Am_lo), ptr(Wm_hi), ptr(Wm_lo), KMP, Bp, Gp, nsplit, ptr(tiled), int(mlo), stream_ptr())
    p = _dec_params(ws, "mat_", B, G, Bp, Gp, mlo, r.sl, tiled, r.Wps[0], r.Aps[0], split_Bp=None if split_rows is None else round_up(int(split_rows), DEC_CELLS_PER_WG))
    lib = _cont(library.flatten())
    if lib.numel() != B:
        raise _abi.SpvError("decoder: the library vector must hold one value per cell")
    _abi.call("spv_dec_lse", C.byref(p), ptr(lib), stream_ptr())
    o = _DecOperands()
    o.p, o.B, o.G, o.Bp, o.Gp, o.Am, o.Wm, o.par, o.keep = p, B, G, Bp, Gp, r.Am[0], r.Wm[0], par, (pz, qz, lib)
    return o


@torch.no_grad()
def materialize_decoder(decoder, px_r: torch.Tensor, private_log_z: torch.Tensor, poe_log_z: torch.Tensor, library: torch.Tensor,
                        training: bool, nsplit: int, ws: Workspace, par=None) -> dict:
    """The decoder outputs the reference's ``generative`` returns for ONE group (module/spVIPESmodule.py:751-768,
    nn/networks.py:314-325): {"px_scale_private", "px_scale_shared", "px_rate_private", "px_rate_shared", "px_mixing"}
    as fp32 [B, G] tensors + "px_r" = exp(px_r).  The training step never needs them (the fused likelihood kernel consumes
    the same quantities in registers); this runs the same operand preparation as ``DecoderFused.forward`` for one group
    (``_prepare_decoder``) and then ``spv_dec_materialize``."""
    o = _prepare_decoder(decoder, px_r, private_log_z, poe_log_z, library, training, nsplit, ws, par, logits=True)
    B, G = o.B, o.G
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=private_log_z.device)
    out = {k: new(B, G) for k in ("px_scale_private", "px_scale_shared", "px_rate_private", "px_rate_shared", "px_mixing")}
    _abi.call("spv_dec_materialize", C.byref(o.p), ptr(out["px_scale_private"]), ptr(out["px_scale_shared"]), ptr(out["px_rate_private"]),
              ptr(out["px_rate_shared"]), ptr(out["px_mixing"]), G, stream_ptr())
    out["px_r"] = _theta(o.par)
    return out


def _gene_selection(genes, G: int, dev, who: str):
    """``genes`` of expected_expression / sample_counts -> (int32 device tensor of ids or None for all genes in order, n_genes)"""
    if genes is None:
        gidx, n = None, G
    elif isinstance(genes, torch.Tensor) and genes.is_cuda:
        if genes.dtype != torch.int32 or genes.dim() != 1 or not genes.is_contiguous():
            raise _abi.SpvError(f"{who}: a device gene list must be a contiguous 1-d int32 tensor")
        gidx, n = genes, int(genes.numel())
    else:
        host = np.asarray(genes.cpu() if isinstance(genes, torch.Tensor) else genes)
        if host.ndim != 1 or (host.size and not np.issubdtype(host.dtype, np.integer)):
            raise TypeError(f"{who}: genes must be a 1-d sequence of integer gene positions")
        bad = np.nonzero((host < 0) | (host >= G))[0]
        if bad.size:
            raise IndexError(f"gene position {int(host[bad[0]])} is out of range for a group of {G} genes")
        gidx, n = torch.as_tensor(host.astype(np.int32), device=dev), int(host.size)
    if n <= 0:
        raise ValueError(f"{who}: the gene selection is empty")
    return gidx, n


def _readout_operands(decoder, px_r, private_log_z, poe_log_z, library, training, nsplit, ws, par, genes, library_size, who: str,
                      log_library: Optional[torch.Tensor] = None, split_rows: Optional[int] = None):
    """the shared prelude of expected_expression / sample_counts / sample_count_stats: ``library_size`` override of the library,
    operand preparation without the tiled logits, gene selection -> (_DecOperands, gene ids or None, n_genes).  ``log_library``: a
    per-cell fp32 device vector [B] of LOG library sizes that wins over ``library_size`` (-inf: a cell whose rates are all 0)."""
    from .data import expression_log_library

    logL = expression_log_library(library_size)
    B = private_log_z.shape[0]
    if log_library is not None:
        if (not isinstance(log_library, torch.Tensor) or not log_library.is_cuda or log_library.dtype != torch.float32 or log_library.dim() != 1
                or log_library.numel() != B or not log_library.is_contiguous()):
            raise _abi.SpvError(f"{who}: the library override must be a contiguous fp32 device vector with one log library size per cell ({B})")
        lib = log_library
    else:
        lib = library if logL is None else torch.full((B,), logL, dtype=torch.float32, device=private_log_z.device)
    o = _prepare_decoder(decoder, px_r, private_log_z, poe_log_z, lib, training, nsplit, ws, par, logits=False, split_rows=split_rows)
    return (o, *_gene_selection(genes, o.G, private_log_z.device, who))


def _fill_readout(a, o: _DecOperands, nsplit: int, gidx, n: int) -> None:
    """the fields SpvDecExpectedArgs and SpvDecSampleArgs share: logits operand images, their width, the gene selection"""
    a.Am_hi, a.Am_lo, a.Wm_hi, a.Wm_lo, a.K, a.nsplit = ptr(o.Am[0]), ptr(o.Am[1]), ptr(o.Wm[0]), ptr(o.Wm[1]), KMP, nsplit
    a.genes, a.n_genes = ptr(gidx), n


@torch.no_grad()
def expected_expression(decoder, px_r: torch.Tensor, private_log_z: torch.Tensor, poe_log_z: torch.Tensor, library: torch.Tensor,
                        training: bool, nsplit: int, ws: Workspace, par=None, *, genes=None, what="mixture", library_size="latent",
                        out: Optional[torch.Tensor] = None, alpha: float = 1.0, accumulate: bool = False) -> torch.Tensor:
    """The mean of ONE group's NB mixture, or one of its ingredients, over a selection of genes as fp32 [B, n_genes]
    (spv_dec_expected; nn/networks.py:314-325, module/spVIPESmodule.py:751-759):
        what = "mixture"  pi * rate_private + (1 - pi) * rate_shared,   "private"  pi * rate_private,
               "shared"   (1 - pi) * rate_shared,                       "mixing"   pi = sigmoid(mixing logits)
    ``genes``: None (all G genes in order), an int32 device tensor of ids in [0, G) (taken as checked: the kernel clamps ids, it
    does not report them), or any host sequence of integers (checked here: IndexError names the first offender); any order,
    repeats allowed.  ``library_size``: "latent" (exp(``library``)) or a positive number L (rate = L * softmax).
    ``out``: fp32 device tensor [>= B, >= n_genes] with unit column stride to write into (rows >= B and columns >= n_genes stay
    untouched); ``out = alpha * value`` or, with ``accumulate``, ``out += alpha * value``.  Same operand preparation as
    ``materialize_decoder``; the softmax denominators always run over all G genes."""
    from .data import expression_what

    code = expression_what(what)
    o, gidx, n = _readout_operands(decoder, px_r, private_log_z, poe_log_z, library, training, nsplit, ws, par, genes, library_size, "expected_expression")
    B, dev = o.B, private_log_z.device
    if out is None:
        if accumulate:
            raise ValueError("expected_expression: accumulate=True needs the ``out`` array to add to")
        out = torch.empty((B, n), dtype=torch.float32, device=dev)
    elif (not out.is_cuda or out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] < B or out.shape[1] < n
          or (out.shape[1] > 1 and out.stride(1) != 1) or (out.shape[0] > 1 and out.stride(0) < n)):
        raise _abi.SpvError(f"expected_expression: out must be an fp32 device tensor [>= {B}, >= {n}] with unit column stride")
    a = SpvDecExpectedArgs()
    _fill_readout(a, o, nsplit, gidx, n)
    a.what, a.out, a.ld_out, a.alpha, a.accumulate = code, ptr(out), (out.stride(0) if out.shape[0] > 1 else max(out.shape[1], n)), float(alpha), int(bool(accumulate))
    _abi.call("spv_dec_expected", C.byref(o.p), C.byref(a), stream_ptr())
    return out[:B, :n]


def sample_key(seed: int) -> int:
    """the 64-bit Philox key of a user seed: the seed in the low word, a fixed tag in the high word (so that the count sampler's
    key space is not the one spv_randn is keyed from for the same seed)"""
    return ((0x53504C43 << 32) | (int(seed) & 0xFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF


def _check_stream(key, sample, who: str) -> None:
    """``key`` / ``sample`` of the count sampler's entry points: integers in [0, 2^64) / [0, 2^32), else ValueError"""
    if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) < 1 << 64:
        raise ValueError(f"{who}: key must be an integer in [0, 2^64), got {key!r}")
    if isinstance(sample, bool) or not isinstance(sample, (int, np.integer)) or not 0 <= int(sample) < 1 << 32:
        raise ValueError(f"{who}: sample must be an integer in [0, 2^32), got {sample!r}")


def _check_cell_ids(cell_ids, B: int, who: str) -> None:
    if cell_ids is not None and (not isinstance(cell_ids, torch.Tensor) or not cell_ids.is_cuda or cell_ids.dtype != torch.int32 or cell_ids.dim() != 1
                                 or cell_ids.numel() < B or not cell_ids.is_contiguous()):
        raise _abi.SpvError(f"{who}: cell_ids must be a contiguous int32 device tensor of at least {B} entries")


@torch.no_grad()
def sample_counts(decoder, px_r: torch.Tensor, private_log_z: torch.Tensor, poe_log_z: torch.Tensor, library: torch.Tensor,
                  training: bool, nsplit: int, ws: Workspace, par=None, *, genes=None, library_size="latent", key: int = 0, sample: int = 0,
                  cell_ids: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One draw per (cell, selected gene) from ONE group's NB mixture as int32 [B, n_genes] (spv_dec_sample;
    module/spVIPESmodule.py:751-759): c ~ Bernoulli(pi), lam ~ Gamma(theta, (c ? rate_private : rate_shared) / theta) clamped at
    1e8, x ~ Poisson(lam), with the rates, pi and theta = exp(px_r) of ``expected_expression`` (same operand preparation, same
    ``genes`` and ``library_size`` handling, same honouring of ``training``).  The random bits of an element depend on
    (``key``, gene id, cell id, ``sample``) only: ``cell_ids`` (int32 device tensor [B]; None = the row number) names the cells,
    ``sample`` (0 .. 2^32 - 1) the draw, ``key`` (0 .. 2^64 - 1) the stream.  ``out``: int32 device tensor to write into, either
    [>= B, >= n_genes] with unit column stride or [>= B, >= n_genes, S] viewed at one sample (``out3[:, :, s]``: column stride S);
    rows >= B, columns >= n_genes and the other samples' elements stay untouched."""
    _check_stream(key, sample, "sample_counts")
    o, gidx, n = _readout_operands(decoder, px_r, private_log_z, poe_log_z, library, training, nsplit, ws, par, genes, library_size, "sample_counts")
    B, dev = o.B, private_log_z.device
    _check_cell_ids(cell_ids, B, "sample_counts")
    if out is None:
        out = torch.empty((B, n), dtype=torch.int32, device=dev)
    elif (not out.is_cuda or out.dtype != torch.int32 or out.dim() != 2 or out.shape[0] < B or out.shape[1] < n
          or (out.shape[1] > 1 and out.stride(1) < 1) or (out.shape[0] > 1 and out.stride(0) < (n - 1) * max(out.stride(1), 1) + 1)):
        raise _abi.SpvError(f"sample_counts: out must be an int32 device tensor [>= {B}, >= {n}] (a [B, n, S] array viewed at one sample is fine)")
    theta = _theta(o.par)
    ld_gene = out.stride(1) if out.shape[1] > 1 else 1
    a = SpvDecSampleArgs()
    _fill_readout(a, o, nsplit, gidx, n)
    a.ld_gene, a.theta, a.cell_ids = ld_gene, ptr(theta), ptr(cell_ids)
    a.key, a.sample = int(key), int(sample)
    a.out, a.ld_out = ptr(out), (out.stride(0) if out.shape[0] > 1 else (n - 1) * ld_gene + 1)
    _abi.call("spv_dec_sample", C.byref(o.p), C.byref(a), stream_ptr())
    return out[:B, :n]


SAMPLE_STATS = ("sum", "non_zeros", "sum_squares", "max")   # the rows of spv_dec_sample_stats' table
_U64 = tuple(t for t in (torch.int64, getattr(torch, "uint64", None)) if t is not None)   # 64-bit integer storage of either signedness


def check_sample_stats_tables(B: int, n: int, seg, n_seg, stats, cell_total, who: str = "sample_count_stats") -> int:
    """The dtype / shape / contiguity checks of ``sample_count_stats``' tables for a minibatch of ``B`` cells and ``n`` selected genes
    -> n_seg.  Pure host code: it looks at tensor metadata only."""
    if isinstance(n_seg, bool) or not isinstance(n_seg, (int, np.integer)) or int(n_seg) < 1:
        raise ValueError(f"{who}: n_seg must be a positive integer, got {n_seg!r}")
    n_seg = int(n_seg)
    if seg is not None and (not isinstance(seg, torch.Tensor) or not seg.is_cuda or seg.dtype != torch.int32 or seg.dim() != 1 or seg.numel() < B
                            or not seg.is_contiguous()):
        raise _abi.SpvError(f"{who}: seg must be a contiguous int32 device tensor of at least {B} segment codes")
    if (not isinstance(stats, torch.Tensor) or not stats.is_cuda or stats.dtype not in _U64 or stats.dim() != 3 or stats.shape[0] != n_seg
            or stats.shape[1] != len(SAMPLE_STATS) or stats.shape[2] < n or not stats.is_contiguous()):
        raise _abi.SpvError(f"{who}: stats must be a contiguous 64-bit integer device tensor [{n_seg}, {len(SAMPLE_STATS)}, >= {n}]")
    if cell_total is not None and (not isinstance(cell_total, torch.Tensor) or not cell_total.is_cuda or cell_total.dtype not in _U64
                                   or cell_total.dim() != 1 or cell_total.numel() < B or not cell_total.is_contiguous()):
        raise _abi.SpvError(f"{who}: cell_total must be a contiguous 64-bit integer device tensor of at least {B} entries")
    return n_seg


@torch.no_grad()
def sample_count_stats(decoder, px_r: torch.Tensor, private_log_z: torch.Tensor, poe_log_z: torch.Tensor, library: torch.Tensor,
                       training: bool, nsplit: int, ws: Workspace, par=None, *, genes=None, library_size="latent", log_library=None,
                       key: int = 0, sample: int = 0, cell_ids: Optional[torch.Tensor] = None, seg: Optional[torch.Tensor] = None,
                       n_seg: int = 1, stats: torch.Tensor, cell_total: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sample_counts``' draws for ONE group's minibatch, reduced inside the kernel instead of stored (spv_dec_sample_stats;
    module/spVIPESmodule.py:751-759): with x[b, j] the integer ``sample_counts`` returns for the same operands, ``genes``,
    ``library_size``, ``key``, ``sample`` and ``cell_ids``,

        stats[k, 0, j] += sum x    stats[k, 1, j] += #(x > 0)    stats[k, 2, j] += sum x^2 (modulo 2^64)    stats[k, 3, j] = max(., max x)

    over the cells b with ``seg[b] == k``, and ``cell_total[b] += sum_j x[b, j]``.  ``seg``: int32 device tensor [>= B] of codes in
    [0, n_seg), None = every cell in segment 0; a cell with a negative code (or one >= n_seg) is neither drawn nor counted.
    ``stats``: 64-bit integer device tensor [n_seg, 4, >= n_genes] (torch.int64 holds the same bits as uint64: view it on the
    host), ``cell_total``: [>= B] or None.  Everything ACCUMULATES with integer atomics: zero the tables once, then one table
    collects every sample of every minibatch, equal bit for bit to the reduction of the stored draws; columns >= n_genes, rows of
    segments without a counted cell and totals of cells that are not counted stay untouched.  ``log_library``: a per-cell fp32
    device vector [B] of log library sizes that wins over ``library_size``.  One launch; nothing of size cells x genes is written.
    Returns ``stats``."""
    who = "sample_count_stats"
    _check_stream(key, sample, who)
    o, gidx, n = _readout_operands(decoder, px_r, private_log_z, poe_log_z, library, training, nsplit, ws, par, genes, library_size, who,
                                   log_library=log_library)
    B = o.B
    _check_cell_ids(cell_ids, B, who)
    n_seg = check_sample_stats_tables(B, n, seg, n_seg, stats, cell_total, who)
    theta = _theta(o.par)
    a = SpvDecSampleStatsArgs()
    _fill_readout(a, o, nsplit, gidx, n)
    a.theta, a.cell_ids, a.key, a.sample = ptr(theta), ptr(cell_ids), int(key), int(sample)
    a.seg, a.n_seg, a.stats, a.ld_stats, a.cell_total = ptr(seg), n_seg, ptr(stats), stats.stride(1), ptr(cell_total)
    _abi.call("spv_dec_sample_stats", C.byref(o.p), C.byref(a), stream_ptr())
    return stats


EXPECTED_STATS = ("sum_mixture", "sum_private", "sum_shared", "sum_mixing", "sq_mixture", "sq_private", "sq_shared", "sq_mixing")   # the rows of spv_dec_expected_stats' table
EXPRESSION_TILE = 32   # cells per tile of spv_dec_expected_stats' tile arrays (one workgroup)


def check_expected_stats_tables(B: int, n: int, tile_seg, tile_n, n_seg, stats, who: str = "expected_expression_stats") -> int:
    """The dtype / device / shape / contiguity checks of ``expected_expression_stats``' tables for ``B`` operand rows and ``n`` selected
    genes -> n_seg.  Pure host code: it looks at tensor metadata only."""
    if isinstance(n_seg, bool) or not isinstance(n_seg, (int, np.integer)) or int(n_seg) < 1:
        raise ValueError(f"{who}: n_seg must be a positive integer, got {n_seg!r}")
    n_seg, n_tiles = int(n_seg), -(-B // EXPRESSION_TILE)
    for name, t in (("tile_seg", tile_seg), ("tile_n", tile_n)):
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or t.numel() < n_tiles or not t.is_contiguous()):
            raise _abi.SpvError(f"{who}: {name} must be a contiguous int32 device tensor with one entry per {EXPRESSION_TILE}-row tile ({n_tiles})")
    if (not isinstance(stats, torch.Tensor) or not stats.is_cuda or stats.dtype != torch.float64 or stats.dim() != 3 or stats.shape[0] != n_seg
            or stats.shape[1] != len(EXPECTED_STATS) or stats.shape[2] < n or not stats.is_contiguous()):
        raise _abi.SpvError(f"{who}: stats must be a contiguous fp64 device tensor [{n_seg}, {len(EXPECTED_STATS)}, >= {n}]")
    if tile_seg.device != stats.device or tile_n.device != stats.device:
        raise _abi.SpvError(f"{who}: tile_seg, tile_n and stats must live on one device")
    return n_seg


@torch.no_grad()
def expected_expression_stats(decoder, px_r: torch.Tensor, private_log_z: torch.Tensor, poe_log_z: torch.Tensor, library: torch.Tensor,
                              training: bool, nsplit: int, ws: Workspace, par=None, *, genes=None, library_size="latent", log_library=None,
                              tile_seg: torch.Tensor, tile_n: torch.Tensor, n_seg: int, stats: torch.Tensor, batch_rows: Optional[int] = None) -> torch.Tensor:
    """``expected_expression``'s four values for ONE group's minibatch, reduced per segment inside the entry point instead of stored
    (spv_dec_expected_stats): with v_w[b, j] the fp32 value ``expected_expression(..., what=w)`` returns for the same operands,
    ``genes`` and ``library_size`` (w = mixture, private, shared, mixing),

        stats[k, w, j] += sum v_w[b, j]        stats[k, 4 + w, j] += sum v_w[b, j] ** 2

    over the counted rows b of segment k, every term widened to fp64 first.  The rows arrive ARRANGED BY SEGMENT (``data.
    expression_tile_plan``): ``tile_seg`` / ``tile_n`` are int32 device tensors with one entry per 32-row tile of the operands --
    tile t belongs to segment ``tile_seg[t]`` (a negative code or one >= n_seg skips the tile) and its first ``tile_n[t]`` rows count;
    the rest are padding.  ``stats``: fp64 device tensor [n_seg, 8, >= n_genes].  Everything ACCUMULATES in a fixed order without
    floating-point atomics: zero the table once, then one table collects a whole walk, and two identical sequences of calls agree bit
    for bit; columns >= n_genes and rows of segments without a counted tile stay untouched.  The per-tile partial sums live in the
    group's ``Workspace`` ([tiles, 8, n_genes] fp64).  ``log_library``: a per-cell fp32 device vector [B] of log library sizes that
    wins over ``library_size``.  ``batch_rows``: the size of the minibatch the rows were gathered from (None: this call's own row
    count).  The softmax denominators over all G genes are added up in gene splits whose number follows the padded row count; with
    ``batch_rows`` they take the split of that minibatch, so every value equals ``expected_expression``'s on the ungathered minibatch
    bit for bit however many padding rows the arrangement added.  Eval mode only: padding rows would enter the batch statistics of
    training mode, and the tile layout assumes that every row is its own computation.  Nothing of size cells x genes is written.
    Returns ``stats``."""
    who = "expected_expression_stats"
    if training:
        raise _abi.SpvError(f"{who}: eval mode only (in training mode the padding rows would enter the BatchNorm batch statistics)")
    if batch_rows is not None and (isinstance(batch_rows, bool) or not isinstance(batch_rows, (int, np.integer)) or int(batch_rows) < 1):
        raise ValueError(f"{who}: batch_rows must be a positive integer, got {batch_rows!r}")
    o, gidx, n = _readout_operands(decoder, px_r, private_log_z, poe_log_z, library, training, nsplit, ws, par, genes, library_size, who,
                                   log_library=log_library, split_rows=batch_rows)
    n_seg = check_expected_stats_tables(o.B, n, tile_seg, tile_n, n_seg, stats, who)
    n_tiles = o.Bp // EXPRESSION_TILE
    need = int(_abi.load().spv_dec_expected_stats_ws_bytes(n, n_tiles))
    part = ws.get("mat_xstats", (1 << max(need // 8 - 1, 0).bit_length(),), torch.float64)   # a power of two: the tile count changes from step to step
    a = SpvDecExpectedStatsArgs()
    _fill_readout(a, o, nsplit, gidx, n)
    a.n_seg, a.tile_seg, a.tile_n, a.stats, a.ld_stats, a.ws = n_seg, ptr(tile_seg), ptr(tile_n), ptr(stats), stats.stride(1), ptr(part)
    _abi.call("spv_dec_expected_stats", C.byref(o.p), C.byref(a), stream_ptr())
    return stats


@torch.no_grad()
def nbmix_sample(rate_p: torch.Tensor, rate_s: torch.Tensor, logit: torch.Tensor, theta: torch.Tensor, *, key: int = 0, sample: int = 0,
                 cell_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [R, G] draws of the NB mixture over given fp32 device parameters [R, G] (``theta``: [G]) -- spv_nbmix_sample, the
    sampler of ``sample_counts`` with gene id = column and cell id = ``cell_ids[row]`` (None: the row number)"""
    R, G = rate_p.shape
    for t in (rate_p, rate_s, logit):
        if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (R, G) or not t.is_contiguous():
            raise _abi.SpvError("nbmix_sample: the parameters must be contiguous fp32 device tensors of one shape [R, G]")
    if not theta.is_cuda or theta.dtype != torch.float32 or tuple(theta.shape) != (G,) or not theta.is_contiguous():
        raise _abi.SpvError("nbmix_sample: theta must be a contiguous fp32 device tensor [G]")
    if cell_ids is not None and (not cell_ids.is_cuda or cell_ids.dtype != torch.int32 or tuple(cell_ids.shape) != (R,) or not cell_ids.is_contiguous()):
        raise _abi.SpvError("nbmix_sample: cell_ids must be a contiguous int32 device tensor [R]")
    out = torch.empty((R, G), dtype=torch.int32, device=rate_p.device)
    _abi.call("spv_nbmix_sample", ptr(rate_p), ptr(rate_s), ptr(logit), G, ptr(theta), R, G, ptr(cell_ids), int(key), int(sample), ptr(out), G, stream_ptr())
    return out
