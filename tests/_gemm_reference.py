"""Float64 references, exactness predicates, error bounds, operand builders and a mutable float32 model for the decoder's MFMA GEMM entry
points (include/spvipes_hip.h: spv_gemm_bf16, spv_gemm_bf16_fix, spv_gemm_bf16_grouped, spv_dec_heads_wgrad, spv_dec_logits[_grouped];
kernels in spvipes_amd/csrc/spv_dec_gemm.h and spv_gemm.h).  Test infrastructure only: no product file imports this.

What the kernels compute, and why it can be checked exactly
  nsplit 1:  C = sum_k a_hi b_hi                                   every product of two bf16 values is exact in fp32
  nsplit 3:  C = sum_k (a_hi b_lo + a_lo b_hi + a_hi b_hi)         (mfma32_split, spv_common.h); lo x lo is NOT part of the definition and
                                                                   the lo plane is an independent operand
Tier 1 ("lattice"): operands are small integers times a power of two, chosen so that EVERY partial sum of the terms, in any order, is a
  multiple of the granularity below 2^24 granules (fp32 output) or at most 2^11 (f16 output): any correct kernel then returns the exact
  value whatever its summation order, and any missing, doubled, misplaced or extra term changes it.  `sums_are_exact` asserts that on the
  reference before a case may be compared under equality.
Tier 2 (real values): N(0, 1) fp32 values split into hi / lo planes as spv_pack_bf16 does.  Bound per element 2 U n S, U = 2^-24, n = the
  number of terms accumulated into the element (K or 3 K of the slab's range, plus the slab adds where slabs are summed), S = the sum of
  their absolute values: valid for ANY summation order with one ulp (not half) lost per add -- the guide documents round-to-nearest chains
  for the f32 MFMA only.  An f16 output adds 2^-11 |value| + half the smallest f16 subnormal; an alpha that is no power of two adds one U.
  `cap_ok`: the bound stays below 1e-3 of the largest reference value of the case, so it cannot hide a wrong kernel.

Every operand array is laid out with its contract padding ZERO and a guard beyond the contract extent (one further tile row / K tile /
image row) filled with bf16 NaN words: a kernel that reads more than the header lets it read returns NaN.  Every output sits in a frame of
CANARY words (columns >= N where ldc > N, one row after the last of every slab, a tail after the last tiled tile) that must come back
untouched.  `model_*` emulate the entry points in numpy float32 ON THE WORDS the device receives, with named value mutations
(MUTATIONS): tests/test_gemm_reference_cpu.py shows that every mutation is caught by the comparisons the GPU tests make."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
NAN_WORD = 0x7FC0
CANARY = -12352.0   # representable in bf16 and f16
CAP = 1e-3


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ---- bf16 words ---------------------------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> the nearest bf16 value (ties to even), as float32; finite inputs"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(x.shape)


def bf16_words(x):
    """float32 values that ARE bf16 values -> their 16-bit words"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    assert not (u & 0xFFFF).any(), "not a bf16 value"
    return (u >> 16).astype(np.uint16).reshape(x.shape)


def words_f32(w):
    w = np.ascontiguousarray(w, dtype=np.uint16)
    return (w.astype(np.uint32) << 16).view(np.float32).reshape(w.shape)


def split_bf16(x):
    """hi = bf16(x), lo = bf16(x - hi) (split_bf16 of spv_common.h, what spv_pack_bf16 stores)"""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_round(x)
    return hi, bf16_round(x - hi)


# ---- accumulator-tile order (include/spvipes_hip.h): T[cell/32][gene/32][qq][lane][j], lane = cell%32 + 32 h, gene%32 = 8 qq + 4 h + j ----
_W = np.arange(1024)                                   # word index inside a tile = qq * 256 + lane * 4 + j
_QQ, _LANE, _J = _W // 256, (_W % 256) // 4, _W % 4
_TILE_CELL, _TILE_GENE = _LANE % 32, 8 * _QQ + 4 * (_LANE // 32) + _J
# the mutation "qq and h swapped": the tile kept h-major, T[..][h][qq][cell%32][j]
_H2, _QQ2, _C2 = _W // 512, (_W % 512) // 128, (_W % 128) // 4
_SWAP_CELL, _SWAP_GENE = _C2, 8 * _QQ2 + 4 * _H2 + _J


def to_tiles(a, swapped: bool = False):
    """[cells][genes] (multiples of 32) -> [cells/32][genes/32][1024]"""
    C, G = a.shape
    assert C % 32 == 0 and G % 32 == 0
    cell, gene = (_SWAP_CELL, _SWAP_GENE) if swapped else (_TILE_CELL, _TILE_GENE)
    blocks = a.reshape(C // 32, 32, G // 32, 32).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(blocks[:, :, cell, gene])


def from_tiles(t, swapped: bool = False):
    ct, gt, n = t.shape
    assert n == 1024
    cell, gene = (_SWAP_CELL, _SWAP_GENE) if swapped else (_TILE_CELL, _TILE_GENE)
    blocks = np.empty((ct, gt, 32, 32), dtype=t.dtype)
    blocks[:, :, cell, gene] = t
    return np.ascontiguousarray(blocks.transpose(0, 2, 1, 3)).reshape(ct * 32, gt * 32)


def tile_offset(cell: int, gene: int, n_gene_tiles: int) -> int:
    """the header's sentence, one element at a time (the loop tests/test_gemm_reference_cpu.py holds to_tiles / from_tiles to)"""
    g = gene % 32
    qq, h, j = g // 8, (g % 8) // 4, g % 4
    lane = cell % 32 + 32 * h
    return (((cell // 32) * n_gene_tiles + gene // 32) * 4 + qq) * 256 + lane * 4 + j


# ---- split-K ranges -------------------------------------------------------------------------------------------------------------------------
def k_per_split(K: int, splits: int) -> int:
    return -(-(-(-K // 64)) // splits) * 64


def split_ranges(K: int, splits: int):
    """[(k0, k1)] per slab: slab s covers [s k_per_split, min(K, (s + 1) k_per_split)), possibly empty (k0 == k1)"""
    kps = k_per_split(K, splits)
    return [(min(s * kps, K), min(K, (s + 1) * kps)) for s in range(splits)]


def tiles_per_split(K: int, splits: int):
    return [-(-(k1 - k0) // 64) for k0, k1 in split_ranges(K, splits)]


def cover(As, Bs, Cs):
    """(a, b, c): every (a, b) and every (a, c) pair once, the third size rotating (tests/_fold_reference.py: cover)"""
    out = []
    for i, a in enumerate(As):
        for j, b in enumerate(Bs):
            out.append((a, b, Cs[(i + j) % len(Cs)]))
        for j, c in enumerate(Cs):
            out.append((a, Bs[(i + 2 * j + 1) % len(Bs)], c))
    return sorted(set(out))


# ---- data ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Lattice:
    a: tuple          # integer range of the A hi plane
    b: tuple          # ... of the B hi plane
    lo: int           # lo planes: integers in [-lo, lo] times gran
    gran: float       # granularity of every term (hi planes are integers)


LAT_F32 = Lattice((-3, 3), (-3, 3), 3, 2.0 ** -6)            # worst |sum| at K = 2048: 2048 (9 + 18 / 64) = 1.9e4 = 1.2e6 granules < 2^24
LAT_F16_1 = Lattice((-1, 3), (0, 2), 0, 1.0)                 # nsplit 1, f16 out, K <= 320: 6 K <= 1920 <= 2^11; mostly positive: sums need > 8 bits
LAT_F16_3 = Lattice((-2, 2), (-2, 2), 1, 0.5)                # nsplit 3, f16 out, K <= 96: (4 + 1 + 1) K / 0.5 <= 1152
LAT_F16_3_DEEP = Lattice((-1, 1), (-1, 1), 1, 0.5)           # nsplit 3, f16 out, K <= 320: (1 + 0.5 + 0.5) K / 0.5 <= 1280


def _planes(rng, shape, tier, irange, lat, nsplit):
    if tier == 1:
        hi = rng.integers(irange[0], irange[1] + 1, size=shape).astype(np.float32)
        lo = (rng.integers(-lat.lo, lat.lo + 1, size=shape) * lat.gran).astype(np.float32) if nsplit == 3 else np.zeros(shape, np.float32)
        return hi, lo
    hi, lo = split_bf16(rng.standard_normal(shape).astype(np.float32))
    return hi, (lo if nsplit == 3 else np.zeros(shape, np.float32))


def sums_are_exact(planes, S, lat: Lattice, f16_out: bool = False) -> bool:
    """every partial sum of the terms is exactly representable: the hi planes are integers, the lo planes multiples of the granularity, and
    the largest sum of |terms| is below 2^24 granules (fp32) / at most 2^11 (f16).  `S`: the sum of |terms| per output element."""
    a_hi, a_lo, b_hi, b_lo = planes
    if not all(np.isfinite(p).all() for p in planes):
        return False
    if (np.mod(a_hi, 1.0) != 0).any() or (np.mod(b_hi, 1.0) != 0).any():
        return False
    if (np.mod(a_lo, lat.gran) != 0).any() or (np.mod(b_lo, lat.gran) != 0).any():
        return False
    granules = float(np.max(S, initial=0.0)) / lat.gran
    return granules <= 2.0 ** 11 if f16_out else granules < 2.0 ** 24


def _terms(a_hi, a_lo, b_hi, b_lo, nsplit):
    """float64 value and sum of |terms| of the definition, over the whole K extent of the planes given ([M][k] x [k][N])"""
    a_hi, a_lo, b_hi, b_lo = (np.asarray(p, dtype=np.float64) for p in (a_hi, a_lo, b_hi, b_lo))
    v, s = a_hi @ b_hi, np.abs(a_hi) @ np.abs(b_hi)
    if nsplit == 3:
        v = v + a_hi @ b_lo + a_lo @ b_hi
        s = s + np.abs(a_hi) @ np.abs(b_lo) + np.abs(a_lo) @ np.abs(b_hi)
    return v, s


def _nan_words(shape):
    return np.full(shape, NAN_WORD, dtype=np.uint16)


def check(got, want, bound=None):
    """got against want (float64, canaries included); bound None / 0 = equality.  Returns (index of the first element outside its bound or
    None, worst error / bound over the elements that have a bound > 0)"""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    b = np.zeros_like(want) if bound is None else np.asarray(bound, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
        bad = ~(err <= b)    # (a NaN is bad)
        ratio = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0), initial=0.0))
    first = tuple(int(i) for i in np.argwhere(bad)[0]) if bad.any() else None
    return first, ratio


def cap_ok(ref, bound) -> bool:
    return float(np.max(bound, initial=0.0)) <= CAP * float(np.max(np.abs(ref), initial=0.0))


# =============================================================================================================================================
# spv_gemm_bf16 / spv_gemm_bf16_fix: C[M][N] = sum_k A(m, k) B(k, n), split-K slabs
# =============================================================================================================================================
@dataclass(frozen=True)
class GemmCase:
    route: str          # "A" LDS-DMA | "B" LDS-DMA + in-launch fix-up | "C" narrow 128 x 32 | "D" register-staged 64 x 320 | "E" a group of spv_gemm_bf16_grouped
    tier: int
    a_kmajor: int
    a_tiled: bool
    M: int
    N: int
    K: int
    nsplit: int
    splits: int
    ldb: int = 320
    b_off: int = 0      # the B pointer is image base + b_off columns
    a_extra: int = 0    # gene tiles per cell tile beyond the minimum (NaN guard tiles)
    ldc_extra: int = 0
    alpha: str = "none"   # "none" | "pow2" (0.25) | "real" (0.37)
    fix: tuple = None     # (n0, c1, n1); n1 == 0: no dst1

    @property
    def name(self) -> str:
        s = f"{self.route}{self.tier}-{'t' if self.a_tiled else 'p'}{'k' if self.a_kmajor else 'm'}{self.nsplit}-M{self.M}-N{self.N}-K{self.K}-s{self.splits}"
        if self.b_off or self.ldb != 320:
            s += f"-ldb{self.ldb}+{self.b_off}"
        if self.a_extra:
            s += f"-x{self.a_extra}"
        if self.ldc_extra:
            s += f"-c{self.ldc_extra}"
        if self.fix:
            s += f"-fix{self.fix[0]}_{self.fix[1]}_{self.fix[2]}-{self.alpha}"
        return s

    @property
    def kernel(self) -> str:
        """the kernel the dispatch conditions of spv_abi.hip select"""
        if self.a_tiled and 32 < self.N <= 320 and self.ldb == 320:
            return "dma4s" if self.nsplit == 3 else "dma4"
        return "narrow" if self.N <= 32 else "wide"

    @property
    def bm(self) -> int:
        return 64 if self.kernel == "wide" else 128

    @property
    def ldc(self) -> int:
        return self.N + self.ldc_extra

    @property
    def window(self) -> int:
        """B columns a workgroup multiplies from the pointer on"""
        return 32 if self.kernel == "narrow" else round_up(self.N, 320)

    @property
    def alpha_value(self) -> float:
        return {"none": 1.0, "pow2": 0.25, "real": float(np.float32(0.37))}[self.alpha]


def _seed(case) -> int:
    return int(np.frombuffer(case.name.encode(), dtype=np.uint8).astype(np.uint64).dot(np.arange(1, len(case.name) + 1, dtype=np.uint64)) % (2 ** 31))


@lru_cache(maxsize=4)     # (a case's two calls and its judgement share one build; the whole grid would be gigabytes)
def build_gemm(case: GemmCase):
    """operands (words, guards included), the planes they hold, the float64 reference per slab and summed, S, n and the bounds"""
    rng = np.random.default_rng(_seed(case))
    M, N, K, ns = case.M, case.N, case.K, case.nsplit
    Mp, Kp, W = round_up(M, case.bm), round_up(K, 64), case.window
    lat = LAT_F32
    a_hi, a_lo = _planes(rng, (M, K), case.tier, lat.a, lat, ns)
    ncols = case.ldb if case.kernel == "narrow" else N      # the narrow kernel's image holds live data in every column
    img_hi, img_lo = _planes(rng, (K, ncols), case.tier, lat.b, lat, ns)
    assert case.b_off + W <= case.ldb
    b_hi, b_lo = img_hi[:, case.b_off:case.b_off + N], img_lo[:, case.b_off:case.b_off + N]

    o = SimpleNamespace(case=case, lat=lat, planes=(a_hi, a_lo, b_hi, b_lo), Mp=Mp, Kp=Kp)
    # ---- A words ------------------------------------------------------------------------------------------------------------------------
    def a_words(plane):
        full = np.zeros((Mp, Kp), np.float32)
        full[:M, :K] = plane
        w = bf16_words(full)
        if case.a_tiled:   # [cells][genes]: a_kmajor 0: cells = M, genes = K;  1: cells = K, genes = M
            cg = w.T if case.a_kmajor else w
            guard_cells = 64 if case.a_kmajor else case.bm
            arr = _nan_words((cg.shape[0] + guard_cells, cg.shape[1] + 32 * case.a_extra))
            arr[:cg.shape[0], :cg.shape[1]] = cg
            return to_tiles(arr).reshape(-1), arr.shape[1] // 32, 0
        mem = w.T if case.a_kmajor else w               # mem[k][m] / mem[m][k]
        guard = (64, case.bm) if case.a_kmajor else (case.bm, 64)
        arr = _nan_words((mem.shape[0] + guard[0], mem.shape[1] + guard[1]))
        arr[:mem.shape[0], :mem.shape[1]] = mem
        return arr.reshape(-1), 0, arr.shape[1]
    o.A_hi, o.a_tiles, o.lda = a_words(a_hi)
    o.A_lo = a_words(a_lo)[0] if ns == 3 else None
    # ---- B words: [Kp + 64][ldb], rows >= Kp NaN, rows K..Kp and (320-column images) columns >= N zero ---------------------------------------
    def b_words(plane):
        arr = _nan_words((Kp + 64, case.ldb))
        arr[:Kp] = 0
        arr[:K, :plane.shape[1]] = bf16_words(plane)
        return arr.reshape(-1)
    o.B_hi = b_words(img_hi)
    o.B_lo = b_words(img_lo) if ns == 3 else None
    # ---- reference ---------------------------------------------------------------------------------------------------------------------------
    o.ranges = split_ranges(K, case.splits)
    o.ref = np.zeros((case.splits, M, N))
    o.S = np.zeros((case.splits, M, N))
    o.n = np.zeros(case.splits)
    for s, (k0, k1) in enumerate(o.ranges):
        o.ref[s], o.S[s] = _terms(a_hi[:, k0:k1], a_lo[:, k0:k1], b_hi[k0:k1], b_lo[k0:k1], ns)
        o.n[s] = ns * (k1 - k0)
    o.bound = 2 * U * o.n[:, None, None] * o.S if case.tier == 2 else np.zeros_like(o.S)
    o.S_sum, alpha = o.S.sum(0), case.alpha_value
    o.ref_sum = alpha * o.ref.sum(0)
    o.n_sum = o.n.sum() + case.splits + (1 if case.alpha == "real" else 0)
    o.bound_sum = 2 * U * o.n_sum * o.S_sum * abs(alpha) if case.tier == 2 else np.zeros_like(o.S_sum)
    o.exact = case.tier == 1 and sums_are_exact(o.planes, o.S_sum, lat)
    # ---- expected buffers: slabs [splits][M + 1][ldc] (one canary row after every slab), dst0 [M + 1][n0 + 3], dst1 [M + 1][n1 + 1] ----------
    def frame(shape, val, bnd, cols):
        want, b = np.full(shape, CANARY), np.zeros(shape)
        want[..., :M, :cols], b[..., :M, :cols] = val, bnd
        return want, b
    o.want, o.want_bound = {}, {}
    o.want["C"], o.want_bound["C"] = frame((case.splits, M + 1, case.ldc), o.ref, o.bound, N)
    if case.fix:
        n0, c1, n1 = case.fix
        o.want["d0"], o.want_bound["d0"] = frame((M + 1, n0 + 3), o.ref_sum[:, :n0], o.bound_sum[:, :n0], n0)
        if n1:
            o.want["d1"], o.want_bound["d1"] = frame((M + 1, n1 + 1), o.ref_sum[:, c1:c1 + n1], o.bound_sum[:, c1:c1 + n1], n1)
    return o


MUTATIONS = ("drop_a_lo_b_hi", "drop_a_hi_b_lo", "add_a_lo_b_lo", "slab_starts_a_tile_late", "slab_stops_a_tile_early", "empty_slab_unwritten",
             "swap_qq_and_h", "b_window_at_offset_0", "store_32_columns", "slab_rounded_to_bf16", "f16_through_bf16")


def _mac(acc, a_hi, a_lo, b_hi, b_lo, nsplit, mut):
    """one 16-deep MFMA step in float32, terms in mfma32_split's order"""
    if nsplit == 3:
        if mut != "drop_a_hi_b_lo":
            acc = acc + a_hi @ b_lo
        if mut != "drop_a_lo_b_hi":
            acc = acc + a_lo @ b_hi
        if mut == "add_a_lo_b_lo":
            acc = acc + a_lo @ b_lo
    return acc + a_hi @ b_hi


def _tile_range(k0, k1, Kp, mut):
    """the 64-deep tiles of a slab [k0, k1) of the padded K extent, with the range mutations"""
    k1 = min(round_up(k1, 64), Kp)
    if mut == "slab_starts_a_tile_late" and k1 > k0:
        k0 += 64
    if mut == "slab_stops_a_tile_early" and k1 > k0:
        k1 -= 64
    return k0, k1


def model_gemm(case: GemmCase, o, mut: str = None):
    """numpy float32 emulation of spv_gemm_bf16[_fix] on the words of `o`: {"C": slabs, "d0": .., "d1": ..} as the device leaves them"""
    Mp, Kp, M, N, ns = o.Mp, o.Kp, case.M, case.N, case.nsplit
    swapped = mut == "swap_qq_and_h"

    def a_plane(words):
        if words is None:
            return None
        if case.a_tiled:
            cg = from_tiles(words.reshape(-1, o.a_tiles, 1024), swapped)
            cg = cg[:Kp, :Mp] if case.a_kmajor else cg[:Mp, :Kp]
            return words_f32(cg.T if case.a_kmajor else cg)
        mem = words.reshape(-1, o.lda)
        return words_f32(mem[:Kp, :Mp].T if case.a_kmajor else mem[:Mp, :Kp])
    off = 0 if mut == "b_window_at_offset_0" else case.b_off
    W = min(case.window, case.ldb - off)

    def b_plane(words):
        return None if words is None else words_f32(words.reshape(-1, case.ldb)[:Kp, off:off + W])
    a_hi, a_lo, b_hi, b_lo = a_plane(o.A_hi), a_plane(o.A_lo), b_plane(o.B_hi), b_plane(o.B_lo)
    out = {"C": np.full((case.splits * (M + 1) * case.ldc,), CANARY, dtype=np.float32)}
    stride = (M + 1) * case.ldc
    ncol = min(32 if (mut == "store_32_columns" and N < 32) else N, W)
    slabs = []
    kps = k_per_split(case.K, case.splits)
    for s in range(case.splits):
        k0, k1 = _tile_range(min(s * kps, Kp), min((s + 1) * kps, Kp), Kp, mut)
        acc = np.zeros((Mp, W), np.float32)
        for k in range(k0, k1, 16):
            sl = slice(k, k + 16)
            acc = _mac(acc, a_hi[:, sl], None if a_lo is None else a_lo[:, sl], b_hi[sl], None if b_lo is None else b_lo[sl], ns, mut)
        if mut == "slab_rounded_to_bf16":
            acc = bf16_round(acc)
        slabs.append(acc[:M, :N])
        if mut == "empty_slab_unwritten" and s * kps >= case.K:
            continue
        for r in range(M):   # (rows in order: a store wider than ldc spills into the next row, which is written afterwards)
            out["C"][s * stride + r * case.ldc: s * stride + r * case.ldc + ncol] = acc[r, :ncol]
    out["C"] = out["C"].reshape(case.splits, M + 1, case.ldc)
    if case.fix:
        n0, c1, n1 = case.fix
        written = out["C"][:, :M, :N]     # the fix-up sums what is in memory, slab 0 first
        total = np.zeros((M, N), np.float32)
        for s in range(case.splits):
            total = total + written[s]
        total = total * np.float32(case.alpha_value)
        out["d0"] = np.full((M + 1, n0 + 3), CANARY, dtype=np.float32)
        out["d0"][:M, :n0] = total[:, :n0]
        if n1:
            out["d1"] = np.full((M + 1, n1 + 1), CANARY, dtype=np.float32)
            out["d1"][:M, :n1] = total[:, c1:c1 + n1]
    return out


def explain_gemm(case: GemmCase, o, buf: str, idx, got: float) -> str:
    """names the first wrong element and, where one 64-deep K tile's terms account for the difference, that tile and term"""
    if buf == "C":
        s, r, c = idx
    else:
        s, (r, c) = None, idx
        c += case.fix[1] if buf == "d1" else 0
    where = f"{case.name}: {buf} row {r} column {c}" + (f" slab {s}" if s is not None else "")
    if r >= case.M or c >= case.N or (buf != "C" and c >= (case.fix[0] if buf == "d0" else case.fix[1] + case.fix[2])):
        return where + f": canary overwritten with {got!r}"
    want = float(o.ref[s, r, c] if s is not None else o.ref_sum[r, c])
    msg = where + f": got {got!r}, want {want!r}"
    if not np.isfinite(got):
        return msg + " (a NaN / infinity: a read outside the operand's contract extent, or an unwritten slab)"
    if got == CANARY:
        return msg + " (the canary: never written)"
    a_hi, a_lo, b_hi, b_lo = (np.asarray(p, dtype=np.float64) for p in o.planes)
    diff = float((got - want) / (case.alpha_value if s is None else 1.0))
    for t in range(0, case.K, 64):
        sl = slice(t, min(t + 64, case.K))
        terms = {"a_hi b_hi": a_hi[r, sl] @ b_hi[sl, c], "a_hi b_lo": a_hi[r, sl] @ b_lo[sl, c], "a_lo b_hi": a_lo[r, sl] @ b_hi[sl, c],
                 "a_lo b_lo": a_lo[r, sl] @ b_lo[sl, c]}
        terms["all terms"] = terms["a_hi b_hi"] + (terms["a_hi b_lo"] + terms["a_lo b_hi"] if case.nsplit == 3 else 0.0)
        for nm, v in terms.items():
            if v != 0 and abs(abs(diff) - abs(v)) <= 1e-9 * abs(v):
                return msg + f": the difference {diff!r} is {'an extra' if diff * v > 0 else 'a missing'} '{nm}' of K tile {t // 64} (k {sl.start}..{sl.stop - 1})"
    return msg + f": difference {diff!r} matches no single K tile's terms"


# ---- the case grids --------------------------------------------------------------------------------------------------------------------------
A_M, A_N, A_K, A_TPS = (1, 127, 128, 129, 300), (33, 36, 319, 320), (1, 63, 64, 65, 192, 320, 1000, 2048), (1, 2, 3, 5)
KERNELS_4 = ((0, 1), (0, 3), (1, 1), (1, 3))   # (a_kmajor, nsplit)


def _splits_for(K: int, tps: int) -> int:
    return max(1, -(-(-(-K // 64)) // tps))


def _dedupe(cases):
    seen, out = set(), []
    for c in cases:
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return out


@lru_cache(maxsize=None)
def route_a_cases():
    out = []
    for kidx, (akm, ns) in enumerate(KERNELS_4):
        trip = [(K, M, N, A_TPS[(i + kidx) % 4]) for i, (K, M, N) in enumerate(cover(A_K, A_M, A_N))]   # every (K, M) and (K, N) pair, the third size rotating
        # every pipeline depth on a K long enough to reach it
        trip += [(2048, 129, 320, 5), (1000, 300, 319, 3), (320, 127, 36, 2), (192, 128, 33, 1)]
        for i, (K, M, N, tps) in enumerate(trip):
            out.append(GemmCase("A", 1, akm, True, M, N, K, ns, _splits_for(K, tps), a_extra=2 * (i % 2), ldc_extra=4 * ((i // 2) % 2)))
        # a trailing EMPTY split: its slab must be zeros, and nothing may be read for it
        out += [GemmCase("A", 1, akm, True, 129, 320, 320, ns, 4, a_extra=2), GemmCase("A", 1, akm, True, 1, 33, 1, ns, 2),
                GemmCase("A", 1, akm, True, 300, 36, 192, ns, 4, ldc_extra=4)]
        # tier 2: K <= 256 (nsplit 3) / <= 1024 (nsplit 1)
        Kbig = 1000 if ns == 1 else 256
        out += [GemmCase("A", 2, akm, True, 129, 320, Kbig, ns, 3), GemmCase("A", 2, akm, True, 300, 36, 192, ns, 4, a_extra=2, ldc_extra=4),
                GemmCase("A", 2, akm, True, 127, 319, 65, ns, 1)]
    return tuple(_dedupe(out))


@lru_cache(maxsize=None)
def route_b_cases():
    out = []
    for kidx, (akm, ns) in enumerate(KERNELS_4):
        def mk(tier, M, N, K, splits, fix, alpha, x=0):
            return GemmCase("B", tier, akm, True, M, N, K, ns, splits, a_extra=x, ldc_extra=round_up(N, 4) + 4 - N, fix=fix, alpha=alpha)
        out += [mk(1, 300, 320, 1000, 3, (256, 256, 64), "pow2"),           # dst1 ends at N
                mk(1, 129, 36, 320, 4, (20, 24, 8), "none", 2),            # dst1 inside; a trailing empty split
                mk(1, 127, 319, 2048, 7, (319, 0, 0), "pow2"),             # no dst1
                mk(1, 1, 33, 65, 2, (17, 20, 13), "none"),
                mk(2, 300, 320, 256, 3, (256, 256, 64), "real"),
                mk(2, 129, 36, 192, 4, (20, 24, 8), "real", 2)]           # a trailing empty split
    return tuple(_dedupe(out))


C_M, C_N = (1, 127, 128, 129, 300), (1, 16, 31, 32)
C_KS = ((1, 1), (65, 2), (192, 1), (250, 1), (320, 1), (1000, 4), (320, 4), (64, 2))   # tiles per split 1 | 1, 1 | 3 | 4 | 5 | 4.. | 2, 2, 1, 0 | 1, 0


@lru_cache(maxsize=None)
def route_c_cases():
    out = []
    kernels = [(t, akm, ns) for t in (True, False) for akm in (0, 1) for ns in (1, 3)]
    for kidx, (tiled, akm, ns) in enumerate(kernels):
        mine = [(M, N) for k, M, N in cover(tuple(range(len(kernels))), C_M, C_N) if k == kidx]   # every (kernel, M) and (kernel, N) pair, K / splits rotating
        for i in range(max(len(mine), len(C_KS))):   # (and every K / splits pair at least once)
            (M, N), (K, splits) = mine[i % len(mine)], C_KS[(i + kidx) % len(C_KS)]
            out.append(GemmCase("C", 1, akm, tiled, M, N, K, ns, splits, ldb=48, b_off=16 * ((i + kidx + 1) % 2), a_extra=2 * (i % 2) if tiled else 0))
        out += [GemmCase("C", 1, akm, tiled, 129, 16, 192, ns, 2, ldb=48, b_off=16),     # the product's shape: 16 columns at b_col_off 16
                GemmCase("C", 1, akm, tiled, 300, 32, 320, ns, 4, ldb=48, b_off=16),     # 32 columns ending at the image's edge, an empty split
                GemmCase("C", 1, akm, tiled, 129, 32, 192, ns, 2, ldb=96, b_off=64),     # the wide K-slot layout: the last 32 columns of a 96-wide image
                GemmCase("C", 2, akm, tiled, 129, 16, 192, ns, 4, ldb=48, b_off=16),
                GemmCase("C", 2, akm, tiled, 300, 31, 250, ns, 1, ldb=48, b_off=0)]
    return tuple(_dedupe(out))


D_M = (1, 63, 64, 65, 130)
D_KS = ((1, 2), (65, 1), (192, 3), (320, 4), (1000, 4), (2048, 7), (64, 1))


@lru_cache(maxsize=None)
def route_d_cases():
    out = []
    kernels = [(t, akm, ns) for t in (False, True) for akm in (0, 1) for ns in (1, 3)]
    for kidx, (tiled, akm, ns) in enumerate(kernels):
        ldb, Ns = (640, (400,)) if tiled else (320, (33, 320, 319))
        mine = [(M, ks) for k, M, ks in cover(tuple(range(len(kernels))), D_M, tuple(range(len(D_KS)))) if k == kidx]   # every (kernel, M) and (kernel, K / splits) pair
        for i, (M, ks) in enumerate(mine):
            K, splits = D_KS[ks]
            out.append(GemmCase("D", 1, akm, tiled, M, Ns[(i + kidx) % len(Ns)], K, ns, splits, ldb=ldb, a_extra=2 * (i % 2) if tiled else 0, ldc_extra=4 * (i % 2)))
        out.append(GemmCase("D", 2, akm, tiled, 130, Ns[0], 192, ns, 4, ldb=ldb))
        out.append(GemmCase("D", 2, akm, tiled, 65, Ns[-1], 1000 if ns == 1 else 256, ns, 2, ldb=ldb, ldc_extra=4))
    return tuple(_dedupe(out))


def gemm_cases():
    return route_a_cases() + route_b_cases() + route_c_cases() + route_d_cases()


def _dma(akm, M, K, splits, tier=1, ns=1, x=0):
    return GemmCase("E", tier, akm, True, M, 320, K, ns, splits, a_extra=x)


def grouped_gemm_cases():
    """(name, groups, [expected launches: "pair" or "single" per launch])"""
    return (
        ("pair-m", (_dma(0, 300, 1000, 3), _dma(0, 129, 192, 1, x=2)), ("pair",)),            # the grid is sized by the larger: 9 against 2 workgroups
        ("pair-k", (_dma(1, 127, 320, 4), _dma(1, 300, 2048, 5)), ("pair",)),                 # the smaller first; a trailing empty split in it
        ("pair-k-real", (_dma(1, 300, 1000, 3, tier=2), _dma(1, 129, 192, 4, tier=2)), ("pair",)),
        ("three", (_dma(0, 129, 320, 2), _dma(0, 1, 65, 2), _dma(0, 300, 192, 1)), ("pair", "single")),
        ("mixed-direction", (_dma(0, 129, 320, 2), _dma(1, 128, 192, 3)), ("single", "single")),
        ("mixed-words", (_dma(0, 129, 320, 2), _dma(0, 128, 192, 3, ns=3)), ("single", "single")),
    )


# =============================================================================================================================================
# spv_dec_heads_wgrad: slabP[s][g][0..15] = sum_cell tP(cell, g) Aps[cell][0..15],  slabS[s][g][0..31] = sum_cell tS(cell, g) Aps[cell][16..47]
# =============================================================================================================================================
@dataclass(frozen=True)
class HeadsCase:
    tier: int
    G: int
    Bp: int
    splits: int
    a_extra: int = 0   # gene tiles beyond the minimum round_up(G, 128) / 32 the entry point accepts

    @property
    def name(self) -> str:
        return f"F{self.tier}-G{self.G}-B{self.Bp}-s{self.splits}-x{self.a_extra}"

    @property
    def min_tiles(self) -> int:
        return round_up(self.G, 128) // 32


HEADS_TAIL = 128 * 32   # canary words after the last slab


@lru_cache(maxsize=4)     # (a case's two calls and its judgement share one build; the whole grid would be gigabytes)
def build_heads(case: HeadsCase):
    rng = np.random.default_rng(_seed(case))
    G, Bp = case.G, case.Bp
    lat = LAT_F32
    tP, _ = _planes(rng, (Bp, G), case.tier, lat.a, lat, 1)
    tS, _ = _planes(rng, (Bp, G), case.tier, lat.a, lat, 1)
    aps, _ = _planes(rng, (Bp, 48), case.tier, lat.b, lat, 1)
    o = SimpleNamespace(case=case, lat=lat, tP=tP, tS=tS, aps=aps, a_tiles=case.min_tiles + case.a_extra)

    def t_words(plane):   # [Bp + 64 guard cells][a_tiles * 32]: genes G .. round_up(G, 128) zero, beyond NaN
        arr = _nan_words((Bp + 64, o.a_tiles * 32))
        arr[:Bp, :case.min_tiles * 32] = 0
        arr[:Bp, :G] = bf16_words(plane)
        return to_tiles(arr).reshape(-1)
    o.tP_w, o.tS_w = t_words(tP), t_words(tS)
    o.aps_w = _nan_words((Bp + 64, 48))
    o.aps_w[:Bp] = bf16_words(aps)
    o.aps_w = o.aps_w.reshape(-1)
    o.ranges = split_ranges(Bp, case.splits)
    z = np.zeros_like
    o.want, o.want_bound, o.ref, o.S = {}, {}, {}, {}
    for nm, t, cols in (("P", tP, slice(0, 16)), ("S", tS, slice(16, 48))):
        w = cols.stop - cols.start
        ref, S, n = np.zeros((case.splits, G, w)), np.zeros((case.splits, G, w)), np.zeros(case.splits)
        for s, (k0, k1) in enumerate(o.ranges):
            ref[s], S[s] = _terms(t[k0:k1].T, z(t[k0:k1].T), aps[k0:k1, cols], z(aps[k0:k1, cols]), 1)
            n[s] = k1 - k0
        bound = 2 * U * n[:, None, None] * S if case.tier == 2 else z(S)
        o.ref[nm], o.S[nm] = ref, S
        o.want[nm] = np.concatenate([ref.reshape(-1), np.full(HEADS_TAIL, CANARY)])
        o.want_bound[nm] = np.concatenate([bound.reshape(-1), np.zeros(HEADS_TAIL)])
    o.exact = case.tier == 1 and all(sums_are_exact((t.T, z(t.T), aps[:, c], z(aps[:, c])), o.S[nm].sum(0), lat)
                                     for nm, t, c in (("P", tP, slice(0, 16)), ("S", tS, slice(16, 48))))
    return o


def model_heads(case: HeadsCase, o, mut: str = None):
    G, Bp = case.G, case.Bp
    Gp = case.min_tiles * 32
    aps = words_f32(o.aps_w.reshape(-1, 48)[:Bp])
    out = {}
    kps = k_per_split(Bp, case.splits)
    for nm, words, c0, w in (("P", o.tP_w, 0, 16), ("S", o.tS_w, 16, 32)):
        t = words_f32(from_tiles(words.reshape(-1, o.a_tiles, 1024), mut == "swap_qq_and_h")[:Bp, :Gp])
        buf = np.full(case.splits * G * w + HEADS_TAIL, CANARY, dtype=np.float32)
        for s in range(case.splits):
            k0, k1 = _tile_range(min(s * kps, Bp), min((s + 1) * kps, Bp), Bp, mut)
            acc = np.zeros((Gp, 32), np.float32)
            for k in range(k0, k1, 16):
                acc = acc + t[k:k + 16].T @ aps[k:k + 16, c0:c0 + 32]
            if mut == "slab_rounded_to_bf16":
                acc = bf16_round(acc)
            if mut == "empty_slab_unwritten" and s * kps >= Bp:
                continue
            buf[s * G * w:(s + 1) * G * w] = acc[:G, :w].reshape(-1)
        out[nm] = buf
    return out


def explain_heads(case: HeadsCase, o, buf: str, idx, got: float) -> str:
    w = 16 if buf == "P" else 32
    i = idx[0]
    if i >= case.splits * case.G * w:
        return f"{case.name}: slab{buf}: canary word {i - case.splits * case.G * w} after the last slab overwritten with {got!r}"
    s, g, c = i // (case.G * w), (i // w) % case.G, i % w
    k0, k1 = o.ranges[s]
    return (f"{case.name}: slab{buf} gene {g} column {c} split {s} (cells {k0}..{k1 - 1}, 64-cell tiles {k0 // 64}..{(k1 - 1) // 64 if k1 > k0 else '-'}): "
            f"got {got!r}, want {float(o.ref[buf][s, g, c])!r}")


F_G, F_B = (1, 127, 128, 129, 300), (64, 128, 320)


@lru_cache(maxsize=None)
def heads_cases():
    out = []
    for i, G in enumerate(F_G):
        for j, Bp in enumerate(F_B):
            splits = (1, 2, 3, Bp // 64 + 1)[(i + j) % 4]
            out.append(HeadsCase(1, G, Bp, splits, a_extra=4 * ((i + j) % 2)))
    out += [HeadsCase(1, 129, 320, 6), HeadsCase(1, 300, 64, 2, 4), HeadsCase(1, 127, 128, 3)]     # more splits than 64-cell tiles: empty slabs
    out += [HeadsCase(2, 300, 320, 2), HeadsCase(2, 129, 128, 3, 4), HeadsCase(2, 1, 64, 1)]
    return tuple(_dedupe(out))


# =============================================================================================================================================
# spv_dec_logits: out(cell, gene) = sum_k Am[cell][k] Wm[gene][k], f16 or f32 in accumulator-tile order
# =============================================================================================================================================
@dataclass(frozen=True)
class LogitsCase:
    tier: int
    K: int
    Bp: int
    Gp: int
    nsplit: int
    out_f32: int

    @property
    def name(self) -> str:
        return f"G{self.tier}-{self.kernel}-K{self.K}-B{self.Bp}-G{self.Gp}-{'f32' if self.out_f32 else 'f16'}"

    @property
    def kernel(self) -> str:
        """the route spv_dec_logits' dispatch conditions select"""
        if self.nsplit == 1 and not self.out_f32 and self.Gp % 256 == 0 and self.Bp % 128 == 0:
            return "dma"
        if self.nsplit == 3:
            return "g128x128s3"
        return "g256x128" if self.Gp % 256 == 0 else "g128x128"


LOGITS_TAIL = 1024


@lru_cache(maxsize=4)     # (a case's two calls and its judgement share one build; the whole grid would be gigabytes)
def build_logits(case: LogitsCase):
    rng = np.random.default_rng(_seed(case))
    K, Bp, Gp, ns = case.K, case.Bp, case.Gp, case.nsplit
    f16 = not case.out_f32
    lat = LAT_F32 if not f16 else LAT_F16_1 if ns == 1 else LAT_F16_3 if K <= 96 else LAT_F16_3_DEEP
    am_hi, am_lo = _planes(rng, (Bp, K), case.tier, lat.a, lat, ns)
    wm_hi, wm_lo = _planes(rng, (Gp, K), case.tier, lat.b, lat, ns)
    o = SimpleNamespace(case=case, lat=lat, planes=(am_hi, am_lo, wm_hi.T, wm_lo.T))

    def words(plane, guard):
        arr = _nan_words((plane.shape[0] + guard, K))
        arr[:plane.shape[0]] = bf16_words(plane)
        return arr.reshape(-1)
    o.Am_hi, o.Wm_hi = words(am_hi, 128), words(wm_hi, 256)
    o.Am_lo, o.Wm_lo = (words(am_lo, 128), words(wm_lo, 256)) if ns == 3 else (None, None)
    o.ref, o.S = _terms(*o.planes, ns)              # [cells][genes]
    o.n = ns * K
    bound = np.zeros_like(o.S)
    if case.tier == 2:
        bound = 2 * U * o.n * o.S + ((2.0 ** -11) * np.abs(o.ref) + 2.0 ** -25 if f16 else 0.0)
    o.bound = bound
    o.exact = case.tier == 1 and sums_are_exact(o.planes, o.S, lat, f16_out=f16)
    o.want = {"out": np.concatenate([to_tiles(o.ref).reshape(-1), np.full(LOGITS_TAIL, CANARY)])}
    o.want_bound = {"out": np.concatenate([to_tiles(bound).reshape(-1), np.zeros(LOGITS_TAIL)])}
    return o


def model_logits(case: LogitsCase, o, mut: str = None):
    K, Bp, Gp, ns = case.K, case.Bp, case.Gp, case.nsplit
    am_hi, wm_hi = words_f32(o.Am_hi.reshape(-1, K)[:Bp]), words_f32(o.Wm_hi.reshape(-1, K)[:Gp]).T
    am_lo, wm_lo = (words_f32(o.Am_lo.reshape(-1, K)[:Bp]), words_f32(o.Wm_lo.reshape(-1, K)[:Gp]).T) if ns == 3 else (None, None)
    acc = np.zeros((Bp, Gp), np.float32)
    for k in range(0, K, 16):
        sl = slice(k, k + 16)
        acc = _mac(acc, am_hi[:, sl], None if am_lo is None else am_lo[:, sl], wm_hi[sl], None if wm_lo is None else wm_lo[sl], ns, mut)
    if case.out_f32:
        vals = acc
    else:
        vals = (bf16_round(acc) if mut == "f16_through_bf16" else acc).astype(np.float16)
    tail = np.full(LOGITS_TAIL, CANARY, dtype=vals.dtype)
    return {"out": np.concatenate([to_tiles(vals, mut == "swap_qq_and_h").reshape(-1), tail])}


def explain_logits(case: LogitsCase, o, buf: str, idx, got: float) -> str:
    i = idx[0]
    if i >= case.Bp * case.Gp:
        return f"{case.name}: canary word {i - case.Bp * case.Gp} after the last tile overwritten with {got!r}"
    T = case.Gp // 32
    tile, w = i // 1024, i % 1024
    cell, gene = (tile // T) * 32 + int(_TILE_CELL[w]), (tile % T) * 32 + int(_TILE_GENE[w])
    return (f"{case.name}: tile (cell tile {tile // T}, gene tile {tile % T}) word {w} = cell {cell}, gene {gene} (qq {w // 256}, lane {(w % 256) // 4}, j {w % 4}): "
            f"got {got!r}, want {float(o.ref[cell, gene])!r}")


G_K = (32, 64, 96, 320)


@lru_cache(maxsize=None)
def logits_cases():
    out = []
    routes = ((1, 0, (256, 512)), (1, 1, (256, 512)), (1, 0, (128, 384)), (1, 1, (384, 128)), (3, 0, (128, 256, 384, 512)), (3, 1, (512, 384, 256, 128)))
    for ridx, (ns, f32, Gps) in enumerate(routes):
        for i, K in enumerate(G_K):
            out.append(LogitsCase(1, K, (128, 256)[(i + ridx) % 2], Gps[i % len(Gps)], ns, f32))
        out.append(LogitsCase(2, 320 if ns == 1 else 96, 256, Gps[0], ns, f32))
        out.append(LogitsCase(2, 64 if ns == 1 else 256, 128, Gps[-1], ns, f32))
    return tuple(_dedupe(out))


def grouped_logits_cases():
    return (
        ("pair", (LogitsCase(1, 64, 128, 512, 1, 0), LogitsCase(1, 320, 256, 256, 1, 0)), ("pair",)),     # unequal K, Bp and Gp: the grid is the larger of each
        ("pair-real", (LogitsCase(2, 320, 256, 256, 1, 0), LogitsCase(2, 96, 128, 512, 1, 0)), ("pair",)),
        ("mixed", (LogitsCase(1, 64, 128, 256, 1, 0), LogitsCase(1, 96, 256, 384, 3, 1)), ("single", "single")),
        ("three", (LogitsCase(1, 32, 128, 256, 1, 0), LogitsCase(1, 96, 256, 512, 1, 0), LogitsCase(1, 64, 128, 128, 1, 0)), ("pair", "single")),
    )


# ---- what each mutation can affect ------------------------------------------------------------------------------------------------------------
def mutation_applies(mut: str, case) -> bool:
    if mut in ("drop_a_lo_b_hi", "drop_a_hi_b_lo", "add_a_lo_b_lo"):
        return getattr(case, "nsplit", 1) == 3
    if mut in ("slab_starts_a_tile_late", "slab_stops_a_tile_early"):
        return isinstance(case, (GemmCase, HeadsCase))
    if mut == "empty_slab_unwritten":
        if isinstance(case, GemmCase):
            return k_per_split(case.K, case.splits) * (case.splits - 1) >= case.K
        return isinstance(case, HeadsCase) and k_per_split(case.Bp, case.splits) * (case.splits - 1) >= case.Bp
    if mut == "swap_qq_and_h":
        return not isinstance(case, GemmCase) or case.a_tiled
    if mut == "b_window_at_offset_0":
        return isinstance(case, GemmCase) and case.b_off > 0
    if mut == "store_32_columns":
        return isinstance(case, GemmCase) and case.kernel == "narrow" and case.N == 16
    if mut == "slab_rounded_to_bf16":
        return isinstance(case, (GemmCase, HeadsCase))
    if mut == "f16_through_bf16":
        return isinstance(case, LogitsCase) and not case.out_f32
    raise KeyError(mut)


def all_cases():
    grouped = tuple(c for _, cs, _ in grouped_gemm_cases() + grouped_logits_cases() for c in cs)
    return tuple(_dedupe(gemm_cases() + heads_cases() + logits_cases() + grouped))


def build(case):
    return build_gemm(case) if isinstance(case, GemmCase) else build_heads(case) if isinstance(case, HeadsCase) else build_logits(case)


def model(case, o, mut: str = None):
    return model_gemm(case, o, mut) if isinstance(case, GemmCase) else model_heads(case, o, mut) if isinstance(case, HeadsCase) else model_logits(case, o, mut)


def explain(case, o, buf, idx, got) -> str:
    f = explain_gemm if isinstance(case, GemmCase) else explain_heads if isinstance(case, HeadsCase) else explain_logits
    return f(case, o, buf, idx, got)


def compare(case, o, got: dict):
    """every output buffer of a case against its expectation.  Returns (list of failure messages, worst error / bound)"""
    fails, worst = [], 0.0
    for buf, want in o.want.items():
        g = np.asarray(got[buf]).reshape(want.shape)
        first, ratio = check(g, want, o.want_bound[buf])
        worst = max(worst, ratio)
        if first is not None:
            fails.append(explain(case, o, buf, first, float(g[first])))
    return fails, worst
