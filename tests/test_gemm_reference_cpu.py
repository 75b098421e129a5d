"""The reference the decoder-GEMM GPU tests (tests/test_gpu_gemm_family.py) compare with, checked on the CPU: the tile-order functions
against the header's formula, every lattice case exact, every real-valued case under the 1e-3 cap, the float32 model equal to / inside the
reference, and every named mutation of the model caught by the comparison the GPU tests make -- in each tier it can affect."""
import numpy as np
import pytest

from tests import _gemm_reference as R

# The tiers in which a mutation must be caught.  `add_a_lo_b_lo` is tier 1 only: a lo x lo product is 2^-16 of the hi x hi one, far below
# the order-free bound 2 U n S of the real-valued tier (that tier exists for precision-class mistakes); the lattice tier sees it as a bit.
MUTATION_TIERS = {m: (1, 2) for m in R.MUTATIONS}
MUTATION_TIERS["add_a_lo_b_lo"] = (1,)


def test_tile_order_functions_are_inverse_and_follow_the_header():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 2 ** 16, size=(96, 160)).astype(np.uint16)
    t = R.to_tiles(a)
    assert t.shape == (3, 5, 1024)
    assert np.array_equal(R.from_tiles(t), a)
    assert np.array_equal(R.to_tiles(R.from_tiles(t)), t)
    flat = t.reshape(-1)
    for cell in range(96):          # index by index: T[cell/32][gene/32][qq][lane = cell%32 + 32 h][j], gene%32 = 8 qq + 4 h + j
        for gene in range(160):
            assert flat[R.tile_offset(cell, gene, 5)] == a[cell, gene]
    # the mutated order is a different permutation of every tile, and self-consistent
    assert not np.array_equal(R.to_tiles(a, swapped=True), t)
    assert np.array_equal(R.from_tiles(R.to_tiles(a, swapped=True), swapped=True), a)


def test_split_ranges():
    assert R.k_per_split(1000, 3) == 384 and R.split_ranges(1000, 3) == [(0, 384), (384, 768), (768, 1000)]
    assert R.split_ranges(320, 4) == [(0, 128), (128, 256), (256, 320), (320, 320)]        # a trailing empty split
    assert R.split_ranges(1, 2) == [(0, 1), (1, 1)]
    assert R.tiles_per_split(2048, 7) == [5, 5, 5, 5, 5, 5, 2]
    for K in (1, 63, 64, 65, 192, 320, 1000, 2048):
        for splits in range(1, 40):
            rg = R.split_ranges(K, splits)
            assert rg[0][0] == 0 and max(k1 for _, k1 in rg) == K and all(a[1] == b[0] or b[0] == b[1] == K for a, b in zip(rg, rg[1:]))


def test_bf16_helpers():
    import torch
    x = np.random.default_rng(1).standard_normal(4096).astype(np.float32)
    x[:4] = [1.00390625, 1.01171875, -1.00390625, 0.0]     # ties: to even
    assert np.array_equal(R.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    hi, lo = R.split_bf16(x)
    assert np.array_equal(R.words_f32(R.bf16_words(hi)), hi)
    assert np.abs(x - (hi.astype(np.float64) + lo)).max() <= 2.0 ** -16 * np.abs(x).max()
    assert np.isnan(R.words_f32(np.array([R.NAN_WORD], dtype=np.uint16)))[0]
    for v in (R.CANARY,):
        assert float(np.float16(v)) == v and float(R.bf16_round(np.array([v]))[0]) == v


def test_the_grids_reach_what_they_name():
    """sizes, pipeline depths and empty splits the issue's table asks for, per kernel"""
    for route, cases in (("A", R.route_a_cases()), ("B", R.route_b_cases())):
        for akm, ns in R.KERNELS_4:
            mine = [c for c in cases if (c.a_kmajor, c.nsplit) == (akm, ns) and c.tier == 1]
            assert all(c.kernel == ("dma4s" if ns == 3 else "dma4") for c in mine)
            assert any(0 in R.tiles_per_split(c.K, c.splits) for c in mine), (route, akm, ns, "no trailing empty split")
            if route == "A":
                assert {max(R.tiles_per_split(c.K, c.splits)) for c in mine} >= {1, 2, 3, 5}
                assert {c.M for c in mine} >= set(R.A_M) and {c.N for c in mine} >= set(R.A_N) and {c.K for c in mine} >= set(R.A_K)
            else:
                assert {c.alpha for c in mine} == {"none", "pow2"} and {c.alpha for c in cases if c.tier == 2} == {"real"}
                assert any(c.fix[2] == 0 for c in mine) and any(c.fix[2] and c.fix[1] + c.fix[2] == c.N for c in mine) and any(c.fix[2] and c.fix[1] + c.fix[2] < c.N for c in mine)
    for tiled in (True, False):
        for akm, ns in R.KERNELS_4:
            mine = [c for c in R.route_c_cases() if (c.a_tiled, c.a_kmajor, c.nsplit) == (tiled, akm, ns) and c.tier == 1]
            assert all(c.kernel == "narrow" and c.ldc == c.N and c.ldb in (48, 96) for c in mine)
            assert {t for c in mine for t in R.tiles_per_split(c.K, c.splits)} >= {0, 1, 3, 4, 5}
            assert {c.N for c in mine} >= set(R.C_N) and {c.M for c in mine} >= set(R.C_M) and {c.b_off for c in mine} == {0, 16, 64}
            assert any(c.N == 16 and c.b_off == 16 for c in mine)
            mine = [c for c in R.route_d_cases() if (c.a_tiled, c.a_kmajor, c.nsplit) == (tiled, akm, ns) and c.tier == 1]
            assert all(c.kernel == "wide" for c in mine) and {c.M for c in mine} >= set(R.D_M)
            assert all((c.N, c.ldb) == (400, 640) for c in mine) if tiled else all(c.N <= 320 and c.ldb == 320 for c in mine)
            assert any(0 in R.tiles_per_split(c.K, c.splits) for c in mine)
    heads = [c for c in R.heads_cases() if c.tier == 1]
    assert {(c.G, c.Bp) for c in heads} >= {(g, b) for g in R.F_G for b in R.F_B} and {c.a_extra for c in heads} == {0, 4}
    assert any(c.splits > c.Bp // 64 for c in heads) and {1, 2, 3} <= {c.splits for c in heads}
    assert {c.kernel for c in R.logits_cases()} == {"dma", "g256x128", "g128x128", "g128x128s3"}
    for kern in ("dma", "g256x128", "g128x128", "g128x128s3"):
        assert {c.K for c in R.logits_cases() if c.kernel == kern and c.tier == 1} == set(R.G_K)
    assert {(c.nsplit, c.out_f32) for c in R.logits_cases()} == {(1, 0), (1, 1), (3, 0), (3, 1)}
    for c in R.all_cases():     # the real-valued tier keeps to the K range its bound was derived for
        if c.tier == 2:
            K = c.Bp if isinstance(c, R.HeadsCase) else c.K
            assert K <= (256 if getattr(c, "nsplit", 1) == 3 else 1024), c.name
    assert len({c.name for c in R.all_cases()}) == len(R.all_cases())


def test_every_lattice_case_is_exact_and_every_real_case_meets_the_cap():
    worst_cap = 0.0
    for c in R.all_cases():
        o = R.build(c)
        if c.tier == 1:
            assert o.exact, f"{c.name}: a partial sum of this lattice may not be representable"
            assert all(float(np.max(b)) == 0.0 for b in o.want_bound.values())
        else:
            pairs = ([(o.ref, o.bound)] + ([(o.ref_sum, o.bound_sum)] if c.fix else [])) if isinstance(c, R.GemmCase) else \
                    [(o.ref[k], o.want_bound[k][:o.ref[k].size]) for k in o.ref] if isinstance(c, R.HeadsCase) else [(o.ref, o.bound)]
            for ref, bound in pairs:
                assert R.cap_ok(ref, bound), (c.name, float(np.max(bound)), float(np.abs(ref).max()))
                worst_cap = max(worst_cap, float(np.max(bound)) / float(np.abs(ref).max()))
    print(f"largest bound / max|reference| over the real-valued cases: {worst_cap:.3g} (cap {R.CAP})")
    assert 0 < worst_cap <= R.CAP


def test_the_model_equals_the_reference_on_lattices_and_stays_inside_the_bound_elsewhere():
    worst, n = {}, {}
    for c in R.all_cases():
        o = R.build(c)
        fails, ratio = R.compare(c, o, R.model(c, o))
        assert not fails, fails[0]
        key = (c.name[0], c.tier)
        n[key] = n.get(key, 0) + 1
        worst[key] = max(worst.get(key, 0.0), ratio)
    for key in sorted(n):
        print(f"route {key[0]} tier {key[1]}: {n[key]} cases, float32 model worst error / bound {worst[key]:.3g}")
    assert all(worst[k] == 0.0 for k in worst if k[1] == 1) and all(0.0 < worst[k] < 1.0 for k in worst if k[1] == 2)


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_is_caught_in_each_tier_it_can_affect(mut):
    caught = {}
    for c in R.all_cases():
        if c.tier in caught or c.tier not in MUTATION_TIERS[mut] or not R.mutation_applies(mut, c):
            continue
        o = R.build(c)
        fails, _ = R.compare(c, o, R.model(c, o, mut))
        if fails:
            caught[c.tier] = fails[0]
    for tier in MUTATION_TIERS[mut]:
        assert tier in caught, f"{mut}: no tier-{tier} case fails"
        print(f"{mut}: tier {tier}: {caught[tier]}")


@pytest.mark.parametrize("kind", ["gemm", "heads", "logits"])
def test_every_mutation_is_caught_on_every_kind_of_entry_point_it_applies_to(kind):
    """... not only somewhere: per entry point family, in some tier"""
    cases = {"gemm": R.gemm_cases(), "heads": R.heads_cases(), "logits": R.logits_cases()}[kind]
    for mut in R.MUTATIONS:
        mine = [c for c in cases if R.mutation_applies(mut, c)]
        if not mine:
            continue
        assert any(R.compare(c, R.build(c), R.model(c, R.build(c), mut))[0] for c in mine), (kind, mut)


def test_the_failure_message_names_slab_element_and_k_tile():
    c = next(c for c in R.route_a_cases() if c.tier == 1 and c.nsplit == 3 and c.K == 1000 and c.splits > 1)
    o = R.build(c)
    fails, _ = R.compare(c, o, R.model(c, o, "slab_starts_a_tile_late"))
    assert "slab 0" in fails[0] and "a missing 'all terms' of K tile 0" in fails[0], fails[0]
    fails, _ = R.compare(c, o, R.model(c, o, "drop_a_lo_b_hi"))
    assert "a missing 'a_lo b_hi' of K tile" in fails[0] or "matches no single K tile" in fails[0], fails[0]
    c = next(c for c in R.route_c_cases() if c.tier == 1 and c.N == 16 and c.b_off == 16)
    o = R.build(c)
    assert "canary overwritten" in R.compare(c, o, R.model(c, o, "store_32_columns"))[0][0]
    c = R.logits_cases()[0]
    o = R.build(c)
    assert "cell" in R.compare(c, o, R.model(c, o, "swap_qq_and_h"))[0][0]
