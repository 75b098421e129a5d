"""CPU: the host side of the nearest-neighbour read-out -- the reference of tests/_knn_reference.py against rational arithmetic and
against itself on lattice data, ``data.vote_labels``, the argument refusals of ``latent_neighbors`` / ``transfer_labels`` (on objects
that are no model: they must refuse before they touch one), tools/knn_host_check.py at its small shapes, and the shape functions
``spv_knn_splits`` / ``spv_knn_ws_bytes``.  No GPU calls."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests._knn_reference import exact_d2, exact_d2_fraction, knn_ref, round_fraction_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_fraction_rounding_to_float32():
    one, ulp = Fraction(1), Fraction(1, 2 ** 23)
    assert round_fraction_f32(one + ulp / 2) == np.float32(1.0)                            # a tie: to even
    assert round_fraction_f32(one + 3 * ulp / 2) == np.float32(1.0) + np.float32(2.0 ** -22)   # a tie: to even, upwards
    assert round_fraction_f32(one + ulp / 2 + Fraction(1, 2 ** 80)) == np.float32(1.0 + 2.0 ** -23)
    assert round_fraction_f32(Fraction(1, 2 ** 150)) == 0 and round_fraction_f32(Fraction(5, 2 ** 151)) == np.float32(2.0 ** -149)   # subnormals
    assert round_fraction_f32(Fraction(3, 2 ** 150)) == np.float32(2.0 ** -148)   # 1.5 units of 2^-149: a tie, to even
    assert round_fraction_f32(Fraction(2) ** 128 - Fraction(2) ** 103) == np.inf and np.isfinite(round_fraction_f32(Fraction(2) ** 128 - Fraction(2) ** 103 - 1))


def test_vectorised_chain_equals_rational_arithmetic():
    """a few thousand pairs: random data at several scales, and accumulators built to sit on float32 midpoints, where float64 loses the
    bit that decides (u * u + acc = s + e with s a midpoint and e != 0)"""
    rng = np.random.default_rng(0)
    pairs = []
    for D, scale in ((1, 1.0), (3, 1e-3), (25, 1.0), (35, 30.0), (64, 1e15), (10, 1e-21)):
        Q, C = (rng.standard_normal((20, D)) * scale).astype(np.float32), (rng.standard_normal((25, D)) * scale).astype(np.float32)
        d = exact_d2(Q, C)
        pairs += [(Q[i], C[j], d[i, j]) for i in range(20) for j in range(25)]
    # near-midpoint constructions, D = 2 or 3: term 0 leaves a tiny acc = 2^-2m, term 1 adds u^2 = ((1 + 2^-12) 2^j)^2 = (1 + 2^-11 + 2^-24) 4^j,
    # which has 25 significant bits and sits exactly between two float32 values.  Once 2m > 53 - 2j or so, float64 absorbs the tiny acc
    # (s = u^2, e = acc > 0) and only the residual says that the sum lies ABOVE the midpoint.  All terms are non-negative, so e < 0 on a
    # midpoint needs a sum that float64 rounds UP to one: other widths w and a third term are thrown in for that.
    for m in range(14, 60):
        for j in range(-3, 4):
            for w in (1 + 2.0 ** -12, 1 + 2.0 ** -12 + 2.0 ** -23, 1 + 2.0 ** -11 + 2.0 ** -12, 1.75 + 2.0 ** -12):
                for tail in ((), (2.0 ** -m,), (1.0,)):
                    q = np.array([2.0 ** -m, w * 2.0 ** j, *tail], np.float32)
                    z = np.zeros_like(q)
                    pairs.append((q, z, exact_d2(q[None], z[None])[0, 0]))
    assert len(pairs) > 3000
    wrong = [(q, c) for q, c, got in pairs if _bits(exact_d2_fraction(q, c)) != _bits(got)]
    assert not wrong
    # the constructions do reach the case the correction exists for: plain float64-then-float32 rounding fails on some of them
    naive = lambda q, c: np.float32(np.float64(np.float32(q[0] - c[0])) ** 2 + np.float64(np.float32(q[1] - c[1])) ** 2)
    assert any(_bits(naive(q, c)) != _bits(got) for q, c, got in pairs if len(q) == 2 and q[0] < 1e-3)


def test_reference_on_lattice_data():
    """multiples of 1/4 in [-8, 8]: every operation is exact in float32, so plain float32 numpy IS the chain"""
    rng = np.random.default_rng(1)
    Q, C = (rng.integers(-32, 33, (n, 7)).astype(np.float32) / 4 for n in (11, 90))
    plain = ((Q[:, None, :] - C[None]) ** 2).sum(-1, dtype=np.float32)
    d = exact_d2(Q, C)
    np.testing.assert_array_equal(d, plain)
    ex = np.array([3, -1, 90, 0, 5, 6, 7, 8, 9, 10, 89], np.int32)
    idx, dist = knn_ref(Q, C, 12, ex)
    for i in range(11):
        pairs = sorted((plain[i, j], j) for j in range(90) if j != ex[i])[:12]
        assert [j for _, j in pairs] == idx[i].tolist() and [v for v, _ in pairs] == dist[i].tolist()
    assert (np.diff(dist, axis=1) == 0).any()   # ties are there
    idx, dist = knn_ref(Q, C[:5], 8)
    assert (idx[:, 5:] == -1).all() and np.isinf(dist[:, 5:]).all() and (idx[:, :5] >= 0).all()
    C2 = C[:6].copy()
    C2[2, 1], C2[4, 0] = np.nan, np.inf
    idx, _ = knn_ref(Q, C2, 6)
    assert (idx[:, 4:] == -1).all() and not np.isin(idx, (2, 4)).any()


def test_vote_labels():
    from spvipes_amd.data import vote_labels
    codes = np.array([2, 1, 1, 0, 2])
    idx = np.array([[0, 1, 2], [-1, -1, -1], [3, -1, 0], [1, 4, -1], [4, 0, 3], [3, 3, 3]])
    pred, conf, n = vote_labels(idx, codes, 3)
    assert pred.tolist() == [1, -1, 0, 1, 2, 0]          # row 2: codes 0 and 2 tie -> 0; row 3: codes 1 and 2 tie -> 1
    assert n.tolist() == [3, 0, 2, 2, 3, 3]
    np.testing.assert_array_equal(conf, np.array([2 / 3, np.nan, 1 / 2, 1 / 2, 2 / 3, 1.0]))
    pred, conf, n = vote_labels(np.zeros((0, 4), np.int32), codes, 3)
    assert pred.shape == conf.shape == n.shape == (0,)
    with pytest.raises(ValueError):
        vote_labels(np.array([[5]]), codes, 3)
    with pytest.raises(ValueError):
        vote_labels(np.array([[0]]), codes, 2)
    with pytest.raises(ValueError):
        vote_labels(np.array([0, 1]), codes, 3)


def test_transfer_frame():
    from spvipes_amd.data import transfer_frame
    f = transfer_frame(["c0", "c1", "c2"], np.array(["B", "T"]), np.array([1, -1, 0]), np.array([0.5, np.nan, 1.0]), np.array([2, 0, 3]))
    assert list(f.columns) == ["predicted", "confidence", "n_neighbors"] and list(f.index) == ["c0", "c1", "c2"]
    assert f["predicted"].tolist() == ["T", None, "B"] and f["n_neighbors"].tolist() == [2, 0, 3] and np.isnan(f["confidence"].iloc[1])


REFUSED = [dict(k=0), dict(k=65), dict(k=2.5), dict(k=True), dict(latent="both"), dict(query=2), dict(target="all"), dict(query=True),
           dict(latent="private"), dict(latent="private", query="both", target="both"), dict(latent="private", query=1, target=0)]


@pytest.mark.parametrize("kw", REFUSED, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c in REFUSED])
def test_latent_neighbors_refuses_before_it_touches_the_model(kw):
    from spvipes_amd.model import spVIPES
    with pytest.raises(ValueError, match="|".join(kw)):
        spVIPES.latent_neighbors(object(), [[0], [1]], **kw)


def test_latent_neighbors_accepts_what_it_should():
    """valid arguments pass the check and go on to the model (an object without one: AttributeError)"""
    from spvipes_amd.model import spVIPES
    for kw in (dict(), dict(k=64, query="both", target="both"), dict(latent="private", query=1, target=1), dict(k=np.int64(3), query=0, target=0)):
        with pytest.raises(AttributeError):
            spVIPES.latent_neighbors(object(), [[0], [1]], **kw)


def test_transfer_labels_refusals():
    from spvipes_amd.model import spVIPES
    for kw, text in ((dict(source=2), "group"), (dict(target="both"), "group"), (dict(k=0), "k must"), (dict(k=100), "k must"), (dict(latent="x"), "latent"),
                     (dict(latent="private"), "private"), (dict(query=1), "query")):
        with pytest.raises(ValueError, match=text):
            spVIPES.transfer_labels(object(), [[0], [1]], **kw)
    with pytest.raises(AttributeError):
        spVIPES.transfer_labels(object(), [[0], [1]])


def test_signatures():
    import inspect
    from spvipes_amd.model import spVIPES
    p = inspect.signature(spVIPES.latent_neighbors).parameters
    assert list(p) == ["self", "group_indices_list", "k", "query", "target", "latent", "give_mean", "include_self", "batch_size", "return_numpy", "_noise"]
    assert (p["k"].default, p["query"].default, p["target"].default, p["latent"].default, p["give_mean"].default, p["include_self"].default) == (15, 0, 1, "shared", True, False)
    p = inspect.signature(spVIPES.transfer_labels).parameters
    assert list(p) == ["self", "group_indices_list", "source", "target", "labels", "k", "neighbor_kwargs"]
    assert (p["source"].default, p["target"].default, p["labels"].default, p["k"].default) == (1, 0, "cell_type", 15)
    assert callable(spVIPES._latents_on_device)


def test_host_check_tool_small_shapes():
    """the kernels' own chain, order, insertion and merge, compiled for the CPU, against the reference (no sanitizer here)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "knn_host_check.py"), "--small"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout and "DIFFER" not in r.stdout


def test_splits_and_workspace_values():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    from spvipes_amd.knn_ops import KNN_DMAX, KNN_KMAX, KNN_SPLIT_MAX
    build()
    lib = _abi.load()
    TQ, TC = lib.spv_knn_tile_q(), lib.spv_knn_tile_c()
    assert (TQ, TC) == (128, 64) and (KNN_DMAX, KNN_KMAX, KNN_SPLIT_MAX) == (64, 64, 64)
    s = lib.spv_knn_splits
    assert s(50000, 50000) == 3          # 391 query tiles: 3 chunks make 1173 workgroups, 4.6 per CU
    assert s(100000, 100000) == 1        # 782 query tiles: two per CU and more
    assert s(65536, 50000) == 1 and s(65408, 50000) == 3   # 512 tiles is the threshold; 511 take ceil(1024 / 511) chunks
    assert s(1, 10 ** 6) == 64 and s(1, 64 * 4 * TC) == 64 and s(1, 64 * 4 * TC - 1) == 63    # capped; a chunk holds at least 4 LDS tiles
    assert s(300, 260) == 1 and s(1, 0) == 1 and s(0, 5) == 1 and s(-3, -3) == 1 and s(1, 2 * 4 * TC) == 2
    w = lib.spv_knn_ws_bytes
    assert w(50000, 15, 3) == 3 * 50000 * 15 * 8 == 18_000_000
    assert w(50000, 15, 1) == 0 and w(50000, 15, 0) == 0 and w(0, 15, 3) == 0 and w(5, 0, 3) == 0
    assert w(2 ** 31 - 1, 64, 64) == (2 ** 31 - 1) * 64 * 64 * 8     # 64-bit arithmetic
