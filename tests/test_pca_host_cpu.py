"""CPU: the host half of count_pca / spVIPES.pca -- the fp64 reference of the GPU tests against scikit-learn, the pairing rule, the sign
rule, every refusal ahead of device work, the CPU check of the kernels' core (tools/pca_host_check.py) and a numpy model of the block
Lanczos iteration on a float32-rounded operator.  No GPU calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _pca_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def planted():
    ad, blocks, uni = R.make_pca_duck(0)
    return ad, blocks, uni, R.reference_joint(blocks, uni)


def test_reference_has_the_planted_gap_and_matches_sklearn(planted):
    from sklearn.decomposition import PCA
    _ad, blocks, uni, ref = planted
    lam = ref["lam"]
    assert lam[4] - lam[5] >= 0.1 * lam[0]                      # five planted factors: the input cannot drift
    pos = R.paired_positions(uni)
    assert len(pos[0]) == 160 and ref["X"].shape == (603, 160)
    A = np.concatenate([R.lognorm(blocks[g], R.weights(blocks[g]))[:, pos[g]] for g in range(2)], 0)
    sk = PCA(n_components=5, svd_solver="full").fit(A)
    assert np.allclose(sk.explained_variance_, lam[:5], rtol=1e-10, atol=0)
    assert np.allclose(sk.explained_variance_ratio_, lam[:5] / ref["total"], rtol=1e-10, atol=0)
    assert np.allclose(np.abs(np.sum(sk.components_ * ref["top"].T, axis=1)), 1.0, atol=1e-9)   # the same vectors up to sign
    assert np.allclose(sk.mean_, ref["mean"], rtol=1e-12)


def test_pairing_rule(planted):
    from spvipes_amd.data import group_var_names, pca_group_keys, pca_pair_genes
    ad, _blocks, uni, _ref = planted
    names, keys = group_var_names(ad), pca_group_keys(ad.uns)
    assert keys == ["a", "b"]
    pos0, pos1, labels = pca_pair_genes(names, keys, None, list(R.N_GENES))
    want0, want1 = R.paired_positions(uni)
    assert np.array_equal(pos0, want0) and np.array_equal(pos1, want1) and pos0.dtype == np.int32
    assert list(labels[:3]) == [f"g{uni[0][i]}" for i in want0[:3]] and np.all(np.diff(pos0) > 0)   # group 0's order
    # without the keys nothing is stripped: "a_g40" and "b_g40" share nothing
    with pytest.raises(ValueError, match="share no gene name"):
        pca_pair_genes(names, None, None, list(R.N_GENES))
    # gene_list pairs by position: names or positions
    p0, p1, _ = pca_pair_genes(names, keys, [["a_g41", "a_g40"] + [f"a_g{j}" for j in range(50, 64)], ["b_g41", "b_g40"] + [f"b_g{j}" for j in range(50, 64)]], list(R.N_GENES))
    assert list(p0[:2]) == [41, 40] and [int(uni[1][i]) for i in p1[:2]] == [41, 40]
    q0, q1, lab = pca_pair_genes([None, None], None, [[3, 1, 2], [7, 9, 8]], [10, 10])
    assert list(q0) == [3, 1, 2] and list(q1) == [7, 9, 8] and list(lab) == [3, 1, 2]
    with pytest.raises(ValueError, match="equal length"):
        pca_pair_genes(names, keys, [[0, 1], [0, 1, 2]], list(R.N_GENES))
    with pytest.raises(ValueError, match="repeats a gene"):
        pca_pair_genes(names, keys, [[0, 1, 1], [0, 1, 2]], list(R.N_GENES))
    with pytest.raises(ValueError, match="BOTH groups"):
        pca_pair_genes(names, keys, [[0, 1, 2], None], list(R.N_GENES))
    with pytest.raises(ValueError, match="neither var_names nor"):
        pca_pair_genes([None, None], keys, None, list(R.N_GENES))
    # a repeated name pairs once, with its first occurrence
    r0, r1, _ = pca_pair_genes([np.array(["a_x", "a_y", "a_x"]), np.array(["b_y", "b_x", "b_y"])], ["a", "b"], None, [3, 3])
    assert list(r0) == [0, 1] and list(r1) == [1, 0]


def test_sign_rule():
    from spvipes_amd.data import pca_sign_flip
    c = np.array([[0.1, -0.9, 0.3], [0.5, 0.2, -0.5], [-0.5, 0.2, 0.5], [0.0, 0.0, 0.0], [-0.2, -0.2, 0.1]])
    assert list(pca_sign_flip(c)) == [-1.0, 1.0, -1.0, 1.0, -1.0]   # ties: the smaller gene index decides
    flipped = c * pca_sign_flip(c)[:, None]
    lead = flipped[np.arange(5), np.argmax(np.abs(flipped), axis=1)]
    assert np.all(lead >= 0)


def test_block_default_and_argument_limits():
    from spvipes_amd.data import PCA_MAX_COMPS, check_pca_args, pca_block
    assert [pca_block(k) for k in (1, 5, 8, 9, 24, 25, 40, 41, 50, 56)] == [16, 16, 16, 32, 32, 48, 48, 64, 64, 64] and PCA_MAX_COMPS == 56
    assert pca_block(20, 30) == 16 and pca_block(20, 40) == 32 and pca_block(50, 63) == 48 and pca_block(5, 10000) == 16
    with pytest.raises(ValueError, match="cannot be wider than the number of genes"):
        check_pca_args(20, n_cells=100, n_genes=30)
    assert check_pca_args(5, 1e-4, 0, 603, 160) == (5, 1e-4, 0)
    for bad, text in ((0, "between 1 and 56"), (57, "between 1 and 56"), (2.0, "between 1 and 56"), (True, "between 1 and 56")):
        with pytest.raises(ValueError, match=text):
            check_pca_args(bad)
    for bad in (0.0, 1.0, -1e-4, float("nan"), "1e-4", True):
        with pytest.raises(ValueError, match="tol must be a number in"):
            check_pca_args(5, tol=bad)
    for bad in (-1, 1 << 32, 0.5, False):
        with pytest.raises(ValueError, match="seed must be an integer"):
            check_pca_args(5, seed=bad)
    with pytest.raises(ValueError, match="at least 2 cells"):
        check_pca_args(1, n_cells=1, n_genes=100)
    with pytest.raises(ValueError, match="at least 16 genes"):
        check_pca_args(5, n_cells=100, n_genes=15)
    with pytest.raises(ValueError, match="smaller than the number of cells"):
        check_pca_args(20, n_cells=20, n_genes=100)
    with pytest.raises(ValueError, match="smaller than the number of genes"):
        check_pca_args(16, n_cells=100, n_genes=16)


def test_plan_and_every_refusal_of_count_pca_ahead_of_device_work(planted):
    from spvipes_amd.data import pca_plan
    ad, _blocks, uni, _ref = planted
    obs_idx, n_genes = ad.uns["groups_obs_indices"], list(R.N_GENES)
    plan = pca_plan(ad, n_genes, obs_idx, obs_idx, n_comps=5)
    assert plan["groups"] == [0, 1] and len(plan["cols"][0]) == 160 and plan["params"]["block"] == 16
    assert np.array_equal(plan["obs"], np.concatenate(obs_idx)) and np.array_equal(plan["rows"][1], np.arange(270))
    assert plan["genes"][0][0].startswith("a_g") and plan["genes"][1][0].startswith("b_g")
    own = pca_plan(ad, n_genes, obs_idx, [obs_idx[0][:50], []], n_comps=5, group=0)
    assert own["groups"] == [0] and len(own["cols"][0]) == 200 and len(own["obs"]) == 50
    sel = pca_plan(ad, n_genes, obs_idx, obs_idx, n_comps=5, group=1, gene_list=[None, np.arange(30)])
    assert sel["groups"] == [1] and list(sel["cols"][0]) == list(range(30))
    # fewer genes than the default block: the block shrinks to the largest multiple of 16 that fits, and still holds n_comps
    for genes, k, block in ((30, 5, 16), (30, 16, 16), (51, 30, 48), (63, 48, 48), (64, 50, 64), (40, 20, 32)):
        small = pca_plan(ad, n_genes, obs_idx, obs_idx, n_comps=k, group=0, gene_list=[np.arange(genes), None])
        assert small["params"]["block"] == block and k <= block <= genes
    for kwargs, exc, text in (
            (dict(target_sum=0), ValueError, "target_sum must be a positive finite number"),
            (dict(normalize=1), ValueError, "normalize must be True or False"),
            (dict(scale="yes"), ValueError, "scale must be True or False"),
            (dict(group=2), ValueError, "group must be 0 or 1"),
            (dict(n_comps=57), ValueError, "between 1 and 56"),
            (dict(tol=2.0), ValueError, "tol must be a number in"),
            (dict(seed=-1), ValueError, "seed must be an integer"),
            (dict(gene_list=[["a_g40"] * 20, [f"b_g{j}" for j in range(40, 60)]]), ValueError, "repeats a gene"),
            (dict(gene_list=[["a_nope"], ["b_g40"]]), KeyError, "a_nope"),
            (dict(gene_list=[np.arange(10), np.arange(10)]), ValueError, "at least 16 genes"),
            (dict(group=0, gene_list=[[1, 1] + list(range(20)), None]), ValueError, "repeats a gene"),
            (dict(group=0, gene_list=[np.arange(20), None], n_comps=20), ValueError, "smaller than the number of genes"),
            (dict(group=0, gene_list=[np.arange(30), None], n_comps=20), ValueError, "cannot be wider than the number of genes"),
            (dict(group=0, gene_list=[np.arange(63), None], n_comps=50), ValueError, "at most n_comps=48")):
        with pytest.raises(exc, match=text):
            pca_plan(ad, n_genes, obs_idx, obs_idx, **{**dict(n_comps=5), **kwargs})
    with pytest.raises(ValueError, match="do not belong to group 0"):
        pca_plan(ad, n_genes, obs_idx, [obs_idx[1], obs_idx[1]], n_comps=5)
    with pytest.raises(ValueError, match="row numbers in"):
        pca_plan(ad, n_genes, obs_idx, [[0, 9999], obs_idx[1]], n_comps=5)
    with pytest.raises(ValueError, match="at least one listed cell"):
        pca_plan(ad, n_genes, obs_idx, [obs_idx[0], []], n_comps=5)
    with pytest.raises(ValueError, match="one list of adata row numbers per group"):
        pca_plan(ad, n_genes, obs_idx, [obs_idx[0]], n_comps=5)
    nameless, _b, _u = R.make_pca_duck(0, names=False)
    with pytest.raises(ValueError, match="pass gene_list="):
        pca_plan(nameless, n_genes, obs_idx, obs_idx, n_comps=5)


def test_every_refusal_of_the_pca_classmethod_ahead_of_device_work(planted):
    from spvipes_amd.model import spVIPES
    ad, _blocks, _uni, _ref = planted
    for kwargs, exc, text in (
            (dict(counts_storage="csr"), ValueError, "counts_storage must be"),
            (dict(layer="counts"), KeyError, "layer 'counts' not found"),
            (dict(key_added=""), ValueError, "key_added must be"),
            (dict(group=0), ValueError, "takes the keyword arguments"),
            (dict(n_comps=0), ValueError, "between 1 and 56"),
            (dict(target_sum=-1.0), ValueError, "target_sum must be"),
            (dict(tol=0), ValueError, "tol must be a number in")):
        with pytest.raises(exc, match=text):
            spVIPES.pca(ad, **kwargs)
    broken, _b, _u = R.make_pca_duck(0)
    del broken.uns["groups_obs_indices"]
    with pytest.raises(ValueError, match="groups_obs_indices"):
        spVIPES.pca(broken)
    nameless, _b, _u = R.make_pca_duck(0, names=False)
    with pytest.raises(ValueError, match="pass gene_list="):
        spVIPES.pca(nameless, n_comps=5)
    assert "X_pca" not in ad.obsm and "pca" not in ad.uns   # nothing was written by a refused call


def test_pca_host_check_tool():
    """the kernels' core compiled for the CPU: operand bits, bounds, pieces against one piece (tools/pca_host_check.py)"""
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pca_host_check.py")], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "pca_host_check: ok" in done.stdout


@pytest.mark.parametrize("block", [16, 32])
def test_block_lanczos_model_reaches_tol_on_a_float32_operator(planted, block):
    _ad, _blocks, _uni, ref = planted
    theta, vec, n_blocks, converged = R.lanczos_model(ref["X"], 5, block, tol=1e-4, max_blocks=12)
    lam = ref["lam"]
    assert converged and n_blocks <= 12
    assert np.max(np.abs(theta / (ref["n"] - 1) - lam[:5])) <= 2e-4 * lam[0]
    # every Ritz vector lies in the reference's top-5 subspace up to the residual over the gap
    out = vec - ref["top"] @ (ref["top"].T @ vec)
    assert np.max(np.linalg.norm(out, axis=0)) <= 1e-4 / 0.1
