"""Shared by the PCA tests: the planted-cluster count generator, the fp64 reference of count_pca (the operand of csrc/spv_pca.h with
np.log1p in fp64, the covariance, eigh) and a numpy model of pca_ops.block_lanczos.  Test infrastructure."""
import numpy as np

from tests._duck import DuckAnnData

N_CELLS = (333, 270)
N_GENES = (200, 230)
N_UNIVERSE = 270          # group 0 holds genes 0 .. 199 of the universe, group 1 genes 40 .. 269 (in a shuffled order): 160 pair
N_FACTORS = 5


def planted_counts(n_cells: int, loadings: np.ndarray, rng) -> np.ndarray:
    """Poisson counts [n_cells, genes] of cells that are 0.8 one-hot + 0.2 Dirichlet(0.5) mixtures of the factors' gene profiles
    (``loadings`` [factors, genes], rows normalised here), at a depth uniform in [300, 3000)"""
    k = loadings.shape[0]
    mix = 0.8 * np.eye(k)[rng.integers(0, k, n_cells)] + 0.2 * rng.dirichlet(np.full(k, 0.5), n_cells)
    profile = mix @ (loadings / loadings.sum(1, keepdims=True))
    depth = rng.uniform(300, 3000, n_cells)
    return rng.poisson(profile / profile.sum(1, keepdims=True) * depth[:, None]).astype(np.float64)


def planted_loadings(n_genes: int, rng, n_factors: int = N_FACTORS) -> np.ndarray:
    """Gamma(0.3) loadings + 0.02 for ``n_factors`` factors"""
    return rng.gamma(0.3, 1.0, (n_factors, n_genes)) + 0.02


def make_pca_duck(seed: int = 0, sparse: bool = False, names: bool = True, dtype=np.float32):
    """The duck-typed AnnData of the API tests: 333 + 270 cells, 200 / 230 genes of which 160 pair by name ("a_g17" / "b_g17"), the
    groups' blocks on the diagonal of X; also returns the groups' count blocks and the universe positions of their genes"""
    rng = np.random.default_rng(seed)
    load = planted_loadings(N_UNIVERSE, rng)
    uni = [np.arange(N_GENES[0]), 40 + rng.permutation(N_GENES[1])]
    blocks = [planted_counts(N_CELLS[g], load[:, uni[g]], rng) for g in range(2)]
    blocks[0][7, :] = 0          # a cell without counts
    n, G = sum(N_CELLS), sum(N_GENES)
    X = np.zeros((n, G), dtype)
    X[:N_CELLS[0], :N_GENES[0]] = blocks[0]
    X[N_CELLS[0]:, N_GENES[0]:] = blocks[1]
    order = rng.permutation(n)   # the groups' cells are interleaved in adata order
    X = X[order]
    group_of = np.where(order < N_CELLS[0], 0, 1)
    obs_idx = [np.nonzero(group_of == g)[0] for g in range(2)]
    blocks = [X[obs_idx[g]][:, (0 if g == 0 else N_GENES[0]):(N_GENES[0] if g == 0 else G)].astype(np.float64) for g in range(2)]
    obs = {"groups": np.where(group_of == 0, "a", "b"), "indices": np.zeros(n, np.int32)}
    for g in range(2):
        obs["indices"][obs_idx[g]] = np.arange(len(obs_idx[g]))
    uns = {"groups_lengths": {0: N_GENES[0], 1: N_GENES[1]}, "groups_var_indices": [np.arange(N_GENES[0]), N_GENES[0] + np.arange(N_GENES[1])],
           "groups_obs_indices": obs_idx, "groups_obs_names": None, "groups_var_names": None, "groups_mapping": {0: "a", 1: "b"}}
    if sparse:
        import scipy.sparse as sp
        X = sp.csr_matrix(X)
    ad = DuckAnnData(X, obs, uns)
    if names:
        ad.var_names = np.array([f"a_g{j}" for j in uni[0]] + [f"b_g{j}" for j in uni[1]])
    ad.obsm = {}
    return ad, blocks, uni


def paired_positions(uni):
    """the default pairing of make_pca_duck's genes: the universe genes both groups hold, in group 0's order -> (pos0, pos1)"""
    where1 = {int(j): i for i, j in enumerate(uni[1])}
    pos0 = [i for i, j in enumerate(uni[0]) if int(j) in where1]
    return np.asarray(pos0), np.asarray([where1[int(uni[0][i])] for i in pos0])


def weights(block: np.ndarray, target_sum: float = 1e4) -> np.ndarray:
    """fp32(target_sum / the cell's total over ALL of the group's genes); 0 for a cell without counts"""
    total = block.sum(1)
    return np.where(total > 0, target_sum / np.where(total > 0, total, 1.0), 0.0).astype(np.float32)


def lognorm(block: np.ndarray, w=None) -> np.ndarray:
    """a = log1p(u) in fp64 of the kernels' u: ONE fp32 multiply of the fp32 count and the fp32 weight"""
    c = block.astype(np.float32)
    u = c if w is None else (c * w.astype(np.float32)[:, None]).astype(np.float32)
    return np.log1p(u.astype(np.float64))


def reference_pca(parts, n_comps: int, scale: bool = False):
    """``parts``: the groups' fp64 matrices of a over the joint columns, stacked -> dict of X (centred, scaled, fp64), mean, var,
    eigenvalues (all, descending, of X^T X / (n - 1)), vectors [p, p], total variance"""
    A = np.concatenate(parts, 0)
    n = A.shape[0]
    mean = A.mean(0)
    var = ((A - mean) ** 2).sum(0) / (n - 1)
    sc = np.where(var > 0, 1.0 / np.sqrt(np.where(var > 0, var, 1.0)), 0.0) if scale else np.ones_like(var)
    X = (A - mean) * sc
    lam, vec = np.linalg.eigh(X.T @ X / (n - 1))
    lam, vec = lam[::-1], vec[:, ::-1]
    return dict(X=X, mean=mean, var=var, lam=lam, vec=vec, total=float((var * sc * sc).sum()), n=n, top=vec[:, :n_comps])


def reference_joint(blocks, uni, n_comps: int = 5, scale: bool = False, normalize: bool = True):
    pos = paired_positions(uni)
    parts = [lognorm(blocks[g], weights(blocks[g]) if normalize else None)[:, pos[g]] for g in range(2)]
    return reference_pca(parts, n_comps, scale)


def lanczos_model(X: np.ndarray, n_comps: int, block: int, tol: float = 1e-4, max_blocks: int = 12, seed: int = 0):
    """pca_ops.block_lanczos in numpy on the operator V -> fp64(fp32(X))^T (fp32(X) fp32(V)), products in fp32 -> (theta, vectors, blocks
    used, converged) without restarts"""
    p = X.shape[1]
    X32 = X.astype(np.float32)
    cur = np.linalg.qr(np.random.default_rng(seed).standard_normal((p, block)))[0]
    Q, AQ = np.zeros((p, 0)), np.zeros((p, 0))
    for step in range(min(max_blocks, p // block)):
        v32 = cur.astype(np.float32)
        Y = X32 @ v32
        Z = (X32.T @ Y).astype(np.float64)
        Q, AQ = np.concatenate([Q, v32.astype(np.float64)], 1), np.concatenate([AQ, Z], 1)
        T = Q.T @ AQ
        theta, S = np.linalg.eigh(0.5 * (T + T.T))
        theta, S = theta[::-1], S[:, ::-1]
        top = S[:, :n_comps]
        res = np.linalg.norm(AQ @ top - (Q @ top) * theta[:n_comps], axis=0)
        if res.max() <= tol * theta[0]:
            return theta[:n_comps], Q @ top, step + 1, True
        W = Z
        for _ in range(2):
            W = W - Q @ (Q.T @ W)
        cur = np.linalg.qr(W)[0]
    return theta[:n_comps], Q @ top, step + 1, False
