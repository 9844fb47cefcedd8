"""KL refit of usages and spectra (models.refit under beta_loss = kullback-leibler,
ops.reference.kl_refit, consensus refit_loss="match") on the CPU: the float64 twin against
sklearn's MU solver with the spectra fixed, the float32 public path against the twin, the
spectra side, gene shards, and the public surface."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.api import cNMF
from cnmf_torch_amd.cli import build_parser
from cnmf_torch_amd.models import refit
from cnmf_torch_amd.ops import reference
from cnmf_torch_amd.utils.io import load_df_from_npz, save_df_to_npz
from cnmf_torch_amd.utils.synthetic import simulate_counts

H_TOL = dict(rtol=1e-4, atol=1e-6)       # usages: the sparse-KL bound (test_sparse_kl_xwide_gpu)
N, G, K, CHUNK = 96, 64, 5, 32


@functools.lru_cache(maxsize=None)
def _problem():
    """Poisson counts 96 x 64 from K = 5 programs, ~25 % non-zero, no zero row, float64, and
    the generating spectra W (K x G) the refits hold fixed."""
    rng = np.random.default_rng(7)
    W = rng.gamma(0.6, 1.0, size=(K, G)) + 0.02
    H = rng.dirichlet(np.full(K, 0.4), size=N)
    lam = H @ W
    X = rng.poisson(lam * (0.29 / lam.mean())).astype(np.float64)
    for i in np.flatnonzero(X.sum(1) == 0):
        X[i, rng.integers(G)] = 1.0
    assert 0.20 < (X != 0).mean() < 0.30 and (X.sum(1) > 0).all()
    return X, W


def _kl(X, P):
    pos = X > 0
    return float((X[pos] * np.log(X[pos] / P[pos])).sum() - X.sum() + P.sum())


def _csr64(X):
    m = sp.csr_matrix(X)
    return ops.KLCSR(torch.from_numpy(m.indptr.astype(np.int32)),
                     torch.from_numpy(m.indices.astype(np.int32)),
                     torch.from_numpy(m.data.astype(np.float64)), *m.shape)


def _init64(n, k, seed=0):
    return refit._init_HT(k, n, None, torch.device("cpu"), torch.float32, seed).double()


def test_twin_reaches_sklearn_objective_and_beats_frobenius_refit():
    """reference.kl_refit (chunks of 32 rows, tol 1e-6 on the chunk rule) against sklearn's MU
    solver with the spectra fixed: the KL objectives agree to 1e-6 relative (both sit at the
    minimum over H; the sketch this bound comes from measured 6e-8).  And the KL refit has a
    lower KL objective than the Frobenius refit of the same data."""
    from sklearn.decomposition import non_negative_factorization

    X, W = _problem()
    Hs, _, _ = non_negative_factorization(X, H=W, update_H=False, solver="mu",
                                          beta_loss="kullback-leibler", max_iter=2000,
                                          tol=1e-10, n_components=K)
    HT = _init64(N, K)
    it = torch.zeros(N // CHUNK, dtype=torch.int32)
    reference.kl_refit(_csr64(X), HT, torch.from_numpy(W), CHUNK, 5000, 1e-6, iters=it)
    f_sk, f_us = _kl(X, Hs @ W), _kl(X, HT.t().numpy() @ W)
    print("KL sklearn", f_sk, "twin", f_us, "rel", abs(f_us - f_sk) / f_sk, "steps", it.tolist())
    assert (it > 1).all() and (it < 5000).all()
    assert abs(f_us - f_sk) <= 1e-6 * f_sk
    Hf = refit.fit_H_online(X, W, chunk_size=CHUNK, device="cpu")
    Hk = refit.fit_H_online(X, W, chunk_size=CHUNK, device="cpu", beta_loss="kullback-leibler")
    f_fro, f_kl = _kl(X, Hf.astype(np.float64) @ W + 1e-300), _kl(X, Hk.astype(np.float64) @ W)
    print("KL of the Frobenius refit", f_fro, "of the KL refit", f_kl)
    assert f_kl < f_fro


@pytest.mark.parametrize("form", ["dense", "scipy", "tensor", "device_csr"])
def test_float32_public_path_matches_the_float64_twin(form):
    """fit_H_online(beta_loss=1, device="cpu") at the production h_tol vs the twin in float64
    from the same seeded init: the same step count per chunk, the usages within the sparse
    KL bound.  Every input form gives the same CSR, so the same result."""
    X, W = _problem()
    HT = _init64(N, K, seed=3)
    it64 = torch.zeros(3, dtype=torch.int32)
    trace = []
    reference.kl_refit(_csr64(X), HT, torch.from_numpy(W), CHUNK, 200, 0.05, iters=it64,
                       trace=trace)
    assert min(abs(r - 0.05) for _, _, r in trace) > 1e-3 * 0.05    # no decision near tol
    Xin = {"dense": X, "scipy": sp.csr_matrix(X), "tensor": torch.from_numpy(X).float(),
           "device_csr": ops.sparse.DeviceCSR.from_scipy(sp.csr_matrix(X.astype(np.float32)))}[form]
    it32 = torch.zeros(3, dtype=torch.int32)
    H = refit.fit_H_online(Xin, W, chunk_size=CHUNK, device="cpu", beta_loss=1, random_state=3,
                           iters=it32)
    assert H.dtype == np.float32 and H.shape == (N, K)
    assert it32.tolist() == it64.tolist()
    ratio = float(((torch.from_numpy(H).double() - HT.t()).abs()
                   / (H_TOL["rtol"] * HT.t().abs() + H_TOL["atol"])).max())
    print("steps", it32.tolist(), "usages: x tolerance", ratio)
    torch.testing.assert_close(torch.from_numpy(H).double(), HT.t(), **H_TOL)


def test_h_init_is_clamped_and_used():
    X, W = _problem()
    H0 = np.random.default_rng(1).normal(0.5, 0.5, size=(N, K))
    a = refit.fit_H_online(X, W, H_init=H0, chunk_size=CHUNK, beta_loss=1.0)
    b = refit.fit_H_online(X, W, H_init=np.clip(H0, 0, None), chunk_size=CHUNK, beta_loss=1.0)
    assert np.array_equal(a, b) and (a >= 0).all()


def test_spectra_side_is_the_usage_refit_of_the_transpose():
    """fit_spectra_online(X, U, beta_loss=1) == fit_H_online(X.T, U.T, beta_loss=1).T from the
    same seeded init (the usage refit draws it at row_offset 0, the spectra refit at
    col_offset 0: the same stream)."""
    X, _ = _problem()
    U = np.random.default_rng(2).random((N, K)) + 0.05
    it_s, it_h = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    S = refit.fit_spectra_online(X, U, chunk_size=40, beta_loss=1, iters=it_s)
    Ht = refit.fit_H_online(X.T.copy(), U.T.copy(), chunk_size=40, beta_loss=1, iters=it_h)
    assert S.shape == (K, G)
    assert it_s.tolist() == it_h.tolist() and (it_s > 0).all()
    assert np.array_equal(S, Ht.T)
    Ssp = refit.fit_spectra_online(sp.csr_matrix(X), U, chunk_size=40, beta_loss=1)
    assert np.array_equal(S, Ssp)


def test_gene_shards_of_whole_chunks_reproduce_the_unsharded_refit():
    X, _ = _problem()
    U = np.random.default_rng(2).random((N, K)) + 0.05
    full = refit.fit_spectra_online(X, U, chunk_size=16, beta_loss=1, random_state=5)
    blocks = refit.gene_blocks(G, 16, 2)
    assert blocks == [(0, 32), (32, 64)]
    for Xin in (X, ops.sparse.DeviceCSR.from_scipy(sp.csr_matrix(X.astype(np.float32)))):
        parts = [refit.fit_spectra_online(refit.col_block(Xin, g0, g1), U, chunk_size=16,
                                          beta_loss=1, random_state=5, col_offset=g0)
                 for g0, g1 in blocks]
        assert np.array_equal(np.concatenate(parts, axis=1), full)


def test_csr_transpose_twin_is_scipys():
    X, _ = _problem()
    X = X.copy()
    X[:, 5] = 0.0
    X[11] = 0.0
    m = sp.csr_matrix(X.astype(np.float32))
    t = ops.csr_transpose(refit.kl_csr_of(m, "cpu"))
    ref = m.T.tocsr()
    ref.sort_indices()
    assert (t.n_rows, t.n_cols) == (G, N)
    assert np.array_equal(t.rowptr.numpy(), ref.indptr)
    assert np.array_equal(t.col.numpy(), ref.indices) and np.array_equal(t.val.numpy(), ref.data)
    big = ops.KLCSR(torch.tensor([0, 2 ** 31], dtype=torch.int64), t.col, t.val, 1, 5)
    with pytest.raises(ValueError, match="int32"):
        ops.csr_transpose(big)


def test_unsupported_losses_raise():
    X, W = _problem()
    for bad in ("itakura-saito", 0, 1.5, "kl", None):
        with pytest.raises(ValueError, match="frobenius.*kullback-leibler"):
            refit.fit_H_online(X, W, beta_loss=bad)
        with pytest.raises(ValueError, match="frobenius.*kullback-leibler"):
            refit.fit_spectra_online(X, np.ones((N, K)), beta_loss=bad)
    a = refit.fit_H_online(X, W, chunk_size=CHUNK)
    assert np.array_equal(a, refit.fit_H_online(X, W, chunk_size=CHUNK, beta_loss=2))
    assert np.array_equal(a, refit.fit_H_online(X, W, chunk_size=CHUNK, beta_loss="frobenius"))


def test_cli_accepts_refit_loss():
    p = build_parser()
    base = ["consensus", "--output-dir", "o", "--name", "n", "--components", "3"]
    assert p.parse_args(base).refit_loss == "frobenius"
    assert p.parse_args(base + ["--refit-loss", "match"]).refit_loss == "match"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--refit-loss", "itakura-saito"])


def _run(tmp_path, name, **kw):
    Xc, cells, genes = simulate_counts(220, 120, 3, seed=4, sparse=False)
    fn = str(tmp_path / "c.df.npz")
    if not os.path.exists(fn):
        save_df_to_npz(pd.DataFrame(Xc, index=cells, columns=genes), fn)
    obj = cNMF(output_dir=str(tmp_path), name=name)
    obj.prepare(fn, components=[3], n_iter=4, seed=1, num_highvar_genes=70, batch_size=64, **kw)
    obj.factorize(verbose=False, device="cpu")
    obj.combine()
    return obj


_ARTIFACTS = ("consensus_usages", "consensus_spectra", "gene_spectra_tpm", "gene_spectra_score")


def _consensus_files(obj, **kw):
    obj.consensus(3, density_threshold=2.0, show_clustering=False, device="cpu", **kw)
    out = {}
    for key in _ARTIFACTS:
        with open(obj.paths[key] % (3, "2_0"), "rb") as fh:
            out[key] = fh.read()
    out["usages_df"] = load_df_from_npz(obj.paths["consensus_usages"] % (3, "2_0"))
    out["spectra_df"] = load_df_from_npz(obj.paths["consensus_spectra"] % (3, "2_0"))
    return out


def test_consensus_match_on_a_kl_run_refits_under_kl(tmp_path):
    """refit_loss="match" on a KL run: the written usages differ from the default's; with the
    final usage refit off the usages are the refit of the normalised counts against the
    consensus spectra, the same spectra in both runs, and the matched ones have the lower KL
    objective there."""
    obj = _run(tmp_path, "kl", beta_loss="kullback-leibler")
    assert obj._refit_loss("match") == "kullback-leibler"
    d = _consensus_files(obj)
    m = _consensus_files(obj, refit_loss="match")
    assert d["consensus_spectra"] == m["consensus_spectra"]
    assert d["consensus_usages"] != m["consensus_usages"]
    assert d["gene_spectra_tpm"] != m["gene_spectra_tpm"]
    Xn = obj._read_norm_counts(torch.device("cpu")).X
    X = np.asarray(Xn.toarray() if sp.issparse(Xn) else Xn, dtype=np.float64)
    f = {}
    for name, kw in (("default", {}), ("match", {"refit_loss": "match"})):
        r = _consensus_files(obj, refit_usage=False, **kw)
        U, S = r["usages_df"].values.astype(np.float64), r["spectra_df"].values.astype(np.float64)
        f[name] = _kl(X, U @ S + 1e-300)
    print("KL objective of the written usages: default", f["default"], "match", f["match"])
    assert f["match"] < f["default"]


def test_consensus_match_on_a_frobenius_run_is_the_default(tmp_path):
    obj = _run(tmp_path, "fro")
    assert obj._refit_loss("match") == "frobenius"
    d = _consensus_files(obj)
    m = _consensus_files(obj, refit_loss="match")
    for key in _ARTIFACTS:
        assert d[key] == m[key], key


def test_consensus_match_on_another_beta_raises_before_any_work(tmp_path):
    obj = _run(tmp_path, "fro2")
    from cnmf_torch_amd.utils.io import dump_yaml, load_yaml

    kw = load_yaml(obj.paths["nmf_run_parameters"])
    kw["beta_loss"] = "itakura-saito"
    dump_yaml(kw, obj.paths["nmf_run_parameters"])
    with pytest.raises(ValueError, match="match.*itakura-saito"):
        obj.consensus(3, density_threshold=2.0, show_clustering=False, device="cpu",
                      refit_loss="match")
    assert not os.path.exists(obj.paths["consensus_usages"] % (3, "2_0"))
    with pytest.raises(ValueError, match="frobenius.*kullback-leibler"):
        obj.refit_usage(np.ones((4, 3)), np.ones((2, 3)), loss="itakura-saito")
