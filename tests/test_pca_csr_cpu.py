"""Sparse PCA from a CSR on CPU tensors: ops.sparse.gram / project (the torch paths that are
the CPU route and the twin of csrc/kernels/pca_csr.hip), models.pp.pca_csr against
pca_tensor of the dense matrix, pp.pca(backend="csr") and the pca_backend switch of
Preprocess.  Cases, oracle and tolerances: pca_csr_cases.py (test_pca_csr_gpu.py runs the
same checks through the kernels)."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import csr_cases as cc
import pca_csr_cases as pc
from cnmf_torch_amd import Preprocess
from cnmf_torch_amd.models import pp
from cnmf_torch_amd.ops import sparse as sops
from cnmf_torch_amd.utils.anndata_lite import AnnData
from cnmf_torch_amd.utils.synthetic import simulate_counts

DEV = "cpu"


@pytest.mark.parametrize("case", pc.exact_cases(), ids=lambda c: c.name)
def test_gram_small_integers_exact(case):
    pc.check_gram(case, DEV, exact=True)


@pytest.mark.parametrize("vd", ["float32", "float64"])
@pytest.mark.parametrize("in_dtype", ["float32", "float64"])
@pytest.mark.parametrize("col_map", ["nomap", "perm"])
@pytest.mark.parametrize("factor", pc.FACTORS)
def test_gram_transform_factors(factor, col_map, in_dtype, vd):
    pc.check_gram(cc.factor_case(factor, col_map, in_dtype), DEV, vd)


@pytest.mark.parametrize("vd", ["float32", "float64"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_gram_every_factor_permuting_map(dtype, vd):
    pc.check_gram(cc.rows_case(130, dtype, "perm"), DEV, vd)


@pytest.mark.parametrize("case", [pc.pairs_case(), pc.n_case(257), pc.nh_case(200),
                                  cc.rows_case(130, "float32", "perm")], ids=lambda c: c.name)
def test_gram_layout_feeds_the_kernel_walk(case):
    """The tile-packed layout the device pre-pass builds, walked the way csr_gram walks it
    (tile pairs I <= J, rows in order, outer product of the row's two tile segments, (I, J)
    mirrored): every segment fits a tile, its local columns are distinct and in range, and
    the walk gives the oracle's Gram."""
    B = sops.valued(case.csr(DEV).view(**case.kw()))
    cm = sops._map(B.xf.get("col_map"), DEV)
    tptr, lcol, val = (x.numpy() for x in sops._gram_layout(B, cm))
    n, nh = case.n, case.n_out
    T = -(-nh // pc.TILE)
    assert tptr.shape == (T * n + 1,) and tptr[0] == 0 and tptr[-1] == lcol.size == val.size
    assert (np.diff(tptr) >= 0).all() and np.diff(tptr).max() <= pc.TILE
    G = np.zeros((T * pc.TILE, T * pc.TILE))
    for I in range(T):
        for J in range(I, T):
            for r in range(n):
                a, b = slice(*tptr[I * n + r:I * n + r + 2]), slice(*tptr[J * n + r:J * n + r + 2])
                la, lb = lcol[a], lcol[b]
                assert np.unique(la).size == la.size and ((0 <= la) & (la < pc.TILE)).all()
                G[np.ix_(I * pc.TILE + la, J * pc.TILE + lb)] += np.outer(val[a], val[b])
            if I != J:
                blk = G[I * pc.TILE:(I + 1) * pc.TILE, J * pc.TILE:(J + 1) * pc.TILE]
                G[J * pc.TILE:(J + 1) * pc.TILE, I * pc.TILE:(I + 1) * pc.TILE] = blk.T
    assert not G[nh:].any() and not G[:, nh:].any()
    D, C = case.DC
    bound = 2 * cc.gamma(C.T @ C + 1) * (np.abs(D).T @ np.abs(D))
    assert (np.abs(G[:nh, :nh] - D.T @ D) <= bound).all()


@pytest.mark.parametrize("vd", ["float32", "float64"])
@pytest.mark.parametrize("shift", [False, True], ids=["noshift", "shift"])
@pytest.mark.parametrize("c", pc.C_LIST)
def test_project(c, shift, vd):
    pc.check_project(cc.rows_case(130), DEV, c, vd, shift)


def test_project_short_rows():
    for n in (1, 3, 4, 5):
        pc.check_project(cc.rows_case(n), DEV, 7, shift=True)


def test_empty_inputs_are_exact_zeros():
    for which in ("norows", "nonnz"):
        case = cc.empty_case(which)
        A = case.csr(DEV)
        G = sops.gram(A)
        assert tuple(G.shape) == (30, 30) and G.dtype == torch.float64 and not G.any()
        out = sops.project(A, torch.ones((30, 5), dtype=torch.float64))
        assert tuple(out.shape) == (case.n, 5) and not out.any()


def test_non_injective_col_map_raises():
    A = cc.rows_case(5).csr(DEV)
    cm = np.arange(600, dtype=np.int32) % 300          # two stored columns per output column
    V = A.view(col_map=cm, n_out=300)
    with pytest.raises(ValueError):
        sops.gram(V)
    with pytest.raises(ValueError):
        sops.project(V, torch.ones((300, 3), dtype=torch.float64))
    with pytest.raises(ValueError):                    # an output column past the view's last
        sops.gram(A.view(col_map=np.arange(600, dtype=np.int32), n_out=10))


@pytest.mark.parametrize("vd", ["float32", "float64"])
@pytest.mark.parametrize("i", [0, 1])
def test_pca_csr_matches_pca_tensor(i, vd):
    pc.check_pca_csr(i, vd, DEV)


def test_pca_csr_clamps_n_comps():
    case = pc.n_case(5)                                # 5 x 130: at most 4 components
    got = pp.pca_csr(case.csr(DEV), n_comps=50)
    ref = pp.pca_tensor(torch.from_numpy(case.DC[0].copy()), 50)
    assert got[0].shape == ref[0].shape == (5, 4) and got[1].shape == ref[1].shape == (4, 130)


def _adata(n=300, g=90, seed=7):
    X = pc.pca_counts(n, g, 4, seed, 0.12).copy()
    rs = np.random.default_rng(seed)
    var = pd.DataFrame({"highly_variable": rs.random(g) < 0.6}, index=[f"g{j}" for j in range(g)])
    return AnnData(X=X, obs=pd.DataFrame(index=[f"c{i}" for i in range(n)]), var=var)


@pytest.mark.parametrize("hv", [False, True], ids=["all", "hvg"])
def test_pp_pca_csr_backend_matches_dense(hv, monkeypatch):
    d = pp.pca(_adata(), n_comps=8, use_highly_variable=hv, backend="dense")
    # the CSR backend never densifies X
    monkeypatch.setattr(sp.csr_matrix, "toarray", lambda *a, **k: pytest.fail("densified"))
    c = pp.pca(_adata(), n_comps=8, use_highly_variable=hv, backend="csr")
    monkeypatch.undo()
    pc.assert_pca_close((c.obsm["X_pca"], c.varm["PCs"].T, c.uns["pca"]["variance"],
                         c.uns["pca"]["variance_ratio"]),
                        (d.obsm["X_pca"], d.varm["PCs"].T, d.uns["pca"]["variance"],
                         d.uns["pca"]["variance_ratio"]))
    if hv:
        assert not c.varm["PCs"][~c.var["highly_variable"].values].any()


def test_pp_pca_csr_backend_needs_sparse():
    ad = _adata()
    ad.X = ad.X.toarray()
    with pytest.raises(ValueError):
        pp.pca(ad, backend="csr")
    with pytest.raises(ValueError):
        pp.pca(_adata(), backend="sparse")


def test_bad_pca_backend_raises():
    p = Preprocess(random_seed=0)
    with pytest.raises(ValueError):
        p.normalize_batchcorrect(_adata(), n_top_genes=20, makeplots=False, pca_backend="sparse")
    with pytest.raises(ValueError):
        p.preprocess_for_cnmf(_adata(), n_top_rna_genes=20, makeplots=False, pca_backend=None)


def test_normalize_batchcorrect_csr_backend_matches_dense():
    Xc, cells, genes = simulate_counts(600, 200, 4, seed=3, sparse=True)
    rs = np.random.default_rng(0)
    obs = pd.DataFrame({"batch": pd.Categorical(rs.choice(["x", "y", "z"], 600))}, index=cells)
    ad = AnnData(X=sp.csr_matrix(Xc, dtype=np.float32), obs=obs, var=pd.DataFrame(index=genes))
    p = Preprocess(random_seed=0)
    kw = dict(harmony_vars=["batch"], n_top_genes=60, makeplots=False, max_iter_harmony=3,
              device="cpu")
    d_out, d_hv = p.normalize_batchcorrect(ad.copy(), **kw)
    c_out, c_hv = p.normalize_batchcorrect(ad.copy(), pca_backend="csr", **kw)
    assert c_hv == d_hv
    # the tolerance of the device-vs-host pipeline test, all 50 components
    np.testing.assert_allclose(c_out.obsm["X_pca"], d_out.obsm["X_pca"], rtol=1e-4, atol=1e-4)
    assert c_out.X.shape == d_out.X.shape == (600, 60)
    assert np.isfinite(c_out.X).all() and (c_out.X >= 0).all()
