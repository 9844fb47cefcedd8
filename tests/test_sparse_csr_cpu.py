"""csr storage of the data matrix (models.nmf.SparseCSRX) on the CPU: the transposed-tile
oracle against scipy, the holder's format and validation, and what the solver and the
public x_storage route reject."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.api import cNMF
from cnmf_torch_amd.models import nmf_base
from cnmf_torch_amd.models.nmf import NMFBatchSolver, NMFOptions, SparseCSRX
from cnmf_torch_amd.utils.io import save_df_to_npz
from cnmf_torch_amd.utils.synthetic import simulate_counts

KL = dict(beta_loss="kullback-leibler")


def _counts(N, G, density, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(1, 10, size=(N, G)).astype(np.float32)
    X[rng.random((N, G)) >= density] = 0.0
    return X


def _check_tiles(X, a, b, tl):
    m = sp.csr_matrix(X)
    m.sort_indices()
    G = X.shape[1]
    tiles = ops.reference.csr_transpose_tiles(m.indptr, m.indices, m.data, a, b, G, tl)
    assert [t0 for t0, *_ in tiles] == list(range(0, b - a, tl))
    for t0, rp, col, val in tiles:
        t1 = min(b - a, t0 + tl)
        ref = m[a + t0:a + t1].T.tocsr()
        ref.sort_indices()
        assert rp.dtype == torch.int32 and col.dtype == torch.int32 and val.dtype == torch.float32
        np.testing.assert_array_equal(rp.numpy(), ref.indptr)
        np.testing.assert_array_equal(col.numpy(), ref.indices)
        np.testing.assert_array_equal(val.numpy(), ref.data.astype(np.float32))


def test_reference_transpose_tiles_equal_scipy():
    _check_tiles(np.array([[3.0]], dtype=np.float32), 0, 1, 64)            # 1 x 1
    X = _counts(37, 5, 0.5, 0)
    X[4] = 0.0                 # an empty row
    X[:, 2] = 0.0              # an empty column
    X[16:24] = 0.0             # an all-zero tile (tl = 8: rows 16..23)
    _check_tiles(X, 0, 37, 8)                          # 8 does not divide 37
    _check_tiles(X, 5, 30, 8)                          # a > 0, 8 does not divide 25
    _check_tiles(X, 0, 37, 64)                         # one tile
    _check_tiles(np.zeros((9, 4), dtype=np.float32), 0, 9, 4)              # nnz == 0


def test_from_scipy_canonicalises_and_reports_its_bytes():
    X = _counts(40, 13, 0.3, 1)
    canon = sp.csr_matrix(X)
    canon.sort_indices()
    # the same matrix with duplicates (split values), unsorted indices and explicit zeros
    r, c = np.nonzero(X)
    v = X[r, c]
    zr, zc = np.nonzero(X == 0)
    rows = np.concatenate([r, r, zr[:20]])[::-1]
    cols = np.concatenate([c, c, zc[:20]])[::-1]
    vals = np.concatenate([v - 1.0, np.ones_like(v), np.zeros(20, dtype=np.float32)])[::-1]
    # (the raw CSR is built by hand so that nothing is canonicalised on the way)
    order = np.argsort(rows, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=40))])
    messy = sp.csr_matrix((vals[order], cols[order], indptr), shape=X.shape)
    assert messy.nnz > canon.nnz and not messy.has_sorted_indices
    for src in (messy, canon, X):
        h = SparseCSRX.from_scipy(src, rows=16)
        assert h.shape == (40, 13) and h.nnz == canon.nnz and h.dtype == torch.float32
        np.testing.assert_array_equal(h.csr.rowptr.numpy(), canon.indptr)
        np.testing.assert_array_equal(h.csr.col.numpy(), canon.indices)
        np.testing.assert_array_equal(h.csr.val.numpy(), canon.data)
        assert h.csr.rowptr.dtype == torch.int32 and h.csr.col.dtype == torch.int32
        np.testing.assert_array_equal(h.to_dense().numpy(), X)
        assert h.nbytes == 8 * canon.nnz + 4 * 41
        assert h.sum == float(X.sum(dtype=np.float64))
    assert messy.nnz > canon.nnz                       # the input was left as it came
    z = SparseCSRX.from_scipy(sp.csr_matrix((7, 3), dtype=np.float32))
    assert z.nnz == 0 and z.nbytes == 8 + 4 * 8 and z.csr.col.numel() == 1
    assert not z.to_dense().any()


def test_validation_raises_before_anything_else(monkeypatch):
    X = _counts(20, 6, 0.5, 2)
    m = sp.csr_matrix(X)

    def broken(**kw):
        parts = dict(data=m.data.copy(), indices=m.indices.copy(), indptr=m.indptr.copy())
        for k, f in kw.items():
            f(parts[k])
        out = sp.csr_matrix(X)
        out.data, out.indices, out.indptr = parts["data"], parts["indices"], parts["indptr"]
        return out

    def setv(i, v):
        def f(a):
            a[i] = v
        return f

    cases = [(broken(indptr=setv(3, int(m.indptr[2]) - 1)), "rowptr"),        # not monotone
             (broken(indptr=setv(0, 1)), "rowptr"),                           # not from 0
             (broken(indptr=setv(-1, m.nnz - 1)), "rowptr"),                  # not to nnz
             (broken(indices=setv(5, 6)), "column index"),                    # col == G
             (broken(indices=setv(5, -1)), "column index"),
             (broken(data=setv(2, -1.0)), "negative or non-finite"),
             (broken(data=setv(2, np.nan)), "negative or non-finite"),
             (broken(data=setv(2, np.inf)), "negative or non-finite")]
    for bad, what in cases:
        with pytest.raises(ValueError, match=f"SparseCSRX.*{what}"):
            SparseCSRX.from_scipy(bad)
    Xn = X.copy()
    Xn[3, 3] = -2.0
    with pytest.raises(ValueError, match="SparseCSRX.*negative or non-finite"):
        SparseCSRX.from_scipy(Xn)
    # the entry count must stay below the int32 limit (lowered here)
    monkeypatch.setattr(nmf_base, "CSR_MAX_NNZ", m.nnz)
    with pytest.raises(ValueError, match="SparseCSRX.*int32"):
        SparseCSRX.from_scipy(m)
    monkeypatch.setattr(nmf_base, "CSR_MAX_NNZ", m.nnz + 1)
    assert SparseCSRX.from_scipy(m).nnz == m.nnz


class _TwoRanks:
    is_distributed = True
    world_size, rank = 2, 0


def test_solver_restrictions_name_the_holder_and_the_option():
    h = SparseCSRX.from_scipy(sp.csr_matrix(_counts(60, 20, 0.3, 3)))
    for kw, what in ((dict(beta_loss="frobenius"), "beta_loss"),
                     (dict(beta_loss="itakura-saito"), "beta_loss"),
                     (dict(beta_loss="frobenius", algo="hals"), "algo"),
                     (dict(beta_loss="frobenius", algo="bpp"), "algo"),
                     (dict(KL, algo="hals"), "algo"),
                     (dict(KL, init="nndsvd"), "init"),
                     (dict(KL, fp_precision="double"), "dtype"),
                     (dict(KL), "device"),                    # a holder on the CPU
                     (dict(KL, mode="batch"), "device")):
        with pytest.raises(ValueError, match=f"SparseCSRX supports.*{what}="):
            NMFBatchSolver(h, NMFOptions(n_components=4, **kw))
    with pytest.raises(ValueError, match="SparseCSRX.*cell-sharded.*row_map"):
        NMFBatchSolver(h, NMFOptions(n_components=4, **KL), row_map=[(0, 60, 0)])
    with pytest.raises(ValueError, match="SparseCSRX.*cell-sharded.*comm"):
        NMFBatchSolver(h, NMFOptions(n_components=4, **KL), comm=_TwoRanks())


def test_rank_above_128_raises_from_run_before_any_launch(monkeypatch):
    # the constructor's device check is what a CPU machine reaches first; with it
    # satisfied by hand, run() must refuse K > 128 before it touches the device
    h = SparseCSRX.from_scipy(sp.csr_matrix(_counts(60, 20, 0.3, 3)))
    s = NMFBatchSolver.__new__(NMFBatchSolver)
    s.opts, s._csr_src = NMFOptions(n_components=4, **KL), h
    with pytest.raises(ValueError, match="SparseCSRX supports K <= 128.*K=129"):
        s.run([1, 2], ks=[129, 129])


def _prepared(tmp_path, name, components=(3, 4), **kw):
    Xc, cells, genes = simulate_counts(220, 120, 3, seed=4, sparse=False)
    fn = str(tmp_path / "c.df.npz")
    if not os.path.exists(fn):
        save_df_to_npz(pd.DataFrame(Xc, index=cells, columns=genes), fn)
    obj = cNMF(output_dir=str(tmp_path), name=name)
    obj.prepare(fn, components=list(components), n_iter=3, seed=1, num_highvar_genes=70, **kw)
    return obj


def _no_replicate_files(obj, ks):
    return not any(os.path.exists(obj.paths["iter_spectra"] % (k, it))
                   for k in ks for it in range(3))


def test_public_route_restrictions(tmp_path, monkeypatch):
    kl = _prepared(tmp_path, "kl", **KL)
    with pytest.raises(ValueError, match="SparseCSRX.*x_storage='csr'.*device='cpu'"):
        kl.factorize(verbose=False, x_storage="csr", device="cpu")
    monkeypatch.setenv("CNMF_X_STORAGE", "csr")        # the variable alone selects the route
    with pytest.raises(ValueError, match="SparseCSRX.*x_storage='csr'.*device='cpu'"):
        kl.factorize(verbose=False, device="cpu")
    monkeypatch.delenv("CNMF_X_STORAGE")
    assert _no_replicate_files(kl, (3, 4))
    fro = _prepared(tmp_path, "fro")
    with pytest.raises(ValueError, match="SparseCSRX.*x_storage='csr'.*beta_loss='frobenius'"):
        fro.factorize(verbose=False, x_storage="csr", device="cpu")
    assert _no_replicate_files(fro, (3, 4))
    wide = _prepared(tmp_path, "wide", components=(3, 129), **KL)
    with pytest.raises(ValueError, match="SparseCSRX.*x_storage='csr'.*K=129"):
        wide.factorize(verbose=False, x_storage="csr", device="cpu")
    assert _no_replicate_files(wide, (3, 129))
    # the cell-sharded route is refused as on tile storage
    with pytest.raises(ValueError, match="SparseCSRX.*x_storage='csr'.*cell-sharded"):
        kl.factorize_jobs([0], x_storage="csr", device="cpu", row_range=(0, 100))
    with pytest.raises(ValueError, match="x_storage 'rows'"):
        kl.factorize(verbose=False, x_storage="rows", device="cpu")
