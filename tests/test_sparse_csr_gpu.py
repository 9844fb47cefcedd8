"""csr storage of the data matrix on the GPU: the device CSR -> transposed tiles builder
(csr_transpose.hip) against the dense-slice builder and the CPU twin, the KL solver on
models.nmf.SparseCSRX against the dense-storage sparse route, its memory, and the public
x_storage='csr' route."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from cnmf_torch_amd import api, ops
from cnmf_torch_amd.api import cNMF
from cnmf_torch_amd.models.nmf import NMFBatchSolver, NMFOptions, SparseCSRX
from cnmf_torch_amd.utils.io import load_df_from_npz, load_yaml, save_df_to_npz
from cnmf_torch_amd.utils.synthetic import normalized_counts_matrix, simulate_counts

gpu = pytest.mark.gpu
KL = dict(beta_loss="kullback-leibler")


def _counts(N, G, density, seed):
    """Integer counts 1..9 at ``density``: every float64 sum of them is exact in any order."""
    rng = np.random.default_rng(seed)
    X = rng.integers(1, 10, size=(N, G)).astype(np.float32)
    X[rng.random((N, G)) >= density] = 0.0
    return X


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _tiles_equal(got, ref_tiles):
    """``got`` (tiles of one shared allocation, absolute row pointers) against a list of
    (t0, rowptr from 0, col, val), bit for bit."""
    assert [t0 for t0, _ in got] == [r[0] for r in ref_tiles]
    for (_, c), (_, rp, col, val) in zip(got, ref_tiles):
        assert c.rowptr.dtype == torch.int32 and c.col.dtype == torch.int32
        assert c.val.dtype == torch.float32 and c.col.numel() >= 1 and c.val.numel() >= 1
        lo, hi = int(c.rowptr[0]), int(c.rowptr[-1])
        np.testing.assert_array_equal((c.rowptr - lo).cpu().numpy(), rp.cpu().numpy())
        np.testing.assert_array_equal(c.col[lo:hi].cpu().numpy(), col.cpu().numpy())
        np.testing.assert_array_equal(_bits(c.val[lo:hi]), _bits(val))


def _builder_case(name):
    if name == "longest_segment":           # tl = 8192: one 8192-entry segment + an 8-row tail
        X = _counts(8200, 3, 0.3, 0)
        X[:, 0] = 1.0 + np.arange(8200) % 7
        return X, 0, 8200, 1, [8192, 8]
    if name == "three_tiles":               # tl = 256: tiles of 256 / 256 / 88
        return _counts(600, 333, 0.10, 1), 0, 600, 128, [256, 256, 88]
    if name == "row_range_wide_scan":       # a rowptr base > 0, G beyond one workgroup's scan
        return _counts(700, 2500, 0.05, 2), 300, 600, 10, [300]
    if name == "empty_middle_tile":
        X = _counts(600, 50, 0.2, 3)
        X[256:512] = 0.0
        return X, 0, 600, 128, [256, 256, 88]
    X = np.zeros((300, 40), dtype=np.float32)                              # all_zero
    return X, 0, 300, 128, [256, 44]


@gpu
@pytest.mark.parametrize("name", ["longest_segment", "three_tiles", "row_range_wide_scan",
                                  "empty_middle_tile", "all_zero"])
def test_tiles_from_csr_equal_the_dense_builder_bitwise(name):
    X, a, b, K, heights = _builder_case(name)
    Xg = torch.from_numpy(X).cuda()
    G = X.shape[1]
    tl = ops.kl_tile_rows(K)
    csr = ops.kl_csr(Xg)
    got = ops.kl_csr_tiles_from_csr(ops.kl_csr_rows(csr, a, b), K)
    assert [c.n_cols for _, c in got] == heights and all(c.n_rows == G for _, c in got)
    if name == "row_range_wide_scan":
        assert int(csr.rowptr[a]) > 0
    if name == "empty_middle_tile":
        assert int(got[1][1].rowptr[-1]) == int(got[1][1].rowptr[0])
    # the parent's builder on the dense slice
    parent = ops.kl_csr_tiles(Xg[a:b], K)
    _tiles_equal(got, [(t0, c.rowptr, c.col, c.val) for t0, c in parent])
    # the CPU twin
    _tiles_equal(got, ops.reference.csr_transpose_tiles(csr.rowptr.cpu(), csr.col.cpu(),
                                                        csr.val.cpu(), a, b, G, tl))
    # a second build: the same bits in the whole allocation
    again = ops.kl_csr_tiles_from_csr(ops.kl_csr_rows(csr, a, b), K)
    for (_, c), (_, d) in zip(got, again):
        np.testing.assert_array_equal(c.rowptr.cpu().numpy(), d.rowptr.cpu().numpy())
    np.testing.assert_array_equal(got[0][1].col.cpu().numpy(), again[0][1].col.cpu().numpy())
    np.testing.assert_array_equal(_bits(got[0][1].val), _bits(again[0][1].val))


def _same_result(a, b):
    np.testing.assert_array_equal(_bits(a.W), _bits(b.W))
    np.testing.assert_array_equal(_bits(a.HT), _bits(b.HT))
    np.testing.assert_array_equal(np.asarray(a.err).view(np.int64),
                                  np.asarray(b.err).view(np.int64))
    np.testing.assert_array_equal(a.n_iter, b.n_iter)


@gpu
@pytest.mark.parametrize("K,mode", [(5, "online"), (40, "online"), (72, "online"),
                                    (5, "batch")])
def test_solver_on_the_holder_equals_dense_storage_bitwise(monkeypatch, K, mode):
    """The two routes hand identical arrays to identical kernels (one rank per slice count
    of sparse_kl.hip: 1, 4 and 8 component slices)."""
    monkeypatch.setenv("CNMF_KL_SPARSE", "1")
    X = _counts(700, 150, 0.10, 5)
    if mode == "online":
        opts = NMFOptions(n_components=K, online_chunk_size=300, online_max_pass=3, **KL)
    else:
        opts = NMFOptions(n_components=K, mode="batch", batch_max_iter=20, **KL)
    dense = NMFBatchSolver(torch.from_numpy(X).cuda(), opts)
    ref = dense.run([1, 2, 3])
    assert dense._kl_sparse() is not None
    h = SparseCSRX.from_scipy(sp.csr_matrix(X), device="cuda")
    monkeypatch.setenv("CNMF_KL_SPARSE", "0")      # does not apply to the only copy of X
    s = NMFBatchSolver(h, opts)
    got = s.run([1, 2, 3])
    assert s._kl_sparse() is h.csr and torch.isnan(s.X[0, 0])
    assert np.all(np.isfinite(got.err)) and np.all(got.err > 0)
    _same_result(got, ref)


@gpu
def test_normalised_data_matches_dense_storage(monkeypatch):
    """Non-integer data: the mean and the chunk sums are float64 sums in another order, so
    the routes are compared at the bounds the project uses between KL routes
    (test_online_kl_xwide_sparse_path_matches_dense): err rtol 2e-3, pass counts within 2."""
    monkeypatch.setenv("CNMF_KL_SPARSE", "1")
    X = normalized_counts_matrix(1500, 300, n_programs=8, seed=3)
    X[X < np.quantile(X, 0.85)] = 0.0
    opts = NMFOptions(n_components=10, online_chunk_size=500, online_max_pass=6, **KL)
    ref = NMFBatchSolver(torch.from_numpy(X).cuda(), opts).run([1, 2, 3])
    h = SparseCSRX.from_scipy(X, device="cuda")
    got = NMFBatchSolver(h, opts).run([1, 2, 3])
    print("err csr", got.err, "dense storage", ref.err, "rel",
          np.abs(got.err - ref.err) / ref.err, "passes", got.n_iter, ref.n_iter)
    np.testing.assert_allclose(got.err, ref.err, rtol=2e-3)
    assert np.abs(got.n_iter - ref.n_iter).max() <= 2, (got.n_iter, ref.n_iter)


def _no_dense(_):
    raise AssertionError("x_storage='csr' densified the matrix")


@gpu
def test_no_dense_copy_on_the_device(monkeypatch):
    N, G = 20000, 2000
    rng = np.random.default_rng(0)
    m = sp.random(N, G, 0.02, format="csr", dtype=np.float32, random_state=rng,
                  data_rvs=lambda n: rng.integers(1, 10, n).astype(np.float32))
    monkeypatch.setattr(api, "_dense32", _no_dense)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    h = SparseCSRX.from_scipy(m, device="cuda")
    assert h.nbytes == 8 * m.nnz + 4 * (N + 1)
    opts = NMFOptions(n_components=5, online_chunk_size=5000, online_max_pass=1, **KL)
    res = NMFBatchSolver(h, opts).run([1, 2])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak device bytes", peak, "holder", h.nbytes, "dense X", N * G * 4)
    assert np.all(np.isfinite(res.err))
    assert peak < N * G * 4 // 2, peak


def _prepared(tmp_path, name, **kw):
    Xc, cells, genes = simulate_counts(220, 120, 3, seed=4, sparse=False)
    fn = str(tmp_path / "c.df.npz")
    if not os.path.exists(fn):
        save_df_to_npz(pd.DataFrame(Xc, index=cells, columns=genes), fn)
    obj = cNMF(output_dir=str(tmp_path), name=name)
    obj.prepare(fn, components=[3, 4], n_iter=3, seed=1, num_highvar_genes=70, **kw)
    return obj


def _replicate_files(obj):
    return [obj.paths["iter_spectra"] % (k, it) for k in (3, 4) for it in range(3)]


@gpu
def test_factorize_csr_without_a_dense_copy(tmp_path, monkeypatch):
    from cnmf_torch_amd.utils.h5ad import read_h5ad

    obj, obj2 = _prepared(tmp_path, "csr", **KL), _prepared(tmp_path, "env", **KL)
    obj3 = _prepared(tmp_path, "fro")
    monkeypatch.setattr(api, "_dense32", _no_dense)      # (prepare itself may densify)
    obj.factorize(verbose=False, x_storage="csr")
    files = _replicate_files(obj)
    assert all(os.path.exists(f) for f in files)
    # bitwise the direct solver run on the holder, same seeds
    rp = load_df_from_npz(obj.paths["nmf_replicate_parameters"])
    rp = rp.sort_values(["n_components", "iter"], kind="stable")
    kwargs = load_yaml(obj.paths["nmf_run_parameters"])
    h = SparseCSRX.from_scipy(read_h5ad(obj.paths["normalized_counts"]).X, device="cuda")
    res = NMFBatchSolver(h, obj._solver_options(kwargs, 3)).run(
        [int(s) for s in rp["nmf_seed"]], ks=[int(k) for k in rp["n_components"]])
    for r, (k, it) in enumerate(zip(rp["n_components"], rp["iter"])):
        got = load_df_from_npz(obj.paths["iter_spectra"] % (int(k), int(it))).values
        np.testing.assert_array_equal(got, res.spectra(r).cpu().numpy())

    # the environment variable alone selects the route
    monkeypatch.setenv("CNMF_X_STORAGE", "csr")
    obj2.factorize(verbose=False)
    for f, f2 in zip(files, _replicate_files(obj2)):
        np.testing.assert_array_equal(load_df_from_npz(f).values, load_df_from_npz(f2).values)
    monkeypatch.delenv("CNMF_X_STORAGE")
    obj.combine()
    assert all(os.path.exists(obj.paths["merged_spectra"] % k) for k in (3, 4))

    # a Frobenius-prepared run raises before any replicate file is written
    with pytest.raises(ValueError, match="SparseCSRX.*x_storage='csr'.*beta_loss="):
        obj3.factorize(verbose=False, x_storage="csr")
    assert not any(os.path.exists(f) for f in _replicate_files(obj3))
