"""Tile storage of the data matrix (models.nmf.SparseTilesX, ops.gemm_tiles) on the CPU:
the format, the solver on the holder, and the public x_storage route."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from cnmf_torch_amd import api, ops
from cnmf_torch_amd.api import cNMF
from cnmf_torch_amd.models.nmf import (NMFBatchSolver, NMFOptions, RowBlocks, SparseTilesX,
                                       _XPlanes)
from cnmf_torch_amd.utils.io import load_df_from_npz, save_df_to_npz
from cnmf_torch_amd.utils.synthetic import simulate_counts

from sparse_tiles_inputs import count_matrix, float_matrix


def _three_inputs(N, G):
    return [("count1", count_matrix(N, G)[0], 1),
            ("count2", count_matrix(N, G, two_planes=True)[0], 2),
            ("float", float_matrix(N, G), _XPlanes._float_planes(G))]


def test_round_trip_planes_statistics_and_bytes():
    N, G = 250, 150
    for name, X, pb in _three_inputs(N, G):
        csr = sp.csr_matrix(X)
        h = SparseTilesX.from_scipy(csr, rows=128)      # two row blocks
        assert h.shape == (N, G) and h.pb == pb, name
        assert (h.unit is None) == (name == "float"), name
        assert h.Gp == 192 and h.nnz == csr.nnz
        D = h.to_dense().numpy()
        if h.unit is None:
            np.testing.assert_array_equal(D, csr.toarray())      # three planes: exact
        else:
            # C * unit reproduces X to the bound _count_units accepts (4e-7 relative)
            np.testing.assert_array_equal(D != 0, csr.toarray() != 0)
            np.testing.assert_allclose(D, csr.toarray(), rtol=1e-6, atol=0)
        X64 = csr.toarray().astype(np.float64)
        np.testing.assert_allclose(h.x_sq, (X64 ** 2).sum(), rtol=1e-12)
        np.testing.assert_allclose(h.sum, X64.sum(), rtol=1e-12)
        tiles = -(-N // 64) * -(-G // 64)
        assert h.tiles.ptr.dtype == torch.int64 and h.tiles.ptr.numel() == tiles + 1
        assert h.nbytes <= 4 * csr.nnz + 8 * (tiles + 1) + 4 * G + 4096 + 2 * csr.nnz * (pb - 1)
    # a dense numpy matrix tiles the same way as its CSR
    a = SparseTilesX.from_scipy(X).tiles
    b = SparseTilesX.from_scipy(sp.csr_matrix(X)).tiles
    assert torch.equal(a.ent, b.ent) and torch.equal(a.ptr, b.ptr)
    # block starts must sit on the tile height
    Xt = torch.from_numpy(X)
    with pytest.raises(ValueError, match="multiple of 64"):
        SparseTilesX(RowBlocks(N, G, lambda: ((a_, Xt[a_:a_ + 100]) for a_ in range(0, N, 100)),
                               "cpu"))


def test_empty_matrix_and_malformed_structure():
    h = SparseTilesX.from_scipy(sp.csr_matrix((70, 30), dtype=np.float32))
    assert h.nnz == 0 and h.tiles.ent.numel() == 1 and float(h.to_dense().abs().sum()) == 0.0
    h = SparseTilesX.from_scipy(sp.csr_matrix(count_matrix(100, 70)[0]))
    t = h.tiles
    last = t.ent.clone()
    last[-1] |= 63 << 22            # a cell beyond row 99 in the last row tile
    h.tiles = t._replace(ent=last)
    with pytest.raises(RuntimeError, match="consistency"):
        h._validate()
    ptr = t.ptr.clone()
    ptr[1] = ptr[-1] + 1
    h.tiles = t._replace(ptr=ptr)
    with pytest.raises(RuntimeError, match="consistency"):
        h._validate()


def test_gemm_tiles_reference_matches_dense_planes():
    """The CPU route of ops.gemm_tiles (reference.gemm_tiles) against ops.gemm_planes on
    planes built from to_dense(): same product, both sides, an unaligned row range."""
    N, G, M = 250, 150, 37
    g = torch.Generator().manual_seed(0)
    for name, X, pb in _three_inputs(N, G):
        h = SparseTilesX.from_scipy(sp.csr_matrix(X))
        xp = _XPlanes(torch.from_numpy(X))
        assert xp.pb == h.pb
        for r0, r1 in ((0, N), (104, 208)):
            W = torch.rand((M, G), generator=g)
            wpl = torch.zeros((3, M, h.Gp), dtype=torch.int16)
            ops.split_planes(W, wpl, col_mul=h.unit)
            got = torch.empty((M, r1 - r0))
            ops.gemm_tiles(got, wpl, h.tiles, "n", r0, r1, M)
            ref = torch.empty((M, r1 - r0))
            ops.gemm_planes(ref, wpl, xp.x[:, r0:], M, r1 - r0, h.Gp)
            np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-6, atol=1e-6)
            kd = -(-(r1 - r0) // 64) * 64
            HT = torch.rand((M, r1 - r0), generator=g)
            hpl = torch.zeros((3, M, kd), dtype=torch.int16)
            ops.split_planes(HT, hpl)
            got = torch.ones((M, G))
            ops.gemm_tiles(got, hpl, h.tiles, "s", r0, r1, M, accumulate=True, col_scale=h.unit)
            ref = torch.ones((M, G))
            ops.gemm_planes(ref, hpl, xp.xt[:, :, r0:], M, G, kd, accumulate=True,
                            col_scale=h.unit)
            np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("algo", ["mu", "hals"])
def test_solver_on_tiles_factorises_like_the_resident_matrix(algo):
    """Same pass counts and errors to fp32 rounding as the resident matrix -- the
    tolerances of test_planes_only_x_factorises_like_the_resident_matrix."""
    X, _ = count_matrix(1200, 300)
    h = SparseTilesX.from_scipy(sp.csr_matrix(X), rows=512)
    assert h.unit is not None and h.pb == 1
    opts = NMFOptions(n_components=5, algo=algo, online_chunk_size=400, online_max_pass=30)
    seeds, ks = [5, 6, 7, 8, 9, 10], [5, 6, 7, 9, 5, 7]
    ref = NMFBatchSolver(torch.from_numpy(X), opts).run(seeds, ks=ks)
    got = NMFBatchSolver(h, opts).run(seeds, ks=ks)
    np.testing.assert_array_equal(got.n_iter, ref.n_iter)
    np.testing.assert_allclose(got.err, ref.err, rtol=1e-5)


def test_solver_restrictions_name_the_holder():
    h = SparseTilesX.from_scipy(sp.csr_matrix(count_matrix(250, 150)[0]))
    for kw, what in ((dict(mode="batch"), "mode"),
                     (dict(beta_loss="kullback-leibler"), "beta_loss"),
                     (dict(init="nndsvd"), "init")):
        with pytest.raises(ValueError, match=f"SparseTilesX supports.*{what}="):
            NMFBatchSolver(h, NMFOptions(n_components=4, **kw))
    # a chunk start off the planes' 8-alignment raises, as for PlanesOnlyX
    with pytest.raises(ValueError, match="SparseTilesX.*multiples of 8"):
        NMFBatchSolver(h, NMFOptions(n_components=3, online_chunk_size=100,
                                     online_max_pass=2)).run([1])


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


def test_factorize_tiles_without_a_dense_copy(tmp_path, monkeypatch):
    def no_dense(_):
        raise AssertionError("x_storage='tiles' densified the matrix")

    obj = _prepared(tmp_path, "tiles")
    monkeypatch.setattr(api, "_dense32", no_dense)
    obj.factorize(verbose=False, x_storage="tiles", device="cpu")
    files = _replicate_files(obj)
    assert all(os.path.exists(f) for f in files)
    # bitwise the direct solver run on the holder, same seeds
    from cnmf_torch_amd.utils.h5ad import read_h5ad
    from cnmf_torch_amd.utils.io import load_yaml

    rp = load_df_from_npz(obj.paths["nmf_replicate_parameters"])
    rp = rp.sort_values(["n_components", "iter"], kind="stable")
    kwargs = load_yaml(obj.paths["nmf_run_parameters"])
    h = SparseTilesX.from_scipy(read_h5ad(obj.paths["normalized_counts"]).X)
    res = NMFBatchSolver(h, obj._solver_options(kwargs, 3)).run(
        [int(s) for s in rp["nmf_seed"]], ks=[int(k) for k in rp["n_components"]])
    for r, (k, it) in enumerate(zip(rp["n_components"], rp["iter"])):
        got = load_df_from_npz(obj.paths["iter_spectra"] % (int(k), int(it))).values
        np.testing.assert_array_equal(got, res.spectra(r).numpy())

    # the environment variable alone selects the route
    obj2 = _prepared(tmp_path, "env")
    monkeypatch.setenv("CNMF_X_STORAGE", "tiles")
    obj2.factorize(verbose=False, device="cpu")
    for f, f2 in zip(files, _replicate_files(obj2)):
        np.testing.assert_array_equal(load_df_from_npz(f).values, load_df_from_npz(f2).values)
    monkeypatch.delenv("CNMF_X_STORAGE")

    # an option the holder does not support raises before any replicate file is written
    obj3 = _prepared(tmp_path, "kl", beta_loss="kullback-leibler")
    with pytest.raises(ValueError, match="SparseTilesX supports.*beta_loss="):
        obj3.factorize(verbose=False, x_storage="tiles", device="cpu")
    assert not any(os.path.exists(f) for f in _replicate_files(obj3))
    with pytest.raises(ValueError, match="x_storage"):
        obj3.factorize(verbose=False, x_storage="csr", device="cpu")
