"""Sparse KL (CSR) kernels at 33 <= K <= 64 (sparse_kl.hip, 4 slices): numerics vs the float64
reference, the replicate gate, the solver on the CSR route against the dense route, and the
automatic routing above K = 32."""
import os
import warnings

import numpy as np
import pytest
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.ops import reference

pytestmark = pytest.mark.gpu

EPS = 1e-10
A, B = 100, 700          # the row chunk


def _problem(K, G):
    """The construction of test_kernels_gpu.py::test_sparse_kl_kernels_match_fp64: R = 3,
    N = 901, X ~15 % dense with row 7 empty, seed = K."""
    g = torch.Generator().manual_seed(K)
    R, N = 3, 901
    X = torch.rand((N, G), generator=g, dtype=torch.float64)
    X[X < 0.85] = 0.0
    X[7] = 0.0
    HT = torch.rand((R, K, N), generator=g, dtype=torch.float64) + 0.05
    W = torch.rand((R, K, G), generator=g, dtype=torch.float64) + 0.05
    return X, HT, W


# K not a multiple of 4 (33), both slice widths (K4 <= 48, K4 > 48), W^T staged in LDS
# (G <= 512 at K = 64) and gathered from L2, two spectra tiles at K = 64 (512-cell tiles,
# 600-cell chunk; 640-cell tiles at K = 48)
@pytest.mark.parametrize("K,G", [(33, 333), (40, 333), (48, 700), (64, 333), (64, 1200)])
def test_sparse_kl_wide_kernels_match_fp64(K, G):
    """Loss, spectra numerators and three 3-step usage blocks with the block-objective rule
    vs the float64 dense reference.  In the reference the block objective changes by
    0.97-0.99 after block 1 and 0.002-0.007 after block 2 at these five inputs (tol 0.05),
    so no stop decision is near its threshold."""
    X, HT, W = _problem(K, G)
    R = HT.shape[0]
    dev = torch.device("cuda")
    Xg, Hg, Wg = X.float().to(dev), HT.float().to(dev), W.float().to(dev)
    csr = ops.kl_csr(Xg)
    assert int(csr.rowptr[-1]) == int((X != 0).sum())
    assert bool(ops._hip.sk_lds(G, K)) == (G * 4 * ((K + 3) // 4 * 4) <= 128 * 1024)
    # loss
    ref_loss = reference.beta_contract(0, X, HT, W, 1.0, EPS, False, True)[2]
    torch.testing.assert_close(ops.kl_sparse_loss(csr, Hg, Wg, EPS).cpu(), ref_loss, rtol=1e-5,
                               atol=1e-6)
    # spectra numerators over a row chunk
    rn, _, _ = reference.beta_contract(1, X[A:B], HT[:, :, A:B], W, 1.0, EPS, True, False)
    tiles = ops.kl_csr_tiles(Xg[A:B], K)
    assert len(tiles) == -(-(B - A) // ops.kl_tile_rows(K)) and (K < 64 or len(tiles) == 2)
    num = ops.kl_sparse_w_num(tiles, Hg[:, :, A:B].contiguous(), Wg, EPS)
    torch.testing.assert_close(num.sum(0).cpu().double(), rn, rtol=2e-5, atol=1e-6)
    # forced 128-cell tiles == the default tiling
    t2 = [(t0, ops.kl_csr(Xg[A + t0:A + min(B - A, t0 + 128)].t()))
          for t0 in range(0, B - A, 128)]
    num2 = ops.kl_sparse_w_num(t2, Hg[:, :, A:B].contiguous(), Wg, EPS)
    torch.testing.assert_close(num2.sum(0), num.sum(0), rtol=1e-5, atol=1e-6)
    # usage blocks with the rule, on a row range of the CSR (rowptr slice)
    h1 = Hg[:, :, A:B].contiguous()
    h2 = HT[:, :, A:B].clone()
    act_g = torch.ones(R, dtype=torch.int32, device=dev)
    act_r = torch.ones(R, dtype=torch.int32)
    it_g = torch.zeros(R, dtype=torch.int32, device=dev)
    it_r = torch.zeros(R, dtype=torch.int32)
    hs_g = torch.zeros((R, 2), dtype=torch.float64, device=dev)
    hs_r = torch.zeros((R, 2), dtype=torch.float64)
    for blk in range(3):
        ops.kl_sparse_h_block(ops.kl_csr_rows(csr, A, B), h1, Wg, EPS, 3, 0.01, 0.0, act=act_g,
                              tol=0.05, iters=it_g, hstate=hs_g, loss_entry=blk == 0)
        reference.beta_h_block(X[A:B], h2, W, 1.0, EPS, 3, 0.01, 0.0, act=act_r, tol=0.05,
                               iters=it_r, hstate=hs_r, loss_entry=blk == 0)
    torch.testing.assert_close(h1.cpu().double(), h2, rtol=1e-4, atol=1e-6)
    assert act_g.cpu().tolist() == act_r.tolist()
    assert it_g.cpu().tolist() == it_r.tolist()
    torch.testing.assert_close(hs_g.cpu(), hs_r, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("K,G", [(40, 333), (64, 1200)])
def test_sparse_kl_wide_gate_leaves_inactive_replicate_untouched(K, G):
    """act = [1, 0, 1]: the inactive replicate's usages are bit-identical after a usage
    launch with the rule, its step count and block-objective state too; the active ones
    moved."""
    X, HT, W = _problem(K, G)
    dev = torch.device("cuda")
    Xg, Hg, Wg = X.float().to(dev), HT.float().to(dev), W.float().to(dev)
    csr = ops.kl_csr(Xg)
    h = Hg[:, :, A:B].contiguous()
    h0 = h.clone()
    act = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    it = torch.zeros(3, dtype=torch.int32, device=dev)
    hs = torch.zeros((3, 2), dtype=torch.float64, device=dev)
    ops.kl_sparse_h_block(ops.kl_csr_rows(csr, A, B), h, Wg, EPS, 3, 0.01, 0.0, act=act,
                          tol=0.05, iters=it, hstate=hs, loss_entry=True)
    assert torch.equal(h[1], h0[1])
    assert not torch.equal(h[0], h0[0]) and not torch.equal(h[2], h0[2])
    assert it.cpu().tolist() == [3, 0, 3]
    assert hs[1].cpu().tolist() == [0.0, 0.0]


def _sparse_counts(n, g, density, seed):
    from cnmf_torch_amd.utils.synthetic import normalized_counts_matrix

    X = normalized_counts_matrix(n, g, n_programs=8, seed=seed)
    X[X < np.quantile(X, 1.0 - density)] = 0.0
    return X


def test_online_kl_wide_sparse_path_matches_dense():
    """Online KL at K = 40 on a ~15 %-dense matrix: the CSR kernels (CNMF_KL_SPARSE=1) and
    the dense split-precision kernels (=0) give the same factorisation, natively."""
    from cnmf_torch_amd.models.nmf import NMFBatchSolver, NMFOptions

    Xg = torch.from_numpy(_sparse_counts(1500, 300, 0.15, seed=3)).cuda()
    opts = NMFOptions(n_components=40, beta_loss="kullback-leibler", online_chunk_size=500,
                      online_max_pass=6)
    res = {}
    old = os.environ.get("CNMF_KL_SPARSE")
    try:
        for flag in ("1", "0"):
            os.environ["CNMF_KL_SPARSE"] = flag
            s = NMFBatchSolver(Xg, opts)
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)
                res[flag] = s.run([1, 2, 3])
            assert (s._kl_sparse() is not None) == (flag == "1")
    finally:
        if old is None:
            os.environ.pop("CNMF_KL_SPARSE", None)
        else:
            os.environ["CNMF_KL_SPARSE"] = old
    a, b = res["1"], res["0"]
    print("err sparse", a.err, "dense", b.err, "passes", a.n_iter, b.n_iter)
    np.testing.assert_allclose(a.err, b.err, rtol=2e-3)
    assert np.abs(a.n_iter - b.n_iter).max() <= 2, (a.n_iter, b.n_iter)


@pytest.mark.parametrize("density,sparse", [(0.05, True), (0.08, True), (0.13, False),
                                            (0.17, False)])
def test_kl_wide_routing_follows_measured_crossover(monkeypatch, density, sparse):
    """Without CNMF_KL_SPARSE, KL at K = 40 takes the CSR kernels up to
    kl_sparse_density_wide (0.10: below the measured crossovers, ~14 % at K = 48 and ~10.7 %
    at K = 64, profiles/p2_kl_wide_ab.txt) and the dense kernels above it -- also at 17 %, where
    K <= 32 still takes the CSR kernels."""
    from cnmf_torch_amd.models.nmf import NMFBatchSolver, NMFOptions

    monkeypatch.delenv("CNMF_KL_SPARSE", raising=False)
    X = _sparse_counts(2000, 300, density, seed=1)
    assert abs(float((X != 0).mean()) - density) < 0.005
    Xg = torch.from_numpy(X).cuda()
    assert NMFOptions(n_components=40).kl_sparse_density_wide == 0.10
    s = NMFBatchSolver(Xg, NMFOptions(n_components=40, beta_loss="kullback-leibler"))
    assert (s._kl_sparse() is not None) == sparse
    s = NMFBatchSolver(Xg, NMFOptions(n_components=24, beta_loss="kullback-leibler"))
    assert s._kl_sparse() is not None            # K <= 32: kl_sparse_density (0.18) as before
