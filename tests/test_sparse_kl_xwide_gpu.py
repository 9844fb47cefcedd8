"""Sparse KL (CSR) kernels at 65 <= K <= 128 (sparse_kl.hip, 8 slices): numerics vs the float64
reference, the penalties, the replicate gate, the solver on the CSR route against the dense
route (beta_any.hip), and the automatic routing above K = 64."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.ops import reference

gpu = pytest.mark.gpu

EPS = 1e-10
A, B = 100, 700          # the row chunk
H_TOL = dict(rtol=1e-4, atol=1e-6)       # usages, the bound at K <= 64


@functools.lru_cache(maxsize=None)
def _problem(K, G):
    """The construction of test_sparse_kl_wide_gpu.py: R = 3, N = 901, X ~15 % dense with
    row 7 empty, seed = K."""
    g = torch.Generator().manual_seed(K)
    R, N = 3, 901
    X = torch.rand((N, G), generator=g, dtype=torch.float64)
    X[X < 0.85] = 0.0
    X[7] = 0.0
    HT = torch.rand((R, K, N), generator=g, dtype=torch.float64) + 0.05
    W = torch.rand((R, K, G), generator=g, dtype=torch.float64) + 0.05
    return X, HT, W


@functools.lru_cache(maxsize=None)
def _ref_blocks(K, G, l1, l2):
    """float64: three 3-step usage blocks with the rule on the row chunk ->
    (usages, act, iters, hstate)."""
    X, HT, W = _problem(K, G)
    R = HT.shape[0]
    h = HT[:, :, A:B].clone()
    act = torch.ones(R, dtype=torch.int32)
    it = torch.zeros(R, dtype=torch.int32)
    hs = torch.zeros((R, 2), dtype=torch.float64)
    for blk in range(3):
        reference.beta_h_block(X[A:B], h, W, 1.0, EPS, 3, l1, l2, act=act, tol=0.05, iters=it,
                               hstate=hs, loss_entry=blk == 0)
    return h, act, it, hs


def _gpu_blocks(K, G, l1, l2):
    X, HT, W = _problem(K, G)
    R = HT.shape[0]
    dev = torch.device("cuda")
    Xg, Wg = X.float().to(dev), W.float().to(dev)
    csr = ops.kl_csr(Xg)
    h = HT.float().to(dev)[:, :, A:B].contiguous()
    act = torch.ones(R, dtype=torch.int32, device=dev)
    it = torch.zeros(R, dtype=torch.int32, device=dev)
    hs = torch.zeros((R, 2), dtype=torch.float64, device=dev)
    for blk in range(3):
        ops.kl_sparse_h_block(ops.kl_csr_rows(csr, A, B), h, Wg, EPS, 3, l1, l2, act=act,
                              tol=0.05, iters=it, hstate=hs, loss_entry=blk == 0)
    return h.cpu().double(), act.cpu(), it.cpu(), hs.cpu()


def _ratio(got, ref, rtol, atol):
    return float(((got - ref).abs() / (rtol * ref.abs() + atol)).max())


# K not a multiple of 4 (65), every 16-wide dispatch bucket (K4 68, 72 / 80 -> 5, 96 -> 6,
# 128 -> 8; 7 shares the instantiation of 8), W^T staged in LDS (G = 333; K = 128, G = 250:
# 128,000 B) and gathered from L2 (G = 700, 1200), two spectra tiles (448 / 448 / 384 / 320-cell tiles,
# 600-cell chunk) and three (256-cell tiles at K = 128)
CASES = [(65, 333), (72, 333), (80, 700), (96, 333), (128, 250), (128, 1200)]


@gpu
@pytest.mark.parametrize("K,G", CASES)
def test_sparse_kl_xwide_kernels_match_fp64(K, G):
    """Loss, spectra numerators and three 3-step usage blocks with the block-objective rule
    vs the float64 dense reference, at the bounds of the K <= 64 kernels.  In the reference
    the block objective changes by 0.986-0.993 after block 1 and 0.002-0.0094 after block 2
    at these six inputs (tol 0.05): every replicate stops after block 2, and no stop decision
    is near its threshold."""
    X, HT, W = _problem(K, G)
    dev = torch.device("cuda")
    Xg, Hg, Wg = X.float().to(dev), HT.float().to(dev), W.float().to(dev)
    csr = ops.kl_csr(Xg)
    assert int(csr.rowptr[-1]) == int((X != 0).sum())
    assert bool(ops._hip.sk_lds(G, K)) == (G * 4 * ((K + 3) // 4 * 4) <= 128 * 1024)
    assert bool(ops._hip.sk_lds(G, K)) == (G <= 333)
    # loss
    ref_loss = reference.beta_contract(0, X, HT, W, 1.0, EPS, False, True)[2]
    loss = ops.kl_sparse_loss(csr, Hg, Wg, EPS).cpu()
    print("loss: x tolerance", _ratio(loss, ref_loss, 1e-5, 1e-6))
    torch.testing.assert_close(loss, ref_loss, rtol=1e-5, atol=1e-6)
    # spectra numerators over a row chunk
    rn, _, _ = reference.beta_contract(1, X[A:B], HT[:, :, A:B], W, 1.0, EPS, True, False)
    tiles = ops.kl_csr_tiles(Xg[A:B], K)
    assert len(tiles) == -(-(B - A) // ops.kl_tile_rows(K))
    assert len(tiles) == (3 if K == 128 else 2)
    num = ops.kl_sparse_w_num(tiles, Hg[:, :, A:B].contiguous(), Wg, EPS)
    print("num: x tolerance", _ratio(num.sum(0).cpu().double(), rn, 2e-5, 1e-6))
    torch.testing.assert_close(num.sum(0).cpu().double(), rn, rtol=2e-5, atol=1e-6)
    # forced 128-cell tiles == the default tiling
    t2 = [(t0, ops.kl_csr(Xg[A + t0:A + min(B - A, t0 + 128)].t()))
          for t0 in range(0, B - A, 128)]
    num2 = ops.kl_sparse_w_num(t2, Hg[:, :, A:B].contiguous(), Wg, EPS)
    torch.testing.assert_close(num2.sum(0), num.sum(0), rtol=1e-5, atol=1e-6)
    # usage blocks with the rule, on a row range of the CSR (rowptr slice)
    h1, act_g, it_g, hs_g = _gpu_blocks(K, G, 0.01, 0.0)
    h2, act_r, it_r, hs_r = _ref_blocks(K, G, 0.01, 0.0)
    assert it_r.tolist() == [6, 6, 6] and act_r.tolist() == [0, 0, 0]
    print("usages: x tolerance", _ratio(h1, h2, **H_TOL),
          "hstate: x tolerance", _ratio(hs_g, hs_r, 1e-5, 1e-6))
    torch.testing.assert_close(h1, h2, **H_TOL)
    assert act_g.tolist() == act_r.tolist()
    assert it_g.tolist() == it_r.tolist()
    torch.testing.assert_close(hs_g, hs_r, rtol=1e-5, atol=1e-6)


PEN_CASE = (80, 700)
PENS = (0.02, 0.03)


@gpu
def test_sparse_kl_xwide_h_block_penalised_matches_fp64():
    """l1 = 0.02, l2 = 0.03 on the three usage blocks with the rule at (80, 700) vs the
    float64 reference, same bounds: usages, flags, step counts and objective state.  In the
    reference the stop decisions under these penalties are those of the unpenalised run
    (change 0.0034 after block 2); after these six steps the penalties are not yet visible
    in the usages, which is what the long block of the next test is for."""
    h1, act_g, it_g, hs_g = _gpu_blocks(*PEN_CASE, *PENS)
    h2, act_r, it_r, hs_r = _ref_blocks(*PEN_CASE, *PENS)
    print("usages: x tolerance", _ratio(h1, h2, **H_TOL))
    torch.testing.assert_close(h1, h2, **H_TOL)
    assert act_g.tolist() == act_r.tolist() and it_g.tolist() == it_r.tolist() == [6, 6, 6]
    torch.testing.assert_close(hs_g, hs_r, rtol=1e-5, atol=1e-6)


PEN_STEPS = 160


@functools.lru_cache(maxsize=None)
def _ref_long_block(l1, l2, reps):
    """float64: one PEN_STEPS-step usage block (no rule) on the row chunk of PEN_CASE, the
    first ``reps`` replicates."""
    X, HT, W = _problem(*PEN_CASE)
    h = HT[:reps, :, A:B].clone()
    reference.beta_h_block(X[A:B], h, W[:reps], 1.0, EPS, PEN_STEPS, l1, l2)
    return h


def _gpu_long_block(l1, l2):
    X, HT, W = _problem(*PEN_CASE)
    dev = torch.device("cuda")
    Xg, Wg = X.float().to(dev), W.float().to(dev)
    h = HT.float().to(dev)[:, :, A:B].contiguous()
    ops.kl_sparse_h_block(ops.kl_csr_rows(ops.kl_csr(Xg), A, B), h, Wg, EPS, PEN_STEPS, l1, l2)
    return h.cpu().double()


@gpu
def test_sparse_kl_xwide_h_block_penalties_are_visible_and_match_fp64():
    """l1 = 0.02, l2 = 0.03 at (80, 700) on one usage block long enough for them to show,
    vs the float64 reference at the same bounds (rtol 1e-4, atol 1e-6).

    The denominators sum_g W_kg are ~385 here, so one step moves a usage by ~5e-5 relative
    under these penalties, and the shift only builds up towards the penalised fixed point.
    In float64 (max |d| / (rtol |h| + atol), all three replicates) the usages with and
    without both penalties differ by 0.54 x the tolerance after 6 steps, 1.04 x after 20,
    1.44 x after 40, 1.82 x after 160; dropping l1 alone moves them by 0.37 / 0.76 / 1.06 /
    1.84 x, dropping l2 alone by 0.20 / 0.32 / 0.56 / 1.35 x.  160 steps is the first count
    tried (6, 10, 20, 30, 40, 60, 80, 120, 160) at which each term alone clears the
    tolerance by a quarter; the block runs without the rule so that all of them run.  The
    count is set by the reference alone, which asserts it here on replicate 0 (1.77 x without
    both, 1.67 x without l1, 1.35 x without l2).  A float32 run of the reference differs from
    the float64 one by 0.08 x the tolerance after the 160 steps (the kernel: 0.054 x; its
    usages with and without both penalties differ by 1.82 x)."""
    ref = _ref_long_block(*PENS, 3)
    for what, alt in (("both", (0.0, 0.0)), ("l1", (0.0, PENS[1])), ("l2", (PENS[0], 0.0))):
        shift = _ratio(_ref_long_block(*alt, 1), ref[:1], **H_TOL)
        print("float64, without", what, ": x tolerance", shift)
        assert shift > 1.0, (what, shift)
    h = _gpu_long_block(*PENS)
    print("usages: x tolerance", _ratio(h, ref, **H_TOL))
    torch.testing.assert_close(h, ref, **H_TOL)
    gpu_shift = _ratio(_gpu_long_block(0.0, 0.0), h, **H_TOL)
    print("GPU, without both: x tolerance", gpu_shift)
    assert gpu_shift > 1.0, gpu_shift


@gpu
@pytest.mark.parametrize("pens", [(20.0, 40.0), (20.0, 0.0), (0.0, 40.0)])
def test_sparse_kl_xwide_h_block_visible_penalties_match_fp64(pens):
    """The penalty sets of test_penalties_gpu.py at (80, 700): each non-zero term alone moves
    the float64 usages by >= 20 x the tolerance and no stop decision is within a factor 2 of
    tol (both asserted by sparse_kl_reference), and the kernel follows."""
    from test_penalties_cpu import sparse_kl_reference

    _, (hr, ar, ir, hsr), _ = sparse_kl_reference(*PEN_CASE, pens,
                                                  torch.ones(3, dtype=torch.int32))
    h, act, it, hs = _gpu_blocks(*PEN_CASE, *pens)
    print("usages: x tolerance", _ratio(h, hr, **H_TOL))
    torch.testing.assert_close(h, hr, **H_TOL)
    assert act.tolist() == ar.tolist() and it.tolist() == ir.tolist()
    torch.testing.assert_close(hs, hsr, rtol=1e-5, atol=1e-6)


@gpu
@pytest.mark.parametrize("K,G", [(72, 333), (128, 1200)])
def test_sparse_kl_xwide_gate_leaves_inactive_replicate_untouched(K, G):
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


@gpu
def test_online_kl_xwide_sparse_path_matches_dense():
    """Online KL at K = 72 on a ~15 %-dense matrix: the CSR kernels (CNMF_KL_SPARSE=1) and
    the dense rank-general route (=0, beta_any.hip) give the same factorisation, natively."""
    from cnmf_torch_amd.models.nmf import NMFBatchSolver, NMFOptions

    Xg = torch.from_numpy(_sparse_counts(1500, 300, 0.15, seed=3)).cuda()
    opts = NMFOptions(n_components=72, beta_loss="kullback-leibler", online_chunk_size=500,
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


@gpu
@pytest.mark.parametrize("density,sparse", [(0.08, True), (0.30, True), (0.40, False)])
def test_kl_xwide_routing_follows_measurement(monkeypatch, density, sparse):
    """Without CNMF_KL_SPARSE, KL at K = 72 takes the CSR kernels up to
    kl_sparse_density_xwide (0.35: the highest density measured, where they still beat the
    rank-general dense route at K = 80 and K = 128, profiles/p3_kl_xwide_ab.txt) and the dense
    route above it; K = 200 is beyond the CSR kernels even when they are forced."""
    from cnmf_torch_amd.models.nmf import NMFBatchSolver, NMFOptions

    monkeypatch.delenv("CNMF_KL_SPARSE", raising=False)
    X = _sparse_counts(2000, 300, density, seed=1)
    assert abs(float((X != 0).mean()) - density) < 0.005
    Xg = torch.from_numpy(X).cuda()
    cap = NMFOptions(n_components=72).kl_sparse_density_xwide
    assert cap == 0.35
    assert density <= cap - 0.03 if sparse else density >= cap + 0.03
    s = NMFBatchSolver(Xg, NMFOptions(n_components=72, beta_loss="kullback-leibler"))
    assert (s._kl_sparse() is not None) == sparse
    monkeypatch.setenv("CNMF_KL_SPARSE", "1")
    s = NMFBatchSolver(Xg, NMFOptions(n_components=72, beta_loss="kullback-leibler"))
    assert s._kl_sparse() is not None
    s = NMFBatchSolver(Xg, NMFOptions(n_components=200, beta_loss="kullback-leibler"))
    assert s._kl_sparse() is None


def test_options_carry_the_xwide_threshold_and_cpu_solver_stays_dense():
    """No GPU: NMFOptions has kl_sparse_density_xwide, and a CPU solver at K = 72 does not
    take the CSR route (the sparse ops are GPU kernels only)."""
    from cnmf_torch_amd.models.nmf import NMFBatchSolver, NMFOptions

    o = NMFOptions(n_components=72, beta_loss="kullback-leibler")
    assert isinstance(o.kl_sparse_density_xwide, float)
    assert 0.0 <= o.kl_sparse_density_xwide <= 1.0
    X = torch.from_numpy(_sparse_counts(200, 60, 0.08, seed=1))
    assert NMFBatchSolver(X, o)._kl_sparse() is None
