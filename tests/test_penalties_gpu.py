"""l1 / l2 penalties on the HIP kernels: every solve and beta-divergence kernel against its
float64 reference under penalties the comparison can see (the checks and their visibility
guard live in test_penalties_cpu.py, which runs them on the float32 reference), then the
solver and the refits on the GPU against the CPU with ``alpha`` / ``l1_reg`` set.
"""
import os
import warnings

import numpy as np
import pytest
import torch

from cnmf_torch_amd import ops
from test_penalties_cpu import (BETA_EPS, BETA_SETS, H_BLOCK_CASES, SOLVE_SETS,
                                SPARSE_CASES, SPARSE_ROWS, SPARSE_TOL, TOL_ANY,
                                TOL_WMFMA, DevSolve, check_beta_h_block_rule,
                                check_beta_h_block_step, check_beta_update_h,
                                check_beta_w_update, check_solve_case, check_solve_clamp,
                                check_solve_nsplit, check_solve_padded, gamma_counts, ref_solve,
                                solve_problem, sparse_kl_reference, visible)

pytestmark = pytest.mark.gpu

DEV = "cuda"
R = 3


def _fixed(algo, K, n, pens, **kw):
    """x after the six fixed steps of one more launch configuration."""
    return DevSolve(DEV, algo, *solve_problem(R, K, n, seed=K), **kw)(pens, 6)[0]


def _plan(algo, K, n, **kw):
    """What ops.solve launches for the penalised solves of one case (``kw`` as passed to
    check_solve_case / _fixed): the same under both stop rules."""
    plans = {ops.solve_plan(algo, K, n, R, penalised=True, conv_mode=c, **kw) for c in (0, 1)}
    assert len(plans) == 1, plans
    return plans.pop()


# ------------------------------------------------------------------------- A. ops.solve
@pytest.mark.parametrize("K", [3, 10, 16])
def test_solve_mfma_penalised(K):
    """solve_mfma.hip (MU, K <= 16, variant 'auto').  A penalised MU solve never takes the
    pipelined kernel, which has no penalty terms, and a launch that ignored them would miss
    the reference by >= 20x the tolerance (the guard)."""
    dev = torch.device(DEV)
    plan = _plan("mu", K, 777)                          # cooperative slices of <= 768 columns
    assert plan.kernel == "mfma"
    assert 0 < -(-777 // plan.slices) <= ops._hip.solve_mfma_max_cols(K)
    check_solve_case(DEV, "mu", K, 777)
    ops.coop_check(dev)


@pytest.mark.parametrize("algo", ["mu", "hals"])
@pytest.mark.parametrize("K", [3, 10, 17, 32])
def test_solve_streaming_penalised(algo, K):
    """solve.hip, the streaming VALU kernel (variant 'stream', K <= 32)."""
    assert _plan(algo, K, 777, variant="stream").kernel == "stream"
    check_solve_case(DEV, algo, K, 777, variant="stream")


@pytest.mark.parametrize("algo", ["mu", "hals"])
@pytest.mark.parametrize("K", [10, 16, 20, 24])
def test_solve_resident_penalised(algo, K):
    """solve_res*.hip with one column per thread (variant 'reg' raises when the slice does
    not fit the resident kernel)."""
    assert ops._hip.solve_reg_max_cols(K) >= 777
    plan = _plan(algo, K, 777, variant="reg", coop=1)
    assert (plan.kernel, plan.slices) == ("resident", 1)
    check_solve_case(DEV, algo, K, 777, variant="reg", coop=1)


@pytest.mark.parametrize("algo", ["mu", "hals"])
def test_solve_resident_lds_numerator_penalised(algo):
    """Resident kernel at U = 3 columns per thread: the numerator is staged in LDS already
    shifted by l1_num, and lin is taken from a reload of the raw one.  Bitwise equal to the
    streaming kernel on the fixed steps, as the unpenalised test asserts."""
    K, n = 10, 2600
    assert 2048 < n <= ops._hip.solve_reg_max_cols(K) == 3072
    assert _plan(algo, K, n, variant="reg", coop=1).kernel == "resident"
    assert _plan(algo, K, n, variant="stream", coop=1).kernel == "stream"
    out = check_solve_case(DEV, algo, K, n, variant="reg", coop=1)
    for pens, x in out.items():
        assert torch.equal(x, _fixed(algo, K, n, pens, variant="stream", coop=1)), pens


@pytest.mark.parametrize("algo", ["mu", "hals"])
@pytest.mark.parametrize("K", [40, 48, 64])
def test_solve_wide_penalised(algo, K):
    """solve_wide.hip (32 < K <= 64; a penalised MU solve has no matrix-core route there)."""
    assert _plan(algo, K, 777).kernel == "wide"
    check_solve_case(DEV, algo, K, 777)


@pytest.mark.parametrize("variant", ["auto", "stream"])
@pytest.mark.parametrize("K", [80, 96])
def test_solve_wmfma_penalised(K, variant):
    """solve_wmfma.hip (MU, 64 < K <= 128; 'auto' = split-bf16 Gram apply at K = 96) at its
    existing 2e-3 tolerance.  The denominators grow with K: P = (10, 5, 10) moves the
    float64 reference by only 18 / 9 / 25 x that tolerance at K = 80 and 14 / 6.5 / 21 x at
    K = 96 (l1_num / l1_den / l2), so these cases run 4 P = (40, 20, 40): 78 / 35 / 89 x and
    59 / 27 / 77 x."""
    bf16 = variant == "auto" and K == 96
    assert _plan("mu", K, 777, variant=variant).kernel == ("wmfma_bf16" if bf16 else "wmfma_f32")
    check_solve_case(DEV, "mu", K, 777, scale=4.0, t=TOL_WMFMA, variant=variant)


@pytest.mark.parametrize("algo,K", [("mu", 37), ("hals", 80)])
def test_solve_any_rank_penalised(algo, K):
    """solve_any.hip (a rank without a tiled instantiation; HALS beyond 64) with the
    tolerances of test_solve_any_rank_matches_float64_reference.  P = (10, 5, 10) moves
    the float64 reference by 50 / 23 / 64 x that tolerance at MU K = 37 and by > 2000 x at
    HALS K = 80."""
    assert _plan(algo, K, 777).kernel == "any"
    check_solve_case(DEV, algo, K, 777, t=TOL_ANY)


@pytest.mark.parametrize("algo,K,variants", [("mu", 10, ("stream", "reg")),
                                             ("hals", 10, ("stream", "reg")),
                                             ("mu", 40, ("auto",))])
def test_solve_cooperative_slices_penalised(algo, K, variants):
    """Three cooperating workgroups per replicate (n = 2600): parts 1-3 under variant
    'auto' -- the resident VALU kernel at K = 10 (three slices of 867 columns do not fit
    the matrix-core kernel's 768), solve_wide at K = 40 -- and per VALU kernel the fixed
    steps bitwise equal to one workgroup per replicate."""
    n, dev = 2600, torch.device(DEV)
    plan = _plan(algo, K, n, coop=3)
    assert (plan.kernel, plan.slices) == ("resident" if K == 10 else "wide", 3)
    check_solve_case(DEV, algo, K, n, coop=3)
    for variant in variants:
        plan = _plan(algo, K, n, variant=variant, coop=3)
        assert (plan.kernel, plan.slices) == (
            {"stream": "stream", "reg": "resident", "auto": "wide"}[variant], 3)
        for pens in SOLVE_SETS:
            a = _fixed(algo, K, n, pens, variant=variant, coop=3)
            assert torch.equal(a, _fixed(algo, K, n, pens, variant=variant, coop=1)), pens
    ops.coop_check(dev)


def test_solve_mfma_cooperative_slices_penalised():
    """MU K = 10, n = 2600 with four cooperating workgroups: slices of 650 columns, the
    matrix-core kernel's cooperative path under penalties (parts 1-3)."""
    dev = torch.device(DEV)
    plan = _plan("mu", 10, 2600, coop=4)
    assert (plan.kernel, plan.slices) == ("mfma", 4)
    check_solve_case(DEV, "mu", 10, 2600, coop=4)
    ops.coop_check(dev)


@pytest.mark.parametrize("K,n", [(10, 2600), (40, 2600), (10, 2100)])
def test_solve_column_split_penalised(K, n):
    """nsplit = 3, one step (batch mode's usage update): three workgroups per replicate,
    lin / quad summed by atomics.  At n = 2600 a slice (867 columns) exceeds the
    matrix-core kernel's 768, so K = 10 runs the VALU split and K = 40 solve_wide's; at
    n = 2100 (700 columns) K = 10 runs solve_mfma's split."""
    plan = _plan("mu", K, n, nsplit=3)
    assert (plan.kernel, plan.slices) == (
        {(10, 2600): "resident", (40, 2600): "wide", (10, 2100): "mfma"}[K, n], 3)
    check_solve_nsplit(DEV, K, n)


@pytest.mark.parametrize("algo", ["mu", "hals"])
@pytest.mark.parametrize("K", [10, 40])
def test_solve_numerator_clamp(algo, K):
    """l1_num at the numerator's 25th percentile: exact zeros under MU, the reference's
    zero pattern under HALS."""
    check_solve_clamp(DEV, algo, K)


def test_solve_padded_rank_penalised():
    """K = 37 zero-padded to 40: the padding stays exactly 0 under l1_den / l2."""
    check_solve_padded(DEV)


# --------------------------------------------------- B. beta-divergence / KL kernels
@pytest.mark.parametrize("pens", BETA_SETS)
@pytest.mark.parametrize("K", [10, 40])
@pytest.mark.parametrize("beta", [1.0, 0.0, 1.5])
def test_beta_update_h_penalised(beta, K, pens):
    """beta_mu.hip's fused usage step, six launches with the iterate rule.  In float64 the
    relative change per step is 0.86-0.97, 0.14-0.18, then <= 0.026 at beta 1 (tol 0.06),
    0.85-0.96 then 0.047-0.135 at beta 1.5 (tol 0.3), and halves down to 0.019-0.031 at
    beta 0 (tol 0.009, no stop): none within a factor 2 of its threshold."""
    check_beta_update_h(DEV, beta, K, pens)


@pytest.mark.parametrize("pens", BETA_SETS)
@pytest.mark.parametrize("beta,K,N,G", H_BLOCK_CASES)
def test_beta_h_block_penalised(beta, K, N, G, pens):
    """beta_planes*.hip: one rule-free step, then four 5-step blocks with the
    block-objective rule.  In float64 the block objective changes by 0.90-0.99 after block
    1 and 0.005-0.025 after block 2 for KL and beta 1.5 (tol 0.1), and by 0.06-0.20 then
    0.002-0.004 for IS (tol 0.015): every live replicate stops at its second check, none
    within a factor 2 of the threshold."""
    check_beta_h_block_step(DEV, beta, K, N, G, pens)
    check_beta_h_block_rule(DEV, beta, K, N, G, pens)


def _sparse_blocks(K, G, pens, act0):
    (X, HT, W), (hr, ar, ir, hsr), _ = sparse_kl_reference(K, G, pens, act0)
    dev = torch.device(DEV)
    a, b = SPARSE_ROWS
    Xg, Wg = X.float().to(dev), W.float().to(dev)
    csr = ops.kl_csr(Xg)
    h0 = HT.float().to(dev)[:, :, a:b].contiguous()
    h, act = h0.clone(), act0.to(dev)
    it = torch.zeros(3, dtype=torch.int32, device=dev)
    hs = torch.zeros((3, 2), dtype=torch.float64, device=dev)
    for blk in range(3):
        ops.kl_sparse_h_block(ops.kl_csr_rows(csr, a, b), h, Wg, BETA_EPS, 3, pens[0], pens[1],
                              act=act, tol=SPARSE_TOL, iters=it, hstate=hs, loss_entry=blk == 0)
    torch.testing.assert_close(h.cpu().double(), hr, rtol=1e-4, atol=1e-6)
    assert act.cpu().tolist() == ar.tolist() and it.cpu().tolist() == ir.tolist()
    torch.testing.assert_close(hs.cpu(), hsr, rtol=1e-5, atol=1e-6)
    return h0, h, it, hs


@pytest.mark.parametrize("pens", BETA_SETS)
@pytest.mark.parametrize("K,G", SPARSE_CASES)
def test_sparse_kl_h_block_penalised(K, G, pens):
    """sparse_kl.hip with one component slice (K <= 32) and four, W^T staged in LDS and gathered:
    three 3-step blocks with the rule (tol 0.05) against the float64 dense reference.  In
    float64 the block objective changes by 0.90-0.99 after block 1 and 0.002-0.007 after
    block 2 at these inputs under every penalty set."""
    assert {bool(ops._hip.sk_lds(g, k)) for k, g in SPARSE_CASES} == {True, False}
    _sparse_blocks(K, G, pens, torch.ones(3, dtype=torch.int32))


@pytest.mark.parametrize("K,G", [(10, 333), (64, 1200)])
def test_sparse_kl_h_block_penalised_gate(K, G):
    """act = [1, 0, 1] under penalties: the inactive replicate is bit-identical, with no
    steps counted and no objective state."""
    h0, h, it, hs = _sparse_blocks(K, G, BETA_SETS[0], torch.tensor([1, 0, 1], dtype=torch.int32))
    assert torch.equal(h[1], h0[1])
    assert not torch.equal(h[0], h0[0]) and not torch.equal(h[2], h0[2])
    assert it.cpu()[1] == 0 and hs[1].cpu().tolist() == [0.0, 0.0]


@pytest.mark.parametrize("pens", BETA_SETS)
@pytest.mark.parametrize("beta", [1.0, 0.0, 1.5])
def test_beta_w_update_penalised(beta, pens):
    """beta_mu.hip's anchored online spectra step."""
    check_beta_w_update(DEV, beta, pens)


# ------------------------------------------------------------------ C2. the solver
def _sparse_counts(n, g, density, seed):
    from cnmf_torch_amd.utils.synthetic import normalized_counts_matrix

    X = normalized_counts_matrix(n, g, n_programs=8, seed=seed)
    X[X < np.quantile(X, 1.0 - density)] = 0.0
    return X


def _solver_gpu_vs_cpu(X, K, alpha, cmp_tol, **kw):
    """The assertions of test_nmf_batch_gpu_matches_cpu with alpha_H = alpha_W = alpha,
    l1_ratio 0.5 on both sides; natively (an eager fallback warns -> fails); and on the
    CPU every replicate's err differs from the alpha = 0 run by >= 10 x cmp_tol."""
    from cnmf_torch_amd.models.nmf import run_nmf_batch

    seeds = [11, 12, 13]
    pen = dict(alpha_H=alpha, alpha_W=alpha, l1_ratio_H=0.5, l1_ratio_W=0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        g = run_nmf_batch(X, K, seeds, device="cuda", **pen, **kw)
    c = run_nmf_batch(X, K, seeds, device="cpu", **pen, **kw)
    c0 = run_nmf_batch(X, K, seeds, device="cpu", **kw)
    shift = np.abs(c.err - c0.err) / np.abs(c0.err)
    print("alpha", alpha, "shift of err on the CPU", shift, "passes", g.n_iter, c.n_iter)
    assert shift.min() >= 10 * cmp_tol, shift
    assert np.abs(g.n_iter - c.n_iter).max() <= 1, (g.n_iter, c.n_iter)
    same = g.n_iter == c.n_iter
    assert same.sum() >= 2, (g.n_iter, c.n_iter)
    rel = np.abs(g.err - c.err) / np.abs(c.err)
    assert rel[same].max() <= cmp_tol, (rel, g.n_iter, c.n_iter)
    assert rel.max() <= 2e-2, rel
    Wg, Wc = g.W.cpu().numpy(), c.W.cpu().numpy()
    ng, nc = np.linalg.norm(Wg, axis=1), np.linalg.norm(Wc, axis=1)
    # a strong l1 switches whole components off (all of their spectrum exactly 0): those
    # must be off on the GPU too; the cosine is taken over the others
    live = nc > 0
    print("live components", int(live.sum()), "of", live.size)
    assert live.reshape(len(seeds), -1).any(axis=1).all()
    assert (ng[~live] <= 1e-6 * ng.max()).all(), ng[~live]
    cos = (Wg * Wc).sum(1)[live] / (ng * nc)[live]
    assert np.median(cos) > 0.99, np.sort(cos)[:5]
    return g


# alpha per case: the smallest of 10 / 30 / 100 at which every replicate's err moves by
# >= 10 x the comparison tolerance on the CPU (observed shift beside it)
@pytest.mark.parametrize("algo,mode,K,alpha", [
    ("mu", "online", 6, 30.0),       # 3.1 % ... 20 %    (alpha 10: one replicate 0.2 %)
    ("mu", "batch", 6, 100.0),       # 5.8 % ... 20 %    (alpha 10: 0.4 % ... 0.7 %; 30: 1.2 %)
    ("hals", "online", 6, 100.0),    # 9.3 % ... 229 %   (alpha 10: 0.8 %; 30: 3.04 %)
    ("hals", "batch", 6, 10.0),      # 8.2 % ... 36 %
    ("mu", "online", 20, 30.0),      # 5.9 % ... 7.5 %   (alpha 10: 1.6 %)
    ("mu", "batch", 20, 10.0),       # 2.6 % ... 2.9 %
    ("hals", "online", 20, 10.0),    # 32 % ... 79 %
    ("hals", "batch", 20, 10.0),     # 52 % ... 71 %
    ("mu", "online", 40, 10.0),      # 4.7 % ... 6.7 %
])
def test_frobenius_solver_with_alpha_gpu_matches_cpu(algo, mode, K, alpha):
    """Frobenius MU (K = 6: matrix-core route, 20: VALU, 40: solve_wide) and HALS, online
    and batch, with alpha on both factors: the GPU run takes the plain penalised kernels
    and agrees with the CPU run as the unpenalised solver test demands (1e-3 MU, 3e-3
    HALS)."""
    _solver_gpu_vs_cpu(gamma_counts(), K, alpha, 1e-3 if algo == "mu" else 3e-3, algo=algo,
                       mode=mode, online_chunk_size=700, online_max_pass=5, batch_max_iter=40)


@pytest.mark.parametrize("mode,alpha", [("online", 30.0), ("batch", 100.0)])
def test_kl_solver_with_alpha_gpu_matches_cpu(mode, alpha):
    """KL at K = 6 (2e-2).  err moves by 57 % ... 160 % online at alpha 30 (alpha 10: one
    replicate 8.9 % < 10 x 2e-2) and by 122 % ... 154 % in batch mode at alpha 100 (alpha
    30: 20.3 % on one replicate)."""
    _solver_gpu_vs_cpu(gamma_counts(), 6, alpha, 2e-2, algo="mu", mode=mode,
                       beta_loss="kullback-leibler", online_chunk_size=700, online_max_pass=5,
                       batch_max_iter=40)


@pytest.mark.parametrize("K,alpha", [(6, 600.0), (40, 100.0)])
def test_sparse_kl_solver_with_alpha_gpu_matches_cpu(K, alpha):
    """Online KL on the CSR kernels (CNMF_KL_SPARSE=1; sparse_kl.hip, one slice at
    K = 6, four at 40) on the ~15 %-dense matrix of
    test_online_kl_wide_sparse_path_matches_dense.  Four passes of <= 20 inner steps, no
    outer stop (tol -1), so the CPU side stays quick and a rising err under the penalty
    cannot end the two runs at different passes.  err moves by 27 % ... 30 % at K = 6,
    alpha 600 (alpha 100: 6 % ... 8 %; 400: 22 % ... 24 %) and by 26 % ... 27 % at K = 40,
    alpha 100 (alpha 30: 8 % ... 9 %).  At that strength the l1 half switches most
    components off on this matrix -- 4 of 18 stay live at K = 6, 43 of 120 at K = 40 -- on
    both devices alike."""
    from cnmf_torch_amd.models.nmf import NMFBatchSolver, NMFOptions

    X = _sparse_counts(1500, 300, 0.15, seed=3)
    old = os.environ.get("CNMF_KL_SPARSE")
    try:
        os.environ["CNMF_KL_SPARSE"] = "1"
        s = NMFBatchSolver(torch.from_numpy(X).cuda(),
                           NMFOptions(n_components=K, beta_loss="kullback-leibler"))
        assert s._kl_sparse() is not None
        _solver_gpu_vs_cpu(X, K, alpha, 2e-2, algo="mu", mode="online",
                           beta_loss="kullback-leibler", online_chunk_size=500,
                           online_max_pass=4, online_chunk_max_iter=20, tol=-1.0)
    finally:
        if old is None:
            os.environ.pop("CNMF_KL_SPARSE", None)
        else:
            os.environ["CNMF_KL_SPARSE"] = old


# ------------------------------------------------------------------ C3. the refits
# Guard ratios on the float64 operands at rtol 5e-3 / atol 1e-5.  Usage refit, (l1, l2) =
# (40, 100): 655 / 265 x at K = 7, 776 / 178 x at K = 37 ((20, 50): l2 only 12 x at K = 37).
# Spectra refit from those usages, l1 = 2: 31 x at K = 7, > 1000 x at K = 37 (its numerators
# are 3.5 ... 8; l1 >= 20 clamps every one of them to zero and the refit returns zeros).
REFIT_L1, REFIT_L2, REFIT_SPECTRA_L1 = 40.0, 100.0, 2.0


def _refit_guard(numer, gram, seed_cols, pens):
    """The guard on chunked_solve's operands (float64 copies of what the refit forms):
    30 MU steps at most, iterate rule at h_tol 0.05, from the refit's seeded init."""
    from cnmf_torch_amd.models.refit import _init_HT

    K = gram.shape[0]
    x0 = _init_HT(K, seed_cols, None, "cpu", torch.float32, 0).double()[None]
    visible(lambda *p: ref_solve("mu", x0, numer[None], gram[None], p, 30, 0.05)[0], pens,
            5e-3, 1e-5)


@pytest.mark.parametrize("K", [7, 37])
def test_refits_with_l1_l2_gpu_match_cpu(K):
    """fit_H_online(l1_reg_H, l2_reg_H) and fit_spectra_online(l1_reg) on the GPU against
    the CPU at K = 7 (runs as it is) and K = 37 (padded to 40), with the tolerance of
    test_refit_wide_and_unpadded_k_on_gpu (rtol 5e-3, atol 1e-5)."""
    from cnmf_torch_amd.models.refit import fit_H_online, fit_spectra_online

    rs = np.random.default_rng(0)
    X = rs.random((900, 300)).astype(np.float32)
    W = rs.random((K, 300)).astype(np.float32)
    Xd, Wd = torch.from_numpy(X).double(), torch.from_numpy(W).double()
    _refit_guard(Wd @ Xd.t(), Wd @ Wd.t(), 900, (REFIT_L1, 0.0, REFIT_L2))
    kw = dict(l1_reg_H=REFIT_L1, l2_reg_H=REFIT_L2, chunk_max_iter=30)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        hg = fit_H_online(X, W, device="cuda", **kw)
    hc = fit_H_online(X, W, device="cpu", **kw)
    np.testing.assert_allclose(hg, hc, rtol=5e-3, atol=1e-5)
    Ud = torch.from_numpy(hc).double()
    _refit_guard(Ud.t() @ Xd, Ud.t() @ Ud, 300, (REFIT_SPECTRA_L1, 0.0, 0.0))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        sg = fit_spectra_online(X, hc, device="cuda", chunk_max_iter=30,
                                l1_reg=REFIT_SPECTRA_L1)
    sc = fit_spectra_online(X, hc, device="cpu", chunk_max_iter=30, l1_reg=REFIT_SPECTRA_L1)
    assert float((sc > 0).mean()) > 0.9 and float((hc > 0).mean()) > 0.9    # not clamped away
    np.testing.assert_allclose(sg, sc, rtol=5e-3, atol=1e-5)
