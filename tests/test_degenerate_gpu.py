"""Exactly degenerate inputs on the HIP kernels: dead components, zero columns and rows,
all-zero numerators and Grams through every solve kernel; dead spectra and usages, cells
without usage (P clamped at eps, at the kernel tests' 1e-10 and the solver's 1e-16) and
empty cells / genes through every beta-divergence and CSR KL kernel; then the solver from
``init="nndsvd"``, whose factors are 45 % exact zeros, on the GPU against the CPU.  The
inputs and checks live in test_degenerate_cpu.py, which runs them on the float32 reference;
every case here asserts the kernel it launches.
"""
import os

import numpy as np
import pytest
import torch

from cnmf_torch_amd import ops
from test_penalties_cpu import TOL_ANY, TOL_TILED, TOL_WMFMA, DevSolve, gamma_counts
from test_degenerate_cpu import (BETA_EPSES, BETAS, DEGENERATE_SETS, H_BLOCK_SHAPES,
                                 NNDSVD_ROUTES, PLAIN, SPARSE_DEGENERATE_CASES,
                                 SPARSE_PATTERN, check_beta_contract_degenerate,
                                 check_beta_h_block_degenerate,
                                 check_beta_h_block_rule_degenerate,
                                 check_beta_update_h_degenerate,
                                 check_beta_w_update_degenerate, check_kl_fp16_degenerate,
                                 check_solve_degenerate, check_solve_degenerate_gram_of,
                                 check_solve_degenerate_nsplit, check_solve_degenerate_padded,
                                 check_sparse_kl_degenerate, degenerate_solve_problem,
                                 run_from_nndsvd, sparse_counts)

pytestmark = pytest.mark.gpu

DEV = "cuda"
R = 5


def _plan(algo, K, n, pens, conv_modes=(0, 1), **kw):
    """What ops.solve launches for one case under each of its stop rules."""
    plans = {ops.solve_plan(algo, K, n, R, penalised=pens != PLAIN, conv_mode=c, **kw)
             for c in conv_modes}
    assert len(plans) == 1, plans
    return plans.pop()


def _solve_case(kernel, algo, K, n, t=TOL_TILED, conv_modes=(0, 1), slices=None, **kw):
    """check_solve_degenerate under the three penalty sets, each on the asserted kernel."""
    for pens in DEGENERATE_SETS:
        plan = _plan(algo, K, n, pens, conv_modes, **kw)
        assert plan.kernel == kernel, (plan, pens)
        if slices is not None:
            assert plan.slices == slices, plan
        check_solve_degenerate(DEV, algo, K, n, pens, t, conv_modes, **kw)


# ------------------------------------------------------------------------- A. ops.solve
@pytest.mark.parametrize("K", [3, 10, 16])
def test_solve_mfma_degenerate(K):
    """solve_mfma.hip (MU, K <= 16) under the iterate rule (an unpenalised solve under the
    objective rule takes the pipelined kernel: next test)."""
    _solve_case("mfma", "mu", K, 777, conv_modes=(0,))
    ops.coop_check(torch.device(DEV))


@pytest.mark.parametrize("K", [10, 24, 32, 40])
def test_solve_pipe_degenerate(K):
    """solve_pipe*.hip: the single-tile instantiations (K <= 16), solve_pipe_b2 (17-24),
    _b3 (25-32) and _b4 (40 ...).  Unpenalised and under the objective rule only -- the
    planner routes nothing else there -- so the fixed steps run under that rule with tol =
    -1 and the step counts are the reference's: the all-zero replicates stop early."""
    assert ops._hip.solve_pipe_k(K)
    assert _plan("mu", K, 777, PLAIN, (1,)).kernel == "pipe"
    check_solve_degenerate(DEV, "mu", K, 777, PLAIN, conv_modes=(1,))
    ops.coop_check(torch.device(DEV))


def test_solve_pipe_bitwise_equals_mfma_kernel_degenerate(monkeypatch):
    """test_solve_pipe_bitwise_equals_mfma_kernel's equality on the degenerate problem: the
    pipelined kernel and (CNMF_SOLVE_PIPE=0) solve_mfma.hip agree bitwise in x, lin, quad
    and the step counts, fixed steps and converged."""
    K, n = 10, 777
    run = DevSolve(DEV, "mu", *degenerate_solve_problem(K, n, seed=K))
    out = {}
    for pipe in ("1", "0"):
        monkeypatch.setenv("CNMF_SOLVE_PIPE", pipe)
        ops.refresh_env()
        assert _plan("mu", K, n, PLAIN, (1,)).kernel == ("pipe" if pipe == "1" else "mfma")
        out[pipe] = (run(PLAIN, 6, tol=-1.0, conv_mode=1, check_every=2)
                     + run(PLAIN, 60, tol=1e-3, conv_mode=1, check_every=5))
    monkeypatch.delenv("CNMF_SOLVE_PIPE")
    ops.refresh_env()
    ops.coop_check(torch.device(DEV))
    for a, b in zip(out["1"], out["0"]):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(out["1"][0]).all())


@pytest.mark.parametrize("algo", ["mu", "hals"])
@pytest.mark.parametrize("K", [3, 17, 32])
def test_solve_streaming_degenerate(algo, K):
    """solve.hip, the streaming VALU kernel (variant 'stream')."""
    _solve_case("stream", algo, K, 777, variant="stream")


@pytest.mark.parametrize("algo", ["mu", "hals"])
@pytest.mark.parametrize("K,n", [(10, 777), (24, 777), (10, 2600)])
def test_solve_resident_degenerate(algo, K, n):
    """solve_res*.hip, one workgroup per replicate (variant 'reg', coop = 1); n = 2600 is
    U = 3 columns per thread with the numerator staged in LDS."""
    assert ops._hip.solve_reg_max_cols(K) >= n
    _solve_case("resident", algo, K, n, slices=1, variant="reg", coop=1)


@pytest.mark.parametrize("algo", ["mu", "hals"])
@pytest.mark.parametrize("K", [40, 64])
def test_solve_wide_degenerate(algo, K):
    """solve_wide.hip (32 < K <= 64; variant 'stream' keeps the unpenalised MU solve under
    the objective rule off the pipelined kernel)."""
    _solve_case("wide", algo, K, 777, variant="stream")


@pytest.mark.parametrize("K,kernel", [(80, "wmfma_f32"), (96, "wmfma_bf16")])
def test_solve_wmfma_degenerate(K, kernel):
    """solve_wmfma.hip: the fp32 and the split-bf16 Gram apply (MU, 64 < K <= 128)."""
    _solve_case(kernel, "mu", K, 777, t=TOL_WMFMA)


@pytest.mark.parametrize("algo,K", [("mu", 37), ("hals", 80)])
def test_solve_any_rank_degenerate(algo, K):
    """solve_any.hip (a rank without a tiled instantiation; HALS beyond 64)."""
    _solve_case("any", algo, K, 777, t=TOL_ANY)


@pytest.mark.parametrize("algo,K,variant,kernel", [("mu", 10, "stream", "stream"),
                                                   ("mu", 10, "reg", "resident"),
                                                   ("hals", 10, "stream", "stream"),
                                                   ("hals", 10, "reg", "resident"),
                                                   ("mu", 40, "stream", "wide"),
                                                   ("hals", 40, "stream", "wide")])
def test_solve_cooperative_slices_degenerate(algo, K, variant, kernel):
    """Three cooperating workgroups per replicate (n = 2600, slices of 867 columns): the
    zero columns of replicate 1 cross both slice boundaries, and the all-zero replicates'
    norms and objectives are exchanged as exact zeros."""
    _solve_case(kernel, algo, K, 2600, slices=3, variant=variant, coop=3)
    ops.coop_check(torch.device(DEV))


def test_solve_mfma_cooperative_slices_degenerate():
    """solve_mfma.hip with four cooperating workgroups (slices of 650 columns)."""
    _solve_case("mfma", "mu", 10, 2600, conv_modes=(0,), slices=4, coop=4)
    ops.coop_check(torch.device(DEV))


@pytest.mark.parametrize("K,n,kernel", [(10, 2600, "resident"), (40, 2600, "wide"),
                                        (10, 2100, "mfma")])
def test_solve_column_split_degenerate(K, n, kernel):
    """nsplit = 3, one step: lin / quad are summed by atomics and stay exactly 0 for the
    all-zero replicates."""
    for pens in DEGENERATE_SETS:
        plan = _plan("mu", K, n, pens, nsplit=3)
        assert (plan.kernel, plan.slices) == (kernel, 3)
        check_solve_degenerate_nsplit(DEV, K, n, pens)


def test_solve_gram_of_degenerate():
    """ops.solve(gram_of=F) with a zero factor row: solve_mfma.hip forms the Gram, with its
    zero row and column, in its prologue."""
    for cm in (0, 1):
        assert ops.solve_plan("mu", 10, 777, 6, conv_mode=cm, gram_of=True).kernel == "mfma"
    check_solve_degenerate_gram_of(DEV)
    ops.coop_check(torch.device(DEV))


def test_solve_padded_rank_degenerate():
    """K = 37 zero-padded to 40 with a dead component among the real 37 (solve_wide.hip)."""
    assert _plan("mu", 40, 777, PLAIN, (0,)).kernel == "wide"
    check_solve_degenerate_padded(DEV)


# --------------------------------------------------- B. beta-divergence / KL kernels
def _panel_kernels(beta, K):
    """beta_planes*.hip unless the rank is beyond the panels (IS / general beta K > 56),
    where the op runs beta_any.hip; KL with the default numerator."""
    assert ops.beta_any_k(K, beta) == (beta != 1.0 and K > 56)
    assert ops.bp_mode(beta) != ops.BP_KL_FP16


@pytest.mark.parametrize("eps", BETA_EPSES)
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("K,N,G", H_BLOCK_SHAPES)
def test_beta_h_block_degenerate(beta, K, N, G, eps):
    """ops.beta_h_block: one and five rule-free steps, then four 5-step blocks with the
    block-objective rule (thresholds and measured changes: H_RULE_TOL,
    check_beta_h_block_rule_degenerate)."""
    _panel_kernels(beta, K)
    check_beta_h_block_degenerate(DEV, beta, K, N, G, eps)
    check_beta_h_block_rule_degenerate(DEV, beta, K, N, G, eps)


@pytest.mark.parametrize("eps", BETA_EPSES)
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("K", [10, 40])
def test_beta_update_h_degenerate(beta, K, eps):
    """beta_mu.hip's fused usage step."""
    assert not ops.beta_any_k(K, beta) and K <= ops._hip.beta_max_k()
    check_beta_update_h_degenerate(DEV, beta, K, eps)


@pytest.mark.parametrize("eps", BETA_EPSES)
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("K", [10, 40, 64, 80])
def test_beta_contract_and_loss_degenerate(beta, K, eps):
    """ops.beta_contract on both sides (beta_mu.hip; K = 80, and 64 for IS / general beta:
    beta_any.hip) and ops.beta_loss (beta_planes*.hip below those ranks)."""
    assert ops.beta_any_k(K, beta) == (K > (64 if beta == 1.0 else 56))
    check_beta_contract_degenerate(DEV, beta, K, eps)


@pytest.mark.parametrize("eps", BETA_EPSES)
@pytest.mark.parametrize("beta", BETAS)
def test_beta_w_update_degenerate(beta, eps):
    """ops.beta_w_partials (beta_planes*.hip, side 1) + ops.beta_w_update (beta_mu.hip): the
    ``B == 0 -> eps`` branch of the spectra update."""
    _panel_kernels(beta, 7)
    check_beta_w_update_degenerate(DEV, beta, eps)


@pytest.mark.parametrize("eps", BETA_EPSES)
@pytest.mark.parametrize("K,N,G", [(10, 777, 320), (40, 300, 131)])
def test_kl_fp16_numerator_degenerate(monkeypatch, K, N, G, eps):
    """The opt-in fp16 numerator (CNMF_KL_FP16=1) with x / eps = 1e10 or 1e16 wherever P is
    exactly 0 -- the cells without usage and, in every cell, the gene without loading: the
    usage block and the spectra partials.  (Before beta_planes.h dropped those elements
    from the fp16 plane, every column that held one was shifted by 2^24 and lost its other
    terms: replicate 2's usages missed float64 by 200-600 x this tolerance, 99 % of its
    spectra partials by up to 2000 x.)"""
    monkeypatch.setenv("CNMF_KL_FP16", "1")
    ops.refresh_env()
    try:
        assert ops.bp_mode(1.0) == ops.BP_KL_FP16
        check_kl_fp16_degenerate(DEV, K, N, G, eps)
    finally:
        monkeypatch.delenv("CNMF_KL_FP16")
        ops.refresh_env()


# ------------------------------------------------------------------- C. CSR KL kernels
def _csr_kl():
    def h_block(X, a, b, h, W, eps, nsteps, **kw):
        ops.kl_sparse_h_block(ops.kl_csr_rows(ops.kl_csr(X), a, b), h, W, eps, nsteps, **kw)

    def loss(X, h, W, eps):
        return ops.kl_sparse_loss(ops.kl_csr(X), h, W, eps)

    def w_num(Xc, h, W, eps, K):
        return ops.kl_sparse_w_num(ops.kl_csr_tiles(Xc, K), h, W, eps).sum(0)

    return h_block, loss, w_num


@pytest.mark.parametrize("eps", BETA_EPSES)
@pytest.mark.parametrize("K,G", SPARSE_DEGENERATE_CASES)
def test_sparse_kl_degenerate(K, G, eps):
    """sparse_kl.hip with 1 (K <= 32), 4 (33-64) and 8 (65-128) component slices,
    W^T staged in LDS and gathered from L2: usage blocks with the rule, loss and spectra
    numerators with a dead spectrum, dead usages, an empty gene and cells without usage
    (eps + P = eps exactly)."""
    assert {bool(ops._hip.sk_lds(g, k)) for k, g in SPARSE_DEGENERATE_CASES} == {True, False}
    check_sparse_kl_degenerate(DEV, K, G, eps, impl=_csr_kl())


# ------------------------------------------------------------------ D. the solver
def _gpu_vs_cpu(X, K, route, **extra):
    opts, tol, mu = NNDSVD_ROUTES[route]
    g = run_from_nndsvd(X, K, "cuda", mu_route=mu, **opts, **extra)
    c = run_from_nndsvd(X, K, "cpu", mu_route=mu, **opts, **extra)
    rel = np.abs(g.err - c.err) / np.abs(c.err)
    print(route, "K", K, "err GPU vs CPU", rel, "passes", g.n_iter, c.n_iter)
    assert np.abs(g.n_iter - c.n_iter).max() <= 1, (g.n_iter, c.n_iter)
    same = g.n_iter == c.n_iter
    assert same.any(), (g.n_iter, c.n_iter)
    assert rel[same].max() <= tol, (rel, g.n_iter, c.n_iter)
    assert rel.max() <= 2e-2, rel
    return g, c


@pytest.mark.parametrize("route,K", [("mu-online", 6), ("mu-online", 40), ("mu-batch", 6),
                                     ("hals-online", 6), ("kl-online", 6), ("is-online", 6)])
def test_solver_from_nndsvd_gpu_matches_cpu(route, K):
    """run_nmf_batch from init="nndsvd" (45 % of both factors exactly 0) natively on the
    GPU against the CPU: err within the route's tolerance (those of
    test_nmf_batch_gpu_matches_cpu: 1e-3 MU, 3e-3 HALS, 2e-2 KL; IS takes the KL figure),
    passes within 1, finite outputs, and on the MU routes the spectra's zeros are exactly
    the init's."""
    _gpu_vs_cpu(gamma_counts(), K, route)


@pytest.mark.parametrize("K", [6, 40])
def test_sparse_kl_solver_from_nndsvd_gpu_matches_cpu(K):
    """The same on the CSR kernels (CNMF_KL_SPARSE=1; sparse_kl.hip, one slice at
    K = 6, four at 40) on the ~15 %-dense matrix."""
    from cnmf_torch_amd.models.nmf import NMFBatchSolver, NMFOptions

    X = sparse_counts()
    old = os.environ.get("CNMF_KL_SPARSE")
    try:
        os.environ["CNMF_KL_SPARSE"] = "1"
        s = NMFBatchSolver(torch.from_numpy(X).cuda(),
                           NMFOptions(n_components=K, beta_loss="kullback-leibler"))
        assert s._kl_sparse() is not None
        _gpu_vs_cpu(X, K, "kl-online", pattern=SPARSE_PATTERN[K])
    finally:
        if old is None:
            os.environ.pop("CNMF_KL_SPARSE", None)
        else:
            os.environ["CNMF_KL_SPARSE"] = old
