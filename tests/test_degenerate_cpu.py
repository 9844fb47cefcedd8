"""Exactly degenerate inputs: dead components, zero columns, eps-clamped products.

Every solve and beta-divergence kernel has branches that only run on exactly degenerate
input -- the MU rate 0 where the denominator is < eps, the HALS component kept where
Gram_kk + l2 <= eps, ``den == 0 -> eps``, ``P`` clamped at ``eps`` -- and production feeds
them: ``init="nndsvd"`` writes exact zeros into both factors, a strong l1 switches whole
components off, padded ranks carry zero rows, and the solver passes ``eps = 1e-16``.  The
input constructors and the checks live here, each written once against a device.  This
file runs them on the CPU, where ``ops`` evaluates ``ops/reference.py`` in float32 -- so
the tolerances and the exactness claims are conditions a float32 implementation can meet
-- and prints the ratios to tolerance; ``test_degenerate_gpu.py`` runs the same checks on
each HIP kernel.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.ops import reference
from test_penalties_cpu import (SPARSE_ROWS, SPARSE_TOL, TOL_TILED, TOL_WMFMA, DevSolve,
                                _gamma, beta_problem, gamma_counts, off_threshold,
                                ratio_to_tol, ref_solve, solve_problem, sparse_problem)

# (l1_num, l1_den, l2): unpenalised, l2 alone, l1_den alone.  A zero numerator stays an
# exact MU zero under the last two (x . 0 / den = 0 with den > 0).
PLAIN = (0.0, 0.0, 0.0)
DEGENERATE_SETS = [PLAIN, (0.0, 0.0, 10.0), (0.0, 5.0, 0.0)]
# the kernel tests' eps and the solver's (NMFOptions.eps)
BETA_EPSES = [1e-10, 1e-16]
BETAS = [1.0, 0.0, 1.5]


def worst(report, what, ratio):
    """Collect and print one ratio to tolerance."""
    print(f"{what}: {ratio:.3f} of its tolerance")
    if report is not None:
        report.append(ratio)
    return ratio


# ------------------------------------------------------------------------- A. solve
def zero_columns(n):
    """(numerator, iterate) column ranges of replicate 1 that are set to 0: 40 and 30
    columns that straddle multiples of 16 (100:140, 200:230), and for the sliced sizes 20
    columns across each boundary of three slices (n = 2600, slices of 867: 860:880 and
    1725:1745)."""
    num, it = [(100, 140)], [(200, 230)]
    if n > 777:
        s = -(-n // 3)
        num.append((s - 7, s + 13))
        it.append((2 * s - 9, 2 * s + 11))
    return num, it


@functools.lru_cache(maxsize=None)
def degenerate_solve_problem(K, n, seed):
    """solve_problem(5, K, n, seed) with exact changes, made in float64 after the float32
    round trip (both sides see identical operands):
      0  dead component d = K // 3: its Gram row, Gram column and numerator row are 0
      1  iterate row K // 2 is 0; zero_columns(n) of the numerator / of the iterate are 0
      2  the numerator is 0 (nothing to fit)
      3  Gram and numerator are 0
      4  untouched (control)
    At K = 1 the changes to replicates 0 and 1's row would repeat 3 and 2: skipped.
    Cached: the callers leave the tensors unchanged."""
    x0, numer, gram = solve_problem(5, K, n, seed)
    d, h = K // 3, K // 2
    if K > 1:
        gram[0, d, :] = 0.0
        gram[0, :, d] = 0.0
        numer[0, d, :] = 0.0
        x0[1, h, :] = 0.0
    ncols, xcols = zero_columns(n)
    for a, b in ncols:
        numer[1, :, a:b] = 0.0
    for a, b in xcols:
        x0[1, :, a:b] = 0.0
    numer[2] = 0.0
    gram[3] = 0.0
    numer[3] = 0.0
    assert bool((x0[0] > 0).all())
    return x0, numer, gram


@functools.lru_cache(maxsize=None)
def degenerate_ref_solve(algo, K, n, pens, max_iter, tol=-1.0, conv_mode=0, check_every=5,
                         nsplit=1):
    """The float64 reference on degenerate_solve_problem(K, n, seed=K), computed once and
    shared by every kernel's test of that case."""
    return ref_solve(algo, *degenerate_solve_problem(K, n, seed=K), pens, max_iter, tol,
                     conv_mode, check_every, nsplit)


def _atol(t, xr):
    return t["atol"] if t["atol"] >= 0 else -t["atol"] * float(xr.abs().max())


def _finite(*ts):
    return all(bool(torch.isfinite(t.double()).all()) for t in ts)


def check_solve_degenerate(dev, algo, K, n, pens, t=TOL_TILED, conv_modes=(0, 1), report=None,
                           **kw):
    """Parts 1-3 on degenerate_solve_problem(K, n, seed=K); ``kw`` goes to ops.solve.
    ``conv_modes``: the stop rules of part 2; the fixed steps of part 1 run under the first
    (rule 1 with tol = -1 and a check every 2 steps: with f_prev = 0 the rule |f_prev - f|
    <= tol |f_prev| reads 0 <= -0, so an all-zero replicate stops at its second zero check
    in the reference too -- the step counts are compared with the reference's, not with 6).
    Returns the device's x after the fixed steps."""
    x0, numer, gram = degenerate_solve_problem(K, n, seed=K)
    run = DevSolve(dev, algo, x0, numer, gram, **kw)
    d, h = K // 3, K // 2
    ncols, xcols = zero_columns(n)
    cm = conv_modes[0]
    # ---- 1. six fixed steps
    xr, lr, qr, ir = degenerate_ref_solve(algo, K, n, pens, 6, -1.0, cm, 2)
    xg, lg, qg, ig = run(pens, 6, tol=-1.0, conv_mode=cm, check_every=2)
    assert _finite(xg, lg, qg), "non-finite output"
    assert ig.tolist() == ir.tolist(), (ig.tolist(), ir.tolist())
    if cm == 0:
        assert ir.tolist() == [6] * 5
    r = worst(report, f"{algo} K={K} n={n} {pens} x", ratio_to_tol(xg, xr, t["rtol"], _atol(t, xr)))
    assert r <= 1.0, r
    torch.testing.assert_close(lg, lr, rtol=t["lq"], atol=1e-3)
    torch.testing.assert_close(qg, qr, rtol=t["lq"], atol=1e-3)
    x0f = x0.float()
    if algo == "mu":
        # holds under every set of DEGENERATE_SETS, for the reference and the device alike
        for x in (xr, xg):
            if K > 1:
                assert bool((x[0, d] == 0).all()), "dead component"
                assert bool((x[1, h] == 0).all()), "dead iterate row"
            for a, b in ncols + xcols:
                assert bool((x[1, :, a:b] == 0).all()), ("zero columns", a, b)
            assert bool((x[2] == 0).all()) and bool((x[3] == 0).all())
        assert lg[2] == 0 and qg[2] == 0 and lg[3] == 0 and qg[3] == 0
        if K > 1:
            live = [k for k in range(K) if k != d]
            assert bool((xg[0, live] > 0).all())
        assert bool((xg[4] > 0).all())
    elif pens == PLAIN:
        # Gram_kk + l2 <= eps keeps the component: bit-identical to x0
        if K > 1:
            assert torch.equal(xg[0, d], x0f[0, d]) and torch.equal(xr[0, d], x0[0, d])
        assert torch.equal(xg[3], x0f[3]) and torch.equal(xr[3], x0[3])
        if K > 1:
            assert float(xr[1, h].max()) > 10 * t["rtol"] and float(xg[1, h].max()) > 0, "revives"
    # ---- 2. converged, unpenalised
    if pens == PLAIN:
        for conv_mode in conv_modes:
            ir = degenerate_ref_solve(algo, K, n, pens, 60, 1e-3, conv_mode, 5)[3]
            xc, lc, qc, ic = run(pens, 60, tol=1e-3, conv_mode=conv_mode, check_every=5)
            assert _finite(xc, lc, qc), "non-finite output"
            slack = 1 if conv_mode == 0 else 5
            diff = (ic - ir).abs()
            assert int(diff[[0, 1, 4]].max()) <= slack, (conv_mode, ic.tolist(), ir.tolist())
            # MU: x is exactly 0 after one step in any precision (2: zero numerator, 3: rate
            # 0); HALS keeps x[3] unchanged, so its change is exactly 0.  HALS on replicate
            # 2 decays and crosses tol between float64 (2 steps) and float32 (3)
            assert int(diff[3]) == 0, (conv_mode, ic.tolist(), ir.tolist())
            assert int(diff[2]) <= (0 if algo == "mu" else slack), (conv_mode, ic.tolist(),
                                                                    ir.tolist())
            if algo == "mu":
                assert ir[2:4].tolist() == ([2, 2] if conv_mode == 0 else [10, 5])
    # ---- 3. a zero-step launch moves nothing
    assert torch.equal(run(pens, 0, conv_mode=cm)[0], x0f)
    return xg


def check_solve_degenerate_nsplit(dev, K, n, pens, report=None):
    """One MU step with the columns split over three blocks: lin / quad are summed by
    atomics and must still be exactly 0 for the all-zero replicates."""
    x0, numer, gram = degenerate_solve_problem(K, n, seed=K)
    xr, lr, qr, ir = degenerate_ref_solve("mu", K, n, pens, 1, nsplit=3)
    xg, lg, qg, ig = DevSolve(dev, "mu", x0, numer, gram)(pens, 1, nsplit=3)
    assert _finite(xg, lg, qg)
    assert ig.tolist() == ir.tolist() == [1] * 5
    r = worst(report, f"mu nsplit K={K} n={n} {pens} x",
              ratio_to_tol(xg, xr, TOL_TILED["rtol"], TOL_TILED["atol"]))
    assert r <= 1.0, r
    torch.testing.assert_close(lg, lr, rtol=TOL_TILED["lq"], atol=1e-3)
    torch.testing.assert_close(qg, qr, rtol=TOL_TILED["lq"], atol=1e-3)
    assert bool((xg[0, K // 3] == 0).all()) and bool((xg[1, K // 2] == 0).all())
    assert bool((xg[2] == 0).all()) and bool((xg[3] == 0).all())
    assert lg[2] == 0 and qg[2] == 0 and lg[3] == 0 and qg[3] == 0


def check_solve_degenerate_padded(dev, K=37, Kp=40, n=777, report=None):
    """The rank-37 degenerate problem zero-padded to 40 as the engine runs it, MU,
    unpenalised: the padding rows and the dead row are exactly 0, the rest equals the
    float64 reference of the unpadded problem."""
    x0, numer, gram = degenerate_solve_problem(K, n, seed=K)
    R = x0.shape[0]
    xp = torch.zeros((R, Kp, n), dtype=torch.float64)
    npad, gp = torch.zeros_like(xp), torch.zeros((R, Kp, Kp), dtype=torch.float64)
    xp[:, :K], npad[:, :K], gp[:, :K, :K] = x0, numer, gram
    xr, lr, qr, _ = degenerate_ref_solve("mu", K, n, PLAIN, 6)
    xg, lg, qg, ig = DevSolve(dev, "mu", xp, npad, gp)(PLAIN, 6)
    assert _finite(xg, lg, qg) and ig.tolist() == [6] * R
    assert bool((xg[:, K:] == 0).all()), "padding rows"
    assert bool((xg[0, K // 3] == 0).all()) and bool((xg[1, K // 2] == 0).all())
    assert bool((xg[2] == 0).all()) and bool((xg[3] == 0).all())
    r = worst(report, f"mu K={K} padded to {Kp} x",
              ratio_to_tol(xg[:, :K], xr, TOL_TILED["rtol"], TOL_TILED["atol"]))
    assert r <= 1.0, r
    torch.testing.assert_close(lg, lr, rtol=TOL_TILED["lq"], atol=1e-3)
    torch.testing.assert_close(qg, qr, rtol=TOL_TILED["lq"], atol=1e-3)


def check_solve_degenerate_gram_of(dev, K=10, m=333, n=777, report=None):
    """ops.solve(gram_of=F) with a zero row in replicate 0's factor (call shape of
    test_solve_gram_of_matches_explicit_gram: strided F, an inactive replicate, fixed
    steps and a converged solve): same iterates as with the explicit Gram, the dead
    component exactly 0, and the fixed steps equal to the float64 reference."""
    R, d = 6, K // 3
    g = torch.Generator().manual_seed(K + m)
    F = torch.rand((R, K, m + 3), generator=g) + 0.05
    F[0, d] = 0.0
    gram = torch.bmm(F[:, :, 1:m + 1].double(), F[:, :, 1:m + 1].transpose(1, 2).double()).float()
    x0 = torch.rand((R, K, n), generator=g) + 0.1
    numer = torch.bmm(gram, torch.rand((R, K, n), generator=g))
    assert bool((gram[0, d] == 0).all()) and bool((numer[0, d] == 0).all())
    dv = torch.device(dev)
    Fd = F.to(dv)[:, :, 1:m + 1]
    numer_d, gram_d = numer.to(dv), gram.to(dv)
    active = torch.tensor([1, 1, 0, 1, 1, 1], dtype=torch.int32, device=dv)
    for max_iter, tol, cm in ((6, -1.0, 0), (300, 1e-4, 1)):
        outs = []
        for use_of in (False, True):
            xg = x0.clone().to(dv)
            lin = torch.zeros(R, device=dv)
            it = torch.zeros(R, dtype=torch.int32, device=dv)
            ops.solve("mu", xg, numer_d, None if use_of else gram_d, max_iter=max_iter, tol=tol,
                      conv_mode=cm, check_every=5, lin_out=lin, iters_out=it, active=active,
                      gram_of=Fd if use_of else None)
            outs.append((xg.cpu(), lin.cpu(), it.cpu()))
        (xa, la, ia), (xb, lb, ib) = outs
        assert _finite(xa, la, xb, lb)
        torch.testing.assert_close(xb, xa, rtol=2e-5, atol=1e-6)
        torch.testing.assert_close(lb, la, rtol=2e-5, atol=1e-4)
        assert (ib - ia).abs().max() <= (0 if tol < 0 else 5)
        assert torch.equal(xb[2], x0[2])
        for x in (xa, xb):
            assert bool((x[0, d] == 0).all())
        if tol < 0:
            live = [0, 1, 3, 4, 5]
            xr = ref_solve("mu", x0.double(), numer.double(), gram.double(), PLAIN, 6)[0]
            r = worst(report, f"mu gram_of K={K} m={m} x",
                      ratio_to_tol(xb[live], xr[live], TOL_TILED["rtol"], TOL_TILED["atol"]))
            assert r <= 1.0, r


# --------------------------------------------------- B. beta-divergence / KL kernels
def degenerate_beta_problem(K, N, G, seed):
    """beta_problem(3, K, N, G, seed) (X with ~30 % zeros) and then
      W[0, 3] = 0          a dead spectrum: numerator and denominator row are 0
      HT[1, 5] = 0         dead usages
      HT[2, :, 10:14] = 0  cells without usage: P is exactly 0 there while X > 0, so the
                           clamp decides Q
      X[20] = 0, X[:, 7] = 0   an empty cell, an empty gene
      W[2, :, 9] = 0       a gene without loading."""
    X, HT, W = beta_problem(3, K, N, G, seed)
    W[0, 3, :] = 0.0
    HT[1, 5, :] = 0.0
    HT[2, :, 10:14] = 0.0
    X[20] = 0.0
    X[:, 7] = 0.0
    W[2, :, 9] = 0.0
    assert bool((X[10:14] > 0).any(dim=1).all())
    return X, HT, W


def _dev(dev, *ts):
    d = torch.device(dev)
    return [None if t is None else t.float().to(d) for t in ts]


def _h_zeros(h):
    """The exact zeros of the usages of degenerate_beta_problem after any number of
    steps."""
    assert bool((h[0, 3] == 0).all()), "dead spectrum"
    assert bool((h[1, 5] == 0).all()), "dead usages"
    assert bool((h[2, :, 10:14] == 0).all()), "cells without usage"


# K, N, G: K <= 10 / 32 / wide panels (40, 64) / the widest IS panel (56); ragged N and G.
# K = 64 runs beta_any.hip for IS and general beta
H_BLOCK_SHAPES = [(10, 777, 320), (32, 129, 64), (40, 300, 131), (64, 129, 64), (56, 200, 100)]


def check_beta_h_block_degenerate(dev, beta, K, N, G, eps, report=None):
    """One step and five steps of the usage block, rule-free, against float64 at the
    unpenalised test's rtol 5e-5 / atol 1e-6."""
    X, HT, W = degenerate_beta_problem(K, N, G, seed=K + N)
    Xd, Wd = _dev(dev, X, W)
    for nsteps in (1, 5):
        hr = HT.clone()
        reference.beta_h_block(X, hr, W, beta, eps, nsteps, gamma=_gamma(beta))
        hg, = _dev(dev, HT)
        ops.beta_h_block(Xd, hg, Wd, beta, eps, nsteps, gamma=_gamma(beta))
        hg = hg.cpu()
        assert _finite(hg) and _finite(hr)
        _h_zeros(hg)
        _h_zeros(hr)
        r = worst(report, f"h_block beta={beta} K={K} eps={eps} {nsteps} step(s)",
                  ratio_to_tol(hg, hr, 5e-5, 1e-6))
        assert r <= 1.0, r


def h_blocks_ref(X, HT, W, beta, eps, act0, nblocks, nsteps, tol, log=None):
    """test_penalties_cpu.h_blocks_ref, unpenalised, at a given eps."""
    R = HT.shape[0]
    h, act = HT.clone(), act0.clone()
    it, hs = torch.zeros(R, dtype=torch.int32), torch.zeros((R, 2), dtype=torch.float64)
    for blk in range(nblocks):
        live = act.clone()
        f_prev = (reference.beta_contract(0, X, h, W, beta, eps, False, True)[2]
                  if blk == 0 else hs[:, 0].clone())
        reference.beta_h_block(X, h, W, beta, eps, nsteps, gamma=_gamma(beta), act=act, tol=tol,
                               iters=it, conv_mode=1, hstate=hs, loss_entry=blk == 0)
        if log is not None:
            ch = (f_prev - hs[:, 0]).abs() / f_prev.abs()
            log.extend(ch[live != 0].tolist())
    return h, act, it, hs


# Block-objective thresholds of check_beta_h_block_rule_degenerate, live replicates 0 and
# 2.  Relative change of the block objective in float64 over H_BLOCK_SHAPES x BETA_EPSES (see
# the function's docstring for the measured figures).
H_RULE_TOL = {1.0: 0.1, 1.5: 0.1, 0.0: 0.015}


def check_beta_h_block_rule_degenerate(dev, beta, K, N, G, eps, report=None):
    """Four 5-step blocks with the block-objective rule, hstate, act, iters and an
    inactive replicate, at check_beta_h_block_rule's tolerances.  Replicate 2's objective
    carries the clamped entries (IS: 1e13 at eps 1e-10, 1e19 at 1e-16 against 1e5 of the
    rest), so the hstate comparison exercises the loss of clamped products.

    Relative change of the block objective in float64, live replicates 0 and 2, over
    H_BLOCK_SHAPES x BETA_EPSES.  KL: 0.84-0.99 after block 1, 0.003-0.028 after block 2 ->
    tol 0.1; beta 1.5: 0.95-0.998, then 0.006-0.035 -> tol 0.1: every live replicate
    passes its first check and stops at its second.  IS: replicate 0 0.036-0.19 after
    block 1, 0.0023-0.0063 after block 2 -> tol 0.015, stops at its second check;
    replicate 2's objective is the clamped entries' (1.6e12-9.4e12 at eps 1e-10,
    1.6e18-9.4e18 at 1e-16, against 6e4-3e6 for replicate 0) and moves by <= 1.4e-8: it
    stops at its first check.  No change is within a factor 2 of its threshold (asserted),
    so no case runs rule-free."""
    X, HT, W = degenerate_beta_problem(K, N, G, seed=K + N)
    act0 = torch.tensor([1, 0, 1], dtype=torch.int32)
    changes, tol = [], H_RULE_TOL[beta]
    rtol = 1e-3 if beta == 1.0 else 2e-4
    hr, ar, ir, hsr = h_blocks_ref(X, HT, W, beta, eps, act0, 4, 5, tol, log=changes)
    off_threshold(changes, tol, "block objective change")
    d = torch.device(dev)
    Xd, Wd, hg = _dev(dev, X, W, HT)
    ag = act0.to(d)
    ig = torch.zeros(3, dtype=torch.int32, device=d)
    hsg = torch.zeros((3, 2), dtype=torch.float64, device=d)
    for blk in range(4):
        ops.beta_h_block(Xd, hg, Wd, beta, eps, 5, gamma=_gamma(beta), act=ag, tol=tol, iters=ig,
                         conv_mode=1, hstate=hsg, loss_entry=blk == 0)
    hg = hg.cpu()
    assert _finite(hg, hsg.cpu())
    assert bool((hg[0, 3] == 0).all()) and bool((hg[2, :, 10:14] == 0).all())
    worst(report, f"h_block rule beta={beta} K={K} eps={eps} h", ratio_to_tol(hg, hr, rtol, 1e-5))
    worst(report, f"h_block rule beta={beta} K={K} eps={eps} hstate",
          ratio_to_tol(hsg.cpu(), hsr, 1e-4, 1e-6))
    torch.testing.assert_close(hg.double(), hr, rtol=rtol, atol=1e-5)
    assert ag.cpu().tolist() == ar.tolist() and ig.cpu().tolist() == ir.tolist()
    torch.testing.assert_close(hsg.cpu(), hsr, rtol=1e-4, atol=1e-6)
    assert torch.equal(hg[1], HT[1].float())                    # inactive: bit-identical
    return changes


def check_beta_update_h_degenerate(dev, beta, K, eps, N=777, G=260, report=None):
    """Six one-step launches of the fused usage update (beta_mu.hip), rule-free, at
    test_beta_update_h_fused_matches_reference's rtol 1e-4 / atol 1e-5."""
    X, HT, W = degenerate_beta_problem(K, N, G, seed=1)
    Xd, Wd, hg = _dev(dev, X, W, HT)
    hr = HT.clone()
    for _ in range(6):
        reference.beta_update_h(X, hr, W, beta, eps, 0.0, 0.0, _gamma(beta))
        ops.beta_update_h(Xd, hg, Wd, beta, eps, 0.0, 0.0, _gamma(beta))
    hg = hg.cpu()
    assert _finite(hg) and _finite(hr)
    _h_zeros(hg)
    _h_zeros(hr)
    r = worst(report, f"update_h beta={beta} K={K} eps={eps}", ratio_to_tol(hg, hr, 1e-4, 1e-5))
    assert r <= 1.0, r


def check_beta_contract_degenerate(dev, beta, K, eps, N=333, G=131, report=None):
    """ops.beta_contract, both sides, and ops.beta_loss against float64.  Contraction:
    rtol 2e-4 / atol 1e-4, objective rtol 1e-4 / atol 1e-3
    (test_beta_contract_matches_reference); ops.beta_loss: rtol 1e-4 (KL) / 2e-5, atol
    1e-6 (test_split_bf16_beta_kernels_match_fp64)."""
    X, HT, W = degenerate_beta_problem(K, N, G, seed=K)
    Xd, Hd, Wd = _dev(dev, X, HT, W)
    for side in ("h", "w"):
        ref = reference.beta_contract(0 if side == "h" else 1, X, HT, W, beta, eps, True,
                                      side == "h")
        out = ops.beta_contract(side, Xd, Hd, Wd, beta, eps, True, side == "h")
        for i in (0, 1):
            if ref[i] is None:
                assert out[i] is None
                continue
            got = out[i].cpu()
            assert _finite(got)
            r = worst(report, f"contract {side} beta={beta} K={K} eps={eps} {'nd'[i]}",
                      ratio_to_tol(got, ref[i], 2e-4, 1e-4))
            assert r <= 1.0, r
            if side == "h":
                assert bool((got[0, 3] == 0).all())             # W[0, 3] = 0
            else:
                assert bool((got[1, 5] == 0).all())             # HT[1, 5] = 0
                if i == 0:
                    assert bool((got[:, :, 7] == 0).all())      # the empty gene
        if side == "h":
            r = worst(report, f"contract loss beta={beta} K={K} eps={eps}",
                      ratio_to_tol(out[2].cpu(), ref[2], 1e-4, 1e-3))
            assert r <= 1.0, r
            got = ops.beta_loss(Xd, Hd, Wd, beta, eps).cpu()
            r = worst(report, f"beta_loss beta={beta} K={K} eps={eps}",
                      ratio_to_tol(got, ref[2], 1e-4 if beta == 1.0 else 2e-5, 1e-6))
            assert r <= 1.0, r


# iterate-rule threshold of check_beta_w_update_degenerate: see its docstring
W_UPDATE_TOL = 1e-3


def check_beta_w_update_degenerate(dev, beta, eps, report=None):
    """Three anchored online spectra steps from ops.beta_w_partials (construction and
    tolerances of check_beta_w_update), with component 2 of replicate 0 dead in the usages,
    its anchors An and Ad 0 and l1 = l2 = 0: the denominator B is exactly 0, the ``B == 0
    -> eps`` branch runs, and that spectrum becomes exactly 0.  Relative change of the
    spectra per step in float64 (the same at both eps): KL and beta 1.5 0.78-0.80, then
    0.021-0.024 twice; IS 0.52-0.59, 0.28-0.31, 0.16-0.17 -> tol 1e-3 never stops; none
    within a factor 2 of it (asserted)."""
    g = torch.Generator().manual_seed(5)
    R, K, N, G = 4, 7, 500, 333
    gamma, kl, tol = (_gamma(beta) if beta < 1 else 1.0), beta == 1.0, W_UPDATE_TOL
    f = lambda *s, lo=0.0: (torch.rand(s, generator=g, dtype=torch.float64) + lo).float().double()
    X, HT, W = f(N, G, lo=0.05), f(R, K, N, lo=0.1), f(R, K, G, lo=0.1)
    An = f(R, K, G)
    Ad = f(*((R, K) if kl else (R, K, G)), lo=0.5)
    HT[0, 2] = 0.0
    An[0, 2] = 0.0
    Ad[0, 2] = 0.0
    act0 = torch.tensor([1, 0, 1, 1], dtype=torch.int32)
    hsum = HT.sum(dim=2).float().double() if kl else None
    live = [0, 2, 3]
    changes = []
    Wr, anr = W.clone(), torch.zeros_like(W)
    dnr = None if kl else torch.zeros_like(W)
    ar, ir = act0.clone(), torch.zeros(R, dtype=torch.int32)
    d = torch.device(dev)
    Xd, Hd, Wg, hsd, And, Add = _dev(dev, X, HT, W, hsum, An, Ad)
    XT = Xd.t().contiguous()
    ang = torch.zeros((R, K, G), device=d)
    dng = None if kl else torch.zeros((R, K, G), device=d)
    ag, ig = act0.to(d), torch.zeros(R, dtype=torch.int32, device=d)
    for _ in range(3):
        old, was = Wr.clone(), ar.clone()
        nr, dr, _ = reference.beta_contract(1, X, HT, Wr, beta, eps, True, False)
        reference.beta_w_update(Wr, nr.unsqueeze(0), None if kl else dr.unsqueeze(0), hsum, An,
                                Ad, anr, dnr, beta, gamma, 0.0, 0.0, eps, tol, ar, ir)
        ch = (Wr - old).norm(dim=(1, 2)) / old.norm(dim=(1, 2))
        changes.extend(ch[was != 0].tolist())
        ng, dg = ops.beta_w_partials(Xd, XT, Hd, Wg, beta, eps, active=ag, splits=2)
        ops.beta_w_update(Wg, ng, dg, hsd, And, Add, ang, dng, beta, gamma, 0.0, 0.0, eps, tol,
                          ag, ig)
    off_threshold(changes, tol, "spectra change per step")
    Wg, ang = Wg.cpu(), ang.cpu()
    assert _finite(Wg, ang)
    assert bool((Wr[0, 2] == 0).all()) and bool((Wg[0, 2] == 0).all()), "B == 0 -> eps"
    r = worst(report, f"w_update beta={beta} eps={eps} W",
              ratio_to_tol(Wg[live], Wr[live], 1e-4, 1e-5))
    assert r <= 1.0, r
    torch.testing.assert_close(ang.double()[live], anr[live], rtol=1e-4, atol=1e-4)
    assert torch.equal(Wg[1], W[1].float())
    assert ig.cpu().tolist() == ir.tolist() and ag.cpu().tolist() == ar.tolist()
    return changes


def check_kl_fp16_degenerate(dev, K, N, G, eps, report=None):
    """The KL usage block (three steps) and the spectra partials on the degenerate problem,
    to be run with the fp16 numerator selected.  x / eps is 1e10 or 1e16 where P is
    exactly 0 -- beyond fp16, and beyond what a shift of the column can carry without
    losing the column's other terms.  Usages: finite, the exact zeros, and equal to float64
    at test_kl_fp16_numerator_overflow_is_redone_with_a_shift's rtol 5e-3 (atol 1e-6).
    Spectra partials: finite and equal to float64 at that test's rtol 1e-3 / atol 1e-5,
    except in the entries (k, g) with w_kg = 0 whose gene has an element with P = 0 and x >
    0 (beta_planes.h: the fp16 plane drops x / eps there); times W -- what the spectra
    update reads -- they are equal everywhere."""
    X, HT, W = degenerate_beta_problem(K, N, G, seed=K + N)
    Xd, Wd, Hd = _dev(dev, X, W, HT)
    hg, hr = Hd.clone(), HT.clone()
    reference.beta_h_block(X, hr, W, 1.0, eps, 3)
    ops.beta_h_block(Xd, hg, Wd, 1.0, eps, 3)
    hg = hg.cpu()
    assert _finite(hg), "non-finite usages"
    _h_zeros(hg)
    r = worst(report, f"kl fp16 K={K} eps={eps} h", ratio_to_tol(hg, hr, 5e-3, 1e-6))
    assert r <= 1.0, r
    rn = reference.beta_contract(1, X, HT, W, 1.0, eps, True, False)[0]
    num, den = ops.beta_w_partials(Xd, Xd.t().contiguous(), Hd, Wd, 1.0, eps, splits=2)
    got = num.sum(0).cpu().double()
    assert den is None and _finite(got), "non-finite spectra partials"
    P = torch.bmm(HT.transpose(1, 2), W)
    dropped = ((P == 0) & (X > 0)).any(dim=1)                   # (R, G)
    free = (W == 0) & dropped[:, None, :]
    assert bool(free[2, :, 9].all()) and int(free.sum()) == K
    assert bool((got[1, 5] == 0).all()) and bool((got[:, :, 7] == 0).all())
    r = worst(report, f"kl fp16 K={K} eps={eps} w partials",
              ratio_to_tol(got[~free], rn[~free], 1e-3, 1e-5))
    assert r <= 1.0, r
    r = worst(report, f"kl fp16 K={K} eps={eps} W x partials",
              ratio_to_tol(W * got, W * rn, 1e-3, 1e-5))
    assert r <= 1.0, r


# ------------------------------------------------------------------- C. CSR KL kernels
SPARSE_DEGENERATE_CASES = [(10, 333), (32, 1200), (33, 333), (64, 1200), (80, 700), (128, 700)]
SPARSE_ZERO_CELLS = (150, 433)        # inside SPARSE_ROWS
SPARSE_EMPTY_GENE = 5


def degenerate_sparse_problem(K, G):
    """sparse_problem(K, G) (R = 3, N = 901, ~15 % dense, row 7 empty) and then an empty
    gene, W[0, 3] = 0, HT[1, 5] = 0 and two cells of replicate 2 without usage that have
    non-zeros in X."""
    X, HT, W = sparse_problem(K, G)
    X[:, SPARSE_EMPTY_GENE] = 0.0
    W[0, 3, :] = 0.0
    HT[1, 5, :] = 0.0
    for c in SPARSE_ZERO_CELLS:
        assert SPARSE_ROWS[0] <= c < SPARSE_ROWS[1] and int((X[c] > 0).sum()) >= 10
        HT[2, :, c] = 0.0
    return X, HT, W


def dense_kl(dev):
    """The three CSR ops on a device that has the dense ones: what a float32
    implementation of the same sums gives (the CPU stand-in for the CSR kernels)."""
    def h_block(X, a, b, h, W, eps, nsteps, **kw):
        ops.beta_h_block(X[a:b], h, W, 1.0, eps, nsteps, **kw)

    def loss(X, h, W, eps):
        return ops.beta_loss(X, h, W, 1.0, eps)

    def w_num(X, h, W, eps, K):
        return ops.beta_contract("w", X, h, W, 1.0, eps)[0]

    return h_block, loss, w_num


def check_sparse_kl_degenerate(dev, K, G, eps, impl=None, report=None):
    """Three 3-step KL usage blocks with the rule on the row chunk (act, iters, hstate),
    the loss and the spectra numerators against the float64 dense reference, at the
    tolerances of the CSR tests (usages rtol 1e-4 / atol 1e-6, hstate and loss rtol 1e-5 /
    atol 1e-6, numerators rtol 2e-5 / atol 1e-6).  ``impl``: (h_block, loss, w_num) taking
    the dense X (h_block: all of it and the row range).  In float64 the block objective of every replicate changes by 0.89-0.99
    after block 1 and by 0.0017-0.0067 after blocks 2 and 3 (all cases, both eps): tol
    0.05, every replicate stops at its second check, none within a factor 2 of the
    threshold (asserted)."""
    h_block, loss, w_num = impl if impl is not None else dense_kl(dev)
    X, HT, W = degenerate_sparse_problem(K, G)
    a, b = SPARSE_ROWS
    Xc, Hc = X[a:b], HT[:, :, a:b].contiguous()
    act0 = torch.ones(3, dtype=torch.int32)
    changes = []
    hr, ar, ir, hsr = h_blocks_ref(Xc, Hc, W, 1.0, eps, act0, 3, 3, SPARSE_TOL, log=changes)
    off_threshold(changes, SPARSE_TOL, "block objective change")
    d = torch.device(dev)
    Xd, Hd, Wd = _dev(dev, X, HT, W)
    # loss over all rows
    ref_loss = reference.beta_contract(0, X, HT, W, 1.0, eps, False, True)[2]
    got = loss(Xd, Hd, Wd, eps).cpu()
    assert _finite(got)
    r = worst(report, f"sparse loss K={K} G={G} eps={eps}", ratio_to_tol(got, ref_loss, 1e-5, 1e-6))
    assert r <= 1.0, r
    # spectra numerators over the row chunk
    rn = reference.beta_contract(1, Xc, Hc, W, 1.0, eps, True, False)[0]
    hc = Hd[:, :, a:b].contiguous()
    num = w_num(Xd[a:b], hc, Wd, eps, K).cpu()
    assert _finite(num)
    assert bool((num[1, 5] == 0).all()), "dead usages"
    assert bool((num[:, :, SPARSE_EMPTY_GENE] == 0).all()), "empty gene"
    r = worst(report, f"sparse w_num K={K} G={G} eps={eps}", ratio_to_tol(num, rn, 2e-5, 1e-6))
    assert r <= 1.0, r
    # usage blocks with the rule
    h, act = hc.clone(), act0.to(d)
    it = torch.zeros(3, dtype=torch.int32, device=d)
    hs = torch.zeros((3, 2), dtype=torch.float64, device=d)
    for blk in range(3):
        h_block(Xd, a, b, h, Wd, eps, 3, act=act, tol=SPARSE_TOL, iters=it, hstate=hs,
                loss_entry=blk == 0)
    h = h.cpu()
    assert _finite(h, hs.cpu())
    za = [c - a for c in SPARSE_ZERO_CELLS]
    for x in (h, hr):
        assert bool((x[0, 3] == 0).all()) and bool((x[1, 5] == 0).all())
        assert bool((x[2][:, za] == 0).all())
    r = worst(report, f"sparse h_block K={K} G={G} eps={eps} h", ratio_to_tol(h, hr, 1e-4, 1e-6))
    assert r <= 1.0, r
    assert act.cpu().tolist() == ar.tolist() and it.cpu().tolist() == ir.tolist()
    r = worst(report, f"sparse h_block K={K} G={G} eps={eps} hstate",
              ratio_to_tol(hs.cpu(), hsr, 1e-5, 1e-6))
    assert r <= 1.0, r
    return changes


# ------------------------------------------- D. the solver from an init with exact zeros
# route -> (options, err tolerance against the CPU run, MU route)
NNDSVD_ROUTES = {
    "mu-online": (dict(algo="mu", mode="online"), 1e-3, True),
    "mu-batch": (dict(algo="mu", mode="batch"), 1e-3, True),
    "hals-online": (dict(algo="hals", mode="online"), 3e-3, False),
    "kl-online": (dict(algo="mu", mode="online", beta_loss="kullback-leibler"), 2e-2, True),
    # IS: the project's KL figure
    "is-online": (dict(algo="mu", mode="online", beta_loss="itakura-saito"), 2e-2, True),
}
NNDSVD_SEEDS = [11, 12]
SPARSE_PATTERN = {6: "equal", 40: "kept"}       # run_from_nndsvd: on sparse_counts()


def sparse_counts(n=1500, g=300, density=0.15, seed=3):
    """The ~15 %-dense matrix of test_online_kl_wide_sparse_path_matches_dense."""
    from cnmf_torch_amd.utils.synthetic import normalized_counts_matrix

    X = normalized_counts_matrix(n, g, n_programs=8, seed=seed)
    X[X < np.quantile(X, 1.0 - density)] = 0.0
    return X


def run_from_nndsvd(X, K, dev, **opts):
    """run_nmf_batch from init="nndsvd" on ``dev`` (natively on a GPU: an eager fallback
    warns, which is an error here): finite outputs, and on the MU routes the zero pattern
    of the spectra is exactly that of the init evaluated on the same device -- >= 40 % of
    the entries.  ``pattern="kept"`` asserts only what MU guarantees on any input: a zero
    of the init is a zero of the result.  (On sparse_counts() at K = 40 the float32 CPU
    run itself ends with 24 more zeros than the init: spectra entries whose numerator is
    exactly 0 because no cell with a count in that gene uses the component, or that
    underflow.)"""
    from cnmf_torch_amd.models.nmf import run_nmf_batch
    from cnmf_torch_amd.models.nmf_base import init_factors

    kw = dict(dict(online_chunk_size=700, online_max_pass=5, batch_max_iter=40), **opts)
    mu, pattern = kw.pop("mu_route"), kw.pop("pattern", "equal")
    with warnings.catch_warnings():
        if torch.device(dev).type == "cuda":
            warnings.simplefilter("error", RuntimeWarning)
        res = run_nmf_batch(X, K, NNDSVD_SEEDS, device=dev, init="nndsvd", **kw)
    W, HT = res.W.cpu().numpy(), res.HT.cpu().numpy()
    assert np.isfinite(W).all() and np.isfinite(HT).all() and np.isfinite(res.err).all()
    if mu:
        Xd = torch.as_tensor(np.asarray(X)).to(dev)
        W0 = init_factors(Xd, K, NNDSVD_SEEDS, init="nndsvd")[1].cpu().numpy()
        frac = float((W0 == 0).mean())
        print(f"K={K} {opts}: {frac:.3f} of the initial spectra are exact zeros")
        assert frac >= 0.4, frac
        assert bool((W[W0 == 0] == 0).all()), "a zero of the init was revived"
        if pattern == "equal":
            assert np.array_equal(W == 0, W0 == 0), int(((W == 0) != (W0 == 0)).sum())
    return res


# --------------------------------------------------- the checks on the float32 reference
@pytest.mark.parametrize("pens", DEGENERATE_SETS)
@pytest.mark.parametrize("algo,K", [("mu", 3), ("mu", 10), ("mu", 40), ("mu", 96),
                                    ("hals", 3), ("hals", 10), ("hals", 40)])
def test_solve_degenerate_float32_reference(algo, K, pens):
    """Parts 1-3 hold for the float32 reference at the kernels' tolerances, with every
    exact claim (n = 777; K = 96 at the wide kernels' tolerance)."""
    check_solve_degenerate("cpu", algo, K, 777, pens, TOL_WMFMA if K > 64 else TOL_TILED)


def test_solve_degenerate_float32_reference_objective_rule_fixed_steps():
    """The fixed steps under the objective rule with tol = -1 (the pipelined kernel's
    case): the all-zero replicates stop at their second zero check, 0 <= -0."""
    x0, numer, gram = degenerate_solve_problem(10, 777, seed=10)
    ir = ref_solve("mu", x0, numer, gram, PLAIN, 6, -1.0, 1, 2)[3]
    assert ir.tolist() == [6, 6, 4, 2, 6]
    check_solve_degenerate("cpu", "mu", 10, 777, PLAIN, conv_modes=(1,))


@pytest.mark.parametrize("pens", DEGENERATE_SETS)
def test_solve_degenerate_float32_reference_sliced_sizes(pens):
    check_solve_degenerate("cpu", "mu", 10, 2600, pens)
    check_solve_degenerate_nsplit("cpu", 10, 2600, pens)


def test_solve_degenerate_float32_reference_padded_and_gram_of():
    check_solve_degenerate_padded("cpu")
    check_solve_degenerate_gram_of("cpu")


@pytest.mark.parametrize("eps", BETA_EPSES)
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("K,N,G", [s for s in H_BLOCK_SHAPES if s[0] in (10, 40)])
def test_beta_h_block_degenerate_float32_reference(beta, K, N, G, eps):
    check_beta_h_block_degenerate("cpu", beta, K, N, G, eps)
    check_beta_h_block_rule_degenerate("cpu", beta, K, N, G, eps)


@pytest.mark.parametrize("eps", BETA_EPSES)
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("K,N,G", [s for s in H_BLOCK_SHAPES if s[0] not in (10, 40)])
def test_beta_h_block_rule_thresholds_are_off_the_float64_decisions(beta, K, N, G, eps):
    """The remaining shapes: the float64 decisions alone (off_threshold)."""
    X, HT, W = degenerate_beta_problem(K, N, G, seed=K + N)
    changes = []
    h_blocks_ref(X, HT, W, beta, eps, torch.tensor([1, 0, 1], dtype=torch.int32), 4, 5,
                 H_RULE_TOL[beta], log=changes)
    off_threshold(changes, H_RULE_TOL[beta], "block objective change")


@pytest.mark.parametrize("eps", BETA_EPSES)
@pytest.mark.parametrize("beta", BETAS)
def test_beta_ops_degenerate_float32_reference(beta, eps):
    check_beta_update_h_degenerate("cpu", beta, 10, eps)
    check_beta_contract_degenerate("cpu", beta, 10, eps)
    check_beta_w_update_degenerate("cpu", beta, eps)
    if beta == 1.0:
        check_kl_fp16_degenerate("cpu", 10, 777, 320, eps)


@pytest.mark.parametrize("eps", BETA_EPSES)
@pytest.mark.parametrize("K,G", SPARSE_DEGENERATE_CASES)
def test_sparse_kl_degenerate_inputs_and_float32_reference(K, G, eps):
    """The CSR kernels use eps + P where the reference clamps, max(P, eps): the two differ
    by eps / P relative, so every P of these inputs must be exactly 0 or >= 1e-3 (1e-7 at
    eps 1e-10, below float32 rounding of the quotient).  The checks themselves run on the
    dense float32 reference here (the CSR ops have no CPU path)."""
    X, HT, W = degenerate_sparse_problem(K, G)
    P = torch.bmm(HT.transpose(1, 2), W)
    assert bool(((P == 0) | (P >= 1e-3)).all())
    assert int((P == 0).sum()) == len(SPARSE_ZERO_CELLS) * G
    check_sparse_kl_degenerate("cpu", K, G, eps)


@pytest.mark.parametrize("route,K", [("mu-online", 6), ("mu-online", 40), ("mu-batch", 6),
                                     ("hals-online", 6), ("kl-online", 6), ("is-online", 6)])
def test_solver_from_nndsvd_cpu(route, K):
    opts, _, mu = NNDSVD_ROUTES[route]
    run_from_nndsvd(gamma_counts(), K, "cpu", mu_route=mu, **opts)


@pytest.mark.parametrize("K", [6, 40])
def test_solver_from_nndsvd_sparse_counts_cpu(K):
    """The matrix of the CSR route (dense on the CPU)."""
    opts, _, mu = NNDSVD_ROUTES["kl-online"]
    run_from_nndsvd(sparse_counts(), K, "cpu", mu_route=mu, pattern=SPARSE_PATTERN[K], **opts)
