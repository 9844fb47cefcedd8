"""l1 / l2 penalties at sizes a test can see.

Every op here is compared with its float64 reference under penalties large enough that
dropping, misplacing or mis-signing any one of them moves the result by >= 20x the
comparison tolerance (``visible``).  The checks are written once, against a device: this
file runs them on the CPU, where ``ops`` evaluates ``ops/reference.py`` in float32 (the
same formulas in the kernels' precision, so the tolerances and the input conditions are
confirmed without a GPU); ``test_penalties_gpu.py`` runs the same checks on the HIP
kernels.  The solver's one-step oracle at the end needs no device at all.
"""
import numpy as np
import pytest
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.ops import reference

EPS = 1e-16
BETA_EPS = 1e-10
GUARD = 20.0

# (l1_num, l1_den, l2): the full set and one term at a time (a sign or placement error in
# one term cannot cancel against another)
P_FULL = (10.0, 5.0, 10.0)
SOLVE_SETS = [P_FULL, (10.0, 0.0, 0.0), (0.0, 5.0, 0.0), (0.0, 0.0, 10.0)]
# (l1, l2) of the beta-divergence updates
BETA_SETS = [(20.0, 40.0), (20.0, 0.0), (0.0, 40.0)]

# x tolerance (rtol, atol; atol < 0: that fraction of max |x|), lin / quad rtol
TOL_TILED = dict(rtol=2e-4, atol=1e-4, lq=1e-3)     # test_solve_matches_reference
TOL_WMFMA = dict(rtol=2e-3, atol=1e-4, lq=2e-3)     # test_solve_wmfma_matches_fp64_reference
TOL_ANY = dict(rtol=2e-3, atol=-2e-5, lq=1e-4)      # test_solve_any_rank_matches_float64_reference


def scaled(pens, s):
    return tuple(float(s) * p for p in pens)


# ------------------------------------------------------------------------- the guard
def visible(run, pens, rtol, atol, factor=GUARD, report=None):
    """Condition on the inputs: ``run(*pens)`` (float64 reference; a tensor or a tuple
    whose first entry is compared) must move by >= ``factor`` x the comparison tolerance
    when any single non-zero penalty term is set to 0, as max |d| / (rtol |x| + atol).
    Returns the full-penalty result; ``report`` (a list) collects the ratios."""
    full = run(*pens)
    x = full[0] if isinstance(full, tuple) else full
    a = atol if atol >= 0 else -atol * float(x.abs().max())
    assert any(p != 0 for p in pens)
    for i, p in enumerate(pens):
        if p == 0:
            continue
        alt = run(*[0.0 if j == i else q for j, q in enumerate(pens)])
        y = alt[0] if isinstance(alt, tuple) else alt
        ratio = float(((y - x).abs() / (rtol * x.abs() + a)).max())
        if report is not None:
            report.append(ratio)
        assert ratio >= factor, (f"penalty term {i} of {pens} is invisible: moves the "
                                 f"reference by {ratio:.1f}x the tolerance (< {factor})")
    return full


def ratio_to_tol(got, ref, rtol, atol):
    return float(((got.double() - ref).abs() / (rtol * ref.abs() + atol)).max())


# ------------------------------------------------------------------------- A. solve
def solve_problem(R, K, n, seed):
    """tests/test_kernels_gpu.py ``_problem`` in float64: Gram diagonal ~25, numerators
    30 ... 640."""
    g = torch.Generator().manual_seed(seed)
    W = torch.rand((R, K, 64), generator=g, dtype=torch.float64) + 0.05
    gram = torch.bmm(W, W.transpose(1, 2))
    x_true = torch.rand((R, K, n), generator=g, dtype=torch.float64)
    numer = torch.bmm(gram, x_true) * (1 + 0.05 * torch.rand((R, K, n), generator=g,
                                                             dtype=torch.float64))
    x0 = torch.rand((R, K, n), generator=g, dtype=torch.float64) + 0.1
    # the kernels see float32 operands: the reference gets exactly those values
    return x0.float().double(), numer.float().double(), gram.float().double()


def ref_solve(algo, x0, numer, gram, pens, max_iter, tol=-1.0, conv_mode=0, check_every=5,
              nsplit=1):
    R = x0.shape[0]
    x = x0.clone()
    lin, quad = torch.zeros(R, dtype=torch.float64), torch.zeros(R, dtype=torch.float64)
    it = torch.zeros(R, dtype=torch.int32)
    reference.solve(ops.ALGOS[algo], x, numer, gram, None, max_iter, tol, pens[0], pens[1],
                    pens[2], EPS, lin, quad, it, nsplit, conv_mode, check_every)
    return x, lin, quad, it


class DevSolve:
    """``ops.solve`` in float32 on ``dev`` for one problem (operands uploaded once)."""

    def __init__(self, dev, algo, x0, numer, gram, **kw):
        self.dev, self.algo, self.kw = torch.device(dev), algo, kw
        self.x0 = x0.float()
        self.numer, self.gram = numer.float().to(self.dev), gram.float().to(self.dev)

    def __call__(self, pens, max_iter, tol=-1.0, conv_mode=0, check_every=5, **kw):
        R = self.x0.shape[0]
        x = self.x0.clone().to(self.dev)
        lin, quad = torch.zeros(R, device=self.dev), torch.zeros(R, device=self.dev)
        it = torch.zeros(R, dtype=torch.int32, device=self.dev)
        ops.solve(self.algo, x, self.numer, self.gram, max_iter=max_iter, tol=tol,
                  l1_num=pens[0], l1_den=pens[1], l2=pens[2], eps=EPS, lin_out=lin,
                  quad_out=quad, iters_out=it, conv_mode=conv_mode, check_every=check_every,
                  **{**self.kw, **kw})
        return x.cpu(), lin.cpu().double(), quad.cpu().double(), it.cpu()


def penalised_objective(x, numer, gram, pens):
    """1/2 sum x^T G x - sum x . max(numer - l1_num, 0) + l1_den sum |x| + 1/2 l2 sum x^2
    per replicate, float64, written out from the definition (not reference._objective)."""
    l1n, l1d, l2 = pens
    x = x.double()
    nb = torch.clamp(numer - l1n, min=0.0)
    return (0.5 * (x * torch.bmm(gram, x)).sum(dim=(1, 2)) - (x * nb).sum(dim=(1, 2))
            + l1d * x.abs().sum(dim=(1, 2)) + 0.5 * l2 * (x * x).sum(dim=(1, 2)))


def _atol(t, xr):
    return t["atol"] if t["atol"] >= 0 else -t["atol"] * float(xr.abs().max())


def check_solve_fixed(run, algo, prob, pens, t=TOL_TILED, steps=6, nsplit=1, **kw):
    """Part 1: ``steps`` fixed steps -- x, lin (from the RAW numerator), quad, step counts
    against float64, behind the visibility guard.  Returns the device's x."""
    x0, numer, gram = prob
    xr, lr, qr, ir = visible(
        lambda *p: ref_solve(algo, x0, numer, gram, p, steps, nsplit=nsplit), pens,
        t["rtol"], t["atol"])
    if nsplit > 1:
        kw = dict(kw, nsplit=nsplit)
    xg, lg, qg, ig = run(pens, steps, **kw)
    assert ig.tolist() == ir.tolist() == [steps] * x0.shape[0]
    r = ratio_to_tol(xg, xr, t["rtol"], _atol(t, xr))
    print(f"{algo} K={x0.shape[1]} {pens}: x at {r:.3f} of its tolerance")
    assert r <= 1.0, r
    if pens[0] > 0:
        # <max(numer - l1_num, 0), x> is a different number at this tolerance (1.5 % off at
        # K = 64, more below): lin really is checked against the raw numerator
        shifted = (torch.clamp(numer - pens[0], min=0.0) * xr).sum(dim=(1, 2))
        assert float(((shifted - lr).abs() / lr.abs()).min()) > 10 * t["lq"]
    torch.testing.assert_close(lg, lr, rtol=t["lq"], atol=1e-3)
    torch.testing.assert_close(qg, qr, rtol=t["lq"], atol=1e-3)
    return xg


def check_solve_converged(run, algo, prob, pens, **kw):
    """Part 2: max_iter 60, tol 1e-3, check_every 5 under both stop rules: step counts
    within 1 (iterate rule) / one check interval (objective rule), x within 5e-3."""
    x0, numer, gram = prob
    for conv_mode in (0, 1):
        xr, _, _, ir = ref_solve(algo, x0, numer, gram, pens, 60, 1e-3, conv_mode, 5)
        xg, _, _, ig = run(pens, 60, tol=1e-3, conv_mode=conv_mode, check_every=5, **kw)
        slack = 1 if conv_mode == 0 else 5
        assert int((ig - ir).abs().max()) <= slack, (conv_mode, ig.tolist(), ir.tolist())
        d = float((xg.double() - xr).norm() / xr.norm())
        assert d < 5e-3, (conv_mode, d)


def check_solve_monotone(run, prob, pens, **kw):
    """Part 3: the penalised objective of the device's iterate after m = 0 ... 6 steps
    (seven launches from the same x0), evaluated in float64 from its definition, never
    rises by more than 1e-5 |f|.  The float64 reference is monotone to 1e-9; the 1e-5 allows
    for float32 iterates and holds for the float32 reference in every case of this file."""
    x0, numer, gram = prob
    f = torch.stack([penalised_objective(run(pens, m, **kw)[0], numer, gram, pens)
                     for m in range(7)])
    assert torch.equal(run(pens, 0, **kw)[0], x0.float())       # a 0-step launch moves nothing
    rise = (f[1:] - f[:-1]) / f[:-1].abs()
    assert float(rise.max()) <= 1e-5, rise.max(dim=1).values.tolist()
    assert bool((f[-1] < f[0]).all())


def check_solve_case(dev, algo, K, n, sets=SOLVE_SETS, scale=1.0, t=TOL_TILED, R=3, **kw):
    """Parts 1-3 for every penalty set; returns {pens: device x after the fixed steps}."""
    prob = solve_problem(R, K, n, seed=K)
    run = DevSolve(dev, algo, *prob, **kw)
    out = {}
    for pens in sets:
        pens = scaled(pens, scale)
        out[pens] = check_solve_fixed(run, algo, prob, pens, t)
        check_solve_converged(run, algo, prob, pens)
        check_solve_monotone(run, prob, pens)
    return out


def check_solve_nsplit(dev, K, n=2600, R=3):
    """One fixed step with the columns split over three blocks: lin / quad are summed by
    atomics.  Every ``ops.solve`` call made here must carry nsplit = 3."""
    prob = solve_problem(R, K, n, seed=K)
    run = DevSolve(dev, "mu", *prob)
    seen, real = [], ops.solve

    def spy(*a, **kw):
        seen.append(kw.get("nsplit"))
        return real(*a, **kw)

    ops.solve = spy
    try:
        for pens in SOLVE_SETS:
            check_solve_fixed(run, "mu", prob, pens, steps=1, nsplit=3)
    finally:
        ops.solve = real
    assert seen == [3] * len(SOLVE_SETS), seen


def check_solve_clamp(dev, algo, K, n=777, R=3, **kw):
    """l1_num at the 25th percentile of the numerator: a quarter of the entries clamp to
    0.  MU gives exact zeros there; HALS has the reference's zero pattern, except where
    the float64 value is below atol."""
    prob = solve_problem(R, K, n, seed=K)
    x0, numer, gram = prob
    l1n = float(torch.quantile(numer.float().flatten()[:1 << 20], 0.25))   # a float32 value
    pens = (l1n, P_FULL[1], P_FULL[2])
    xr = ref_solve(algo, x0, numer, gram, pens, 6)[0]
    clamped = (numer - l1n) <= 0
    assert 0.2 < float(clamped.double().mean()) < 0.3
    xg = check_solve_fixed(DevSolve(dev, algo, *prob, **kw), algo, prob, pens)
    if algo == "mu":
        assert bool((xr[clamped] == 0).all())
        assert bool((xg[clamped] == 0).all())
        assert bool((xg[~clamped] > 0).all())
    else:
        assert 0.01 < float((xr == 0).double().mean())         # the pattern is not trivial
        differ = (xg == 0) != (xr == 0)
        assert bool((xr[differ] < TOL_TILED["atol"]).all()), int(differ.sum())
        assert float(differ.double().mean()) < 1e-3
    return xg


def check_solve_padded(dev, K=37, Kp=40, n=777, R=3):
    """A rank-37 MU solve run as the engine runs it, zero-padded to 40 (chunked_solve,
    native_rank): the padding rows stay exactly 0 under every penalty set, the others
    equal the float64 reference of the unpadded problem."""
    x0, numer, gram = solve_problem(R, K, n, seed=K)
    xp, npad = torch.zeros((R, Kp, n), dtype=torch.float64), torch.zeros((R, Kp, n),
                                                                          dtype=torch.float64)
    gp = torch.zeros((R, Kp, Kp), dtype=torch.float64)
    xp[:, :K], npad[:, :K], gp[:, :K, :K] = x0, numer, gram
    run = DevSolve(dev, "mu", xp, npad, gp)
    for pens in SOLVE_SETS:
        xr = visible(lambda *p: ref_solve("mu", x0, numer, gram, p, 6)[0], pens,
                     TOL_TILED["rtol"], TOL_TILED["atol"])
        xg = run(pens, 6)[0]
        assert bool((xg[:, K:] == 0).all())
        assert ratio_to_tol(xg[:, :K], xr, TOL_TILED["rtol"], TOL_TILED["atol"]) <= 1.0


# --------------------------------------------------- B. beta-divergence / KL kernels
def beta_problem(R, K, N, G, seed, zeros=True, lo=0.0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand((N, G), generator=g, dtype=torch.float64) + lo
    if zeros:
        X[X < 0.3] = 0.0
    HT = torch.rand((R, K, N), generator=g, dtype=torch.float64) + 0.05
    W = torch.rand((R, K, G), generator=g, dtype=torch.float64) + 0.05
    return X.float().double(), HT.float().double(), W.float().double()


def _gamma(beta):
    return 1.0 if beta else 0.5


def off_threshold(values, tol, what):
    """No stop decision within a factor 2 of its threshold (float64 reference)."""
    v = np.asarray(values, dtype=np.float64)
    assert not ((v > tol / 2) & (v < 2 * tol)).any(), (what, tol, v.tolist())


# iterate-rule thresholds of check_beta_update_h.  Relative change per step in float64 at
# K = 10 / 40 under the three penalty sets: beta 1: 0.86-0.97, then 0.14-0.18 (none under
# (20, 0)), then <= 0.026 -> 0.06 stops at step 2 or 3; beta 1.5: 0.85-0.96, then
# 0.047-0.135 -> 0.3 stops at step 2; beta 0 halves every step down to 0.019-0.031 at step
# 6 -> 0.009 never stops.  No change is within a factor 2 of its threshold.
UPDATE_H_TOL = {1.0: 0.06, 1.5: 0.3, 0.0: 0.009}


def check_beta_update_h(dev, beta, K, pens, N=777, G=260):
    """Six one-step launches of the fused usage update with the iterate stop rule and an
    inactive replicate (construction and tolerance of
    test_beta_update_h_fused_matches_reference: X = rand, rtol 1e-4 / atol 1e-5).
    Thresholds UPDATE_H_TOL, against the relative change per step measured in float64 at
    K = 10 / 40 under the three penalty sets: beta 1: 0.86-0.97, then 0.14-0.18 (none
    under (20, 0)), then <= 0.026 -> tol 0.06 stops at step 2 or 3; beta 1.5: 0.85-0.96,
    then 0.047-0.135 -> tol 0.3 stops at step 2; beta 0: halves every step down to
    0.019-0.031 at step 6 -> tol 0.009 never stops.  No change is within a factor 2 of its
    threshold (asserted)."""
    R, tol = 3, UPDATE_H_TOL[beta]
    X, HT, W = beta_problem(R, K, N, G, seed=1, zeros=False)
    act0 = torch.tensor([1, 1, 0], dtype=torch.int32)
    changes = []

    def ref(l1, l2, log=None):
        h, act, it = HT.clone(), act0.clone(), torch.zeros(R, dtype=torch.int32)
        for _ in range(6):
            old, live = h.clone(), act.clone()
            reference.beta_update_h(X, h, W, beta, BETA_EPS, l1, l2, _gamma(beta), act, tol, it)
            if log is not None:
                ch = (h - old).norm(dim=(1, 2)) / old.norm(dim=(1, 2))
                log.extend(ch[live != 0].tolist())
        return h, act, it

    visible(ref, pens, 1e-4, 1e-5)
    hr, ar, ir = ref(*pens, log=changes)
    off_threshold(changes, tol, "iterate change per step")
    d = torch.device(dev)
    Xd, Wd = X.float().to(d), W.float().to(d)
    hg, ag, ig = HT.float().to(d), act0.to(d), torch.zeros(R, dtype=torch.int32, device=d)
    for _ in range(6):
        ops.beta_update_h(Xd, hg, Wd, beta, BETA_EPS, pens[0], pens[1], _gamma(beta), ag, tol, ig)
    torch.testing.assert_close(hg.cpu().double(), hr, rtol=1e-4, atol=1e-5)
    assert ag.cpu().tolist() == ar.tolist() and ig.cpu().tolist() == ir.tolist()
    assert torch.equal(hg[2].cpu(), HT[2].float())             # inactive: bit-identical
    return changes


# beta, K, N, G: shapes of test_split_bf16_beta_kernels(_wide_k)_match_fp64
H_BLOCK_CASES = [(1.0, 10, 777, 320), (0.0, 10, 777, 320), (1.5, 10, 777, 320),
                 (1.0, 32, 129, 64), (0.0, 32, 129, 64), (1.5, 32, 129, 64),
                 (1.0, 40, 300, 131), (1.0, 64, 129, 64), (0.0, 56, 200, 100)]
# block-objective thresholds of check_beta_h_block_rule.  Relative change of the block
# objective in float64 over these nine cases x three penalty sets: KL and beta 1.5: 0.90-0.99
# after block 1, 0.005-0.025 after block 2 -> 0.1; IS: 0.06-0.20 after block 1, 0.002-0.004
# after block 2 -> 0.015.  Every replicate passes its first check and stops at its second;
# no change is within a factor 2 of its threshold.
H_BLOCK_TOL = {1.0: 0.1, 1.5: 0.1, 0.0: 0.015}


def check_beta_h_block_step(dev, beta, K, N, G, pens):
    """One rule-free step of the split-bf16 usage block against float64 (rtol 5e-5 / atol
    1e-6, the unpenalised test's)."""
    X, HT, W = beta_problem(3, K, N, G, seed=K + N)
    hr = visible(lambda l1, l2: _h_block_ref(X, HT, W, beta, 1, l1, l2), pens, 5e-5, 1e-6)
    d = torch.device(dev)
    hg = HT.float().to(d)
    ops.beta_h_block(X.float().to(d), hg, W.float().to(d), beta, BETA_EPS, 1, pens[0], pens[1],
                     gamma=_gamma(beta))
    torch.testing.assert_close(hg.cpu().double(), hr, rtol=5e-5, atol=1e-6)


def _h_block_ref(X, HT, W, beta, nsteps, l1, l2):
    h = HT.clone()
    reference.beta_h_block(X, h, W, beta, BETA_EPS, nsteps, l1, l2, gamma=_gamma(beta))
    return h


def h_blocks_ref(X, HT, W, beta, pens, act0, nblocks, nsteps, tol, log=None):
    """``nblocks`` blocks of ``nsteps`` steps with the block-objective rule (entry
    objective on the first) in float64; ``log`` collects every live replicate's relative
    objective change per block."""
    R = HT.shape[0]
    h, act = HT.clone(), act0.clone()
    it, hs = torch.zeros(R, dtype=torch.int32), torch.zeros((R, 2), dtype=torch.float64)
    for blk in range(nblocks):
        live = act.clone()
        f_prev = (reference.beta_contract(0, X, h, W, beta, BETA_EPS, False, True)[2]
                  if blk == 0 else hs[:, 0].clone())
        reference.beta_h_block(X, h, W, beta, BETA_EPS, nsteps, pens[0], pens[1],
                               gamma=_gamma(beta), act=act, tol=tol, iters=it, conv_mode=1,
                               hstate=hs, loss_entry=blk == 0)
        if log is not None:
            ch = (f_prev - hs[:, 0]).abs() / f_prev.abs()
            log.extend(ch[live != 0].tolist())
    return h, act, it, hs


def check_beta_h_block_rule(dev, beta, K, N, G, pens):
    """Four 5-step blocks with the block-objective rule: iterate, flags, step counts and
    objective state (tolerances of test_split_bf16_h_block_rule_matches_reference).  The
    block objective is the beta-divergence alone -- no penalty term, as the reference
    defines it.  Thresholds H_BLOCK_TOL, against the relative change of the block objective
    measured in float64 over H_BLOCK_CASES x BETA_SETS: KL and beta 1.5: 0.90-0.99 after
    block 1, 0.005-0.025 after block 2 -> tol 0.1; IS: 0.06-0.20 after block 1, 0.002-0.004
    after block 2 -> tol 0.015.  Every live replicate passes its first check and stops at
    its second; no change is within a factor 2 of its threshold (asserted)."""
    X, HT, W = beta_problem(3, K, N, G, seed=K + N)
    act0 = torch.tensor([1, 0, 1], dtype=torch.int32)
    changes, tol = [], H_BLOCK_TOL[beta]
    rtol = 1e-3 if beta == 1.0 else 2e-4
    visible(lambda l1, l2: h_blocks_ref(X, HT, W, beta, (l1, l2), act0, 4, 5, tol)[0], pens,
            rtol, 1e-5)
    hr, ar, ir, hsr = h_blocks_ref(X, HT, W, beta, pens, act0, 4, 5, tol, log=changes)
    off_threshold(changes, tol, "block objective change")
    d = torch.device(dev)
    Xd, Wd = X.float().to(d), W.float().to(d)
    hg, ag = HT.float().to(d), act0.to(d)
    ig = torch.zeros(3, dtype=torch.int32, device=d)
    hsg = torch.zeros((3, 2), dtype=torch.float64, device=d)
    for blk in range(4):
        ops.beta_h_block(Xd, hg, Wd, beta, BETA_EPS, 5, pens[0], pens[1], gamma=_gamma(beta),
                         act=ag, tol=tol, iters=ig, conv_mode=1, hstate=hsg,
                         loss_entry=blk == 0)
    torch.testing.assert_close(hg.cpu().double(), hr, rtol=rtol, atol=1e-5)
    assert ag.cpu().tolist() == ar.tolist() and ig.cpu().tolist() == ir.tolist()
    torch.testing.assert_close(hsg.cpu(), hsr, rtol=1e-4, atol=1e-6)
    assert torch.equal(hg[1].cpu(), HT[1].float())             # inactive: bit-identical
    return changes


SPARSE_CASES = [(10, 333), (32, 1200), (33, 333), (64, 333), (64, 1200)]
SPARSE_ROWS = (100, 700)         # the row chunk of tests/test_sparse_kl_wide_gpu.py
SPARSE_TOL = 0.05


def sparse_problem(K, G):
    """``_problem`` of tests/test_sparse_kl_wide_gpu.py: R = 3, N = 901, X ~15 % dense with
    row 7 empty, seed = K."""
    g = torch.Generator().manual_seed(K)
    R, N = 3, 901
    X = torch.rand((N, G), generator=g, dtype=torch.float64)
    X[X < 0.85] = 0.0
    X[7] = 0.0
    HT = torch.rand((R, K, N), generator=g, dtype=torch.float64) + 0.05
    W = torch.rand((R, K, G), generator=g, dtype=torch.float64) + 0.05
    return X.float().double(), HT.float().double(), W.float().double()


def sparse_kl_reference(K, G, pens, act0, tol=SPARSE_TOL):
    """float64 expectation of three 3-step KL usage blocks with the rule on the row chunk,
    behind the guard; also the relative block-objective changes."""
    X, HT, W = sparse_problem(K, G)
    a, b = SPARSE_ROWS
    Xc, Hc = X[a:b], HT[:, :, a:b].contiguous()
    changes = []
    visible(lambda l1, l2: h_blocks_ref(Xc, Hc, W, 1.0, (l1, l2), act0, 3, 3, tol)[0], pens,
            1e-4, 1e-6)
    out = h_blocks_ref(Xc, Hc, W, 1.0, pens, act0, 3, 3, tol, log=changes)
    off_threshold(changes, tol, "block objective change")
    return (X, HT, W), out, changes


def check_beta_w_update(dev, beta, pens, tol=1e-3):
    """Three anchored online spectra steps (construction and tolerances of
    test_beta_w_update_matches_reference)."""
    g = torch.Generator().manual_seed(5)
    R, K, N, G = 4, 7, 500, 333
    gamma, kl = _gamma(beta) if beta < 1 else 1.0, beta == 1.0
    f = lambda *s, lo=0.0: (torch.rand(s, generator=g, dtype=torch.float64) + lo).float().double()
    X, HT, W = f(N, G, lo=0.05), f(R, K, N, lo=0.1), f(R, K, G, lo=0.1)
    An = f(R, K, G)
    Ad = f(*((R, K) if kl else (R, K, G)), lo=0.5)
    act0 = torch.tensor([1, 0, 1, 1], dtype=torch.int32)
    hsum = HT.sum(dim=2).float().double() if kl else None
    live = [0, 2, 3]
    changes = []

    def ref(l1, l2, log=None):
        Wr, an = W.clone(), torch.zeros_like(W)
        dn = None if kl else torch.zeros_like(W)
        act, it = act0.clone(), torch.zeros(R, dtype=torch.int32)
        for _ in range(3):
            old, was = Wr.clone(), act.clone()
            nr, dr, _ = reference.beta_contract(1, X, HT, Wr, beta, BETA_EPS, True, False)
            reference.beta_w_update(Wr, nr.unsqueeze(0), None if kl else dr.unsqueeze(0), hsum,
                                    An, Ad, an, dn, beta, gamma, l1, l2, BETA_EPS, tol, act, it)
            if log is not None:
                ch = (Wr - old).norm(dim=(1, 2)) / old.norm(dim=(1, 2))
                log.extend(ch[was != 0].tolist())
        return Wr[live], an[live], act, it

    visible(ref, pens, 1e-4, 1e-5)
    Wr, anr, ar, ir = ref(*pens, log=changes)
    off_threshold(changes, tol, "spectra change per step")
    d = torch.device(dev)
    up = lambda t_: None if t_ is None else t_.float().to(d)
    Wg, ang = up(W), torch.zeros((R, K, G), device=d)
    dng = None if kl else torch.zeros((R, K, G), device=d)
    ag, ig = act0.to(d), torch.zeros(R, dtype=torch.int32, device=d)
    for _ in range(3):
        ng, dg, _ = ops.beta_contract("w", up(X), up(HT), Wg, beta, BETA_EPS, active=ag,
                                      reduce=False)
        ops.beta_w_update(Wg, ng, dg, up(hsum), up(An), up(Ad), ang, dng, beta, gamma, pens[0],
                          pens[1], BETA_EPS, tol, ag, ig)
    torch.testing.assert_close(Wg.cpu().double()[live], Wr, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(ang.cpu().double()[live], anr, rtol=1e-4, atol=1e-4)
    assert torch.equal(Wg[1].cpu(), W[1].float())
    assert ig.cpu().tolist() == ir.tolist() and ag.cpu().tolist() == ar.tolist()


# --------------------------------------------------- the checks on the float32 reference
@pytest.mark.parametrize("algo", ["mu", "hals"])
@pytest.mark.parametrize("K", [3, 10, 17, 40])
def test_solve_float32_reference_meets_the_kernel_checks(algo, K):
    """Parts 1-3 of the solve checks hold for the float32 reference with the kernels'
    tolerances, so they are conditions the HIP kernels can meet; the guard passes at
    >= 20x for P = (10, 5, 10) and each single term (6 fixed steps, n = 777).  The single
    terms run at K <= 10 only here (HALS in torch is a loop over components)."""
    check_solve_case("cpu", algo, K, 777, sets=SOLVE_SETS if K <= 10 else [P_FULL])


@pytest.mark.parametrize("K,scale,t", [(80, 4.0, TOL_WMFMA), (96, 4.0, TOL_WMFMA)])
def test_solve_float32_reference_wide_rank_penalties_are_visible(K, scale, t):
    """K > 64 at the wide kernels' 2e-3 tolerance: P = (10, 5, 10) is not visible there;
    4 P = (40, 20, 40) is (guard ratios in test_penalties_gpu.py)."""
    prob = solve_problem(3, K, 777, seed=K)
    run = DevSolve("cpu", "mu", *prob)
    for pens in SOLVE_SETS:
        check_solve_fixed(run, "mu", prob, scaled(pens, scale), t)
    check_solve_monotone(run, prob, scaled(P_FULL, scale))


@pytest.mark.parametrize("algo", ["mu", "hals"])
@pytest.mark.parametrize("K", [10, 40])
def test_solve_float32_reference_numerator_clamp(algo, K):
    check_solve_clamp("cpu", algo, K)


def test_solve_float32_reference_padded_rank():
    check_solve_padded("cpu")


def test_solve_float32_reference_column_split():
    check_solve_nsplit("cpu", 10, n=999)


@pytest.mark.parametrize("beta", [1.0, 0.0, 1.5])
@pytest.mark.parametrize("pens", BETA_SETS)
def test_beta_update_h_float32_reference(beta, pens):
    check_beta_update_h("cpu", beta, 10, pens)


@pytest.mark.parametrize("beta,K,N,G", [c for c in H_BLOCK_CASES if c[1] in (10, 64)])
@pytest.mark.parametrize("pens", BETA_SETS)
def test_beta_h_block_float32_reference(beta, K, N, G, pens):
    check_beta_h_block_step("cpu", beta, K, N, G, pens)
    check_beta_h_block_rule("cpu", beta, K, N, G, pens)


@pytest.mark.parametrize("K,G", SPARSE_CASES)
@pytest.mark.parametrize("pens", BETA_SETS)
def test_sparse_kl_block_inputs_are_visible_and_off_threshold(K, G, pens):
    """The inputs of the CSR usage-block test (GPU only: the op has no CPU path) meet the
    guard, and no float64 stop decision is near tol."""
    sparse_kl_reference(K, G, pens, torch.ones(3, dtype=torch.int32))


@pytest.mark.parametrize("beta", [1.0, 0.0, 1.5])
@pytest.mark.parametrize("pens", BETA_SETS)
def test_beta_w_update_float32_reference(beta, pens):
    check_beta_w_update("cpu", beta, pens)


# ------------------------------------------------------------- C1. the solver, one step
def gamma_counts(N=1500, G=400, K=6):
    """The matrix of test_nmf_batch_gpu_matches_cpu."""
    rs = np.random.default_rng(0)
    return (rs.gamma(1, 1, (N, K)) @ rs.gamma(0.5, 1, (K, G)) + 0.1 * rs.random((N, G))).astype(
        np.float32)


def _mu(x, numer, gram, l1, l2):
    den = gram @ x + l2 * x + l1
    return np.where(den < EPS, 0.0, x * numer / np.where(den < EPS, 1.0, den))


def _hals(x, numer, gram, l1, l2):
    x = x.copy()
    for k in range(x.shape[0]):
        if gram[k, k] + l2 > EPS:
            x[k] = np.maximum(x[k] + (numer[k] - l1 - gram[k] @ x - l2 * x[k]) / (gram[k, k] + l2),
                              0.0)
    return x


def one_step(X, HT, W, kind, l1h, l2h, l1w, l2w):
    """One batch iteration in float64 numpy: the usages from the old spectra, then the
    spectra from the new usages; l1 in the denominator (HALS: off the numerator) and
    l2 x beside it, as NMFOptions.l1_H ... l2_W define them."""
    if kind == "kl":
        Q = X / np.maximum(HT.T @ W, EPS)
        d = W.sum(1, keepdims=True) + l1h + l2h * HT
        HT = HT * (W @ Q.T) / np.where(d == 0, EPS, d)
        Q = X / np.maximum(HT.T @ W, EPS)
        d = HT.sum(1, keepdims=True) + l1w + l2w * W
        return HT, W * (HT @ Q) / np.where(d == 0, EPS, d)
    upd = _mu if kind == "mu" else _hals
    HT = upd(HT, W @ X.T, W @ W.T, l1h, l2h)
    return HT, upd(W, HT @ X, HT @ HT.T, l1w, l2w)


def full_objective(X, HT, W, kind, l1h, l2h, l1w, l2w):
    P = HT.T @ W
    if kind == "kl":
        Pc = np.maximum(P, EPS)
        fit = (np.where(X > 0, X * np.log(np.where(X > 0, X, 1.0) / Pc), 0.0) - X + Pc).sum()
    else:
        fit = 0.5 * ((X - P) ** 2).sum()
    return (fit + l1h * np.abs(HT).sum() + 0.5 * l2h * (HT ** 2).sum()
            + l1w * np.abs(W).sum() + 0.5 * l2w * (W ** 2).sum())


@pytest.mark.parametrize("l1_ratio", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("kind", ["mu", "hals", "kl"])
def test_batch_solver_iteration_is_the_penalised_update(kind, l1_ratio):
    """run_nmf_batch (batch mode, float64, alpha_H = alpha_W = 10) after m + 1 iterations ==
    one penalised step, written out in numpy, from its factors after m iterations, m = 1
    ... 4, to 1e-9; and the penalised objective never rises.  The reported ``err`` is the
    reconstruction error alone (docs/COVERAGE.md C19)."""
    from cnmf_torch_amd.models.nmf import run_nmf_batch

    X, K, seeds, alpha = gamma_counts(), 6, [11, 12], 10.0
    pens = (alpha * l1_ratio, alpha * (1 - l1_ratio)) * 2
    kw = dict(algo="hals" if kind == "hals" else "mu", mode="batch",
              beta_loss="kullback-leibler" if kind == "kl" else "frobenius",
              fp_precision="double", loss_every=1, tol=-1e30, alpha_H=alpha, alpha_W=alpha,
              l1_ratio_H=l1_ratio, l1_ratio_W=l1_ratio)
    runs = []
    for m in range(1, 6):
        res = run_nmf_batch(X, K, seeds, device="cpu", batch_max_iter=m, **kw)
        assert res.n_iter.tolist() == [m] * len(seeds)
        runs.append((res.HT.numpy().reshape(len(seeds), K, -1),
                     res.W.numpy().reshape(len(seeds), K, -1), res.err))
    Xd = X.astype(np.float64)
    for r in range(len(seeds)):
        f = [full_objective(Xd, HT[r], W[r], kind, *pens) for HT, W, _ in runs]
        assert all(b <= a * (1 + 1e-12) for a, b in zip(f, f[1:])), f
        for (HT, W, _), (HT1, W1, err1) in zip(runs, runs[1:]):
            h, w = one_step(Xd, HT[r], W[r], kind, *pens)
            np.testing.assert_allclose(HT1[r], h, rtol=1e-9, atol=1e-300)
            np.testing.assert_allclose(W1[r], w, rtol=1e-9, atol=1e-300)
            if kind != "kl":
                # err^2 = |X|^2 - 2 lin + quad with lin / quad kept in float32 (2^-24 each
                # on sums ~20x err^2): 1e-4 is far above that and far below the penalty
                # terms, which are 3 % ... 22 % of err^2 in these runs
                np.testing.assert_allclose(err1[r], np.linalg.norm(Xd - HT1[r].T @ W1[r]),
                                           rtol=1e-4)
                pen = full_objective(Xd, HT1[r], W1[r], kind, *pens) - 0.5 * err1[r] ** 2
                assert pen > 0.02 * err1[r] ** 2
