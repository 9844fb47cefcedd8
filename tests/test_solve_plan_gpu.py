"""ops.solve_plan, the one place that picks the kernel of the fused inner solve: the rules
of docs/ARCHITECTURE.md ("Solve dispatch") as invariants over a grid of solves, the named
cases the penalty tests rely on, and the launcher's side of the contract (cnmf_solve runs
the kernel it is told to, or fails).  Needs the extension's geometry queries; the only
launch attempted is rejected on the host."""
import itertools

import pytest
import torch

from cnmf_torch_amd import ops

pytestmark = pytest.mark.gpu

RESIDENT = 240      # co-residency budget passed to every plan: 256 CUs less the margin
KS = [3, 10, 16, 17, 20, 32, 37, 40, 64, 80, 96, 128, 130]
GRID = list(itertools.product(["mu", "hals"], KS, [300, 777, 2600, 20000], [1, 3, 100], [1, 3],
                              [0, 1], [False, True], ["auto", "stream", "reg", "mfma"],
                              ["auto", 1, 3]))
VALU = ("wide", "resident", "stream")


@pytest.fixture
def env(monkeypatch):
    """Sets CNMF_SOLVE_* knobs; the device's budget is RESIDENT for pipe_slices."""
    key = torch.cuda.current_device()
    ops._coop_resident(torch.device("cuda", key))
    monkeypatch.setitem(ops._COOP_RESIDENT, key, RESIDENT)

    def set_(**kw):
        for k in ("CNMF_SOLVE_PIPE", "CNMF_SOLVE_COOP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            monkeypatch.setenv("CNMF_SOLVE_" + k, str(v))
        ops.refresh_env()
    set_()
    yield set_
    monkeypatch.undo()
    ops.refresh_env()


def _plan(algo, K, n, nblocks, **kw):
    return ops.solve_plan(algo, K, n, nblocks, resident=RESIDENT, **kw)


def _check(case, plan):
    """The invariants of the dispatch table for one planned solve."""
    algo, K, n, nblocks, nsplit, conv_mode, penalised, variant, coop = case
    h = ops._hip
    kernel, S, rpl, threads = plan
    assert kernel in {"any", *h.SOLVE_KERNEL_IDS}, case
    mu = algo == "mu"
    assert (kernel == "any") == ops.solve_any_k(ops.ALGOS[algo], K), case
    if kernel == "any":
        assert plan == ("any", 1, 0, 0) and variant != "mfma", case
        return
    per = -(-n // S)
    assert S == nsplit if nsplit > 1 else (1 <= S <= ops.kCoopMaxSlices), case
    if nsplit == 1 and coop != "auto":
        assert S == coop, case
    pipe_takes = (mu and not penalised and conv_mode == 1 and nsplit == 1
                  and ops._ENV["CNMF_SOLVE_PIPE"] != "0" and h.solve_pipe_tiles(K, per) > 0)
    if kernel == "pipe":
        assert pipe_takes and variant in ("auto", "mfma"), case
    if kernel == "mfma":
        assert mu and variant in ("auto", "mfma") and not pipe_takes, case
        assert per <= h.solve_mfma_max_cols(K), case
    if variant == "mfma":
        assert kernel in ("pipe", "mfma"), case
    if variant in ("stream", "reg"):
        assert kernel not in ("pipe", "mfma"), case
    assert (rpl == 0) if kernel != "pipe" else (rpl == 0 or 0 < rpl < nblocks), case
    if S > 1 and nsplit == 1:       # cooperating workgroups are all resident at once
        per_cu = {"pipe": h.solve_pipe_wg_per_cu(K), "mfma": ops.MFMA_WG_PER_CU}.get(kernel, 1)
        assert S * min(nblocks, rpl or nblocks) <= per_cu * RESIDENT, case
    assert (kernel == "wide") == (32 < K <= 64 and kernel != "pipe"), case
    assert (kernel in ("wmfma_bf16", "wmfma_f32")) == (K > 64), case
    if K > 64:
        assert mu and (kernel == "wmfma_bf16") == (variant != "stream" and K % 32 == 0), case
    if kernel in ("resident", "stream"):
        assert K <= 32, case
        fits = per <= h.solve_reg_max_cols(K)
        assert (kernel == "resident") == (variant == "reg" or (variant == "auto" and fits)), case
    if kernel in VALU:
        assert 64 <= threads <= h.solve_max_threads(K) and threads % 64 == 0, case
    else:
        assert threads == 0, case


def _sweep():
    """Plans the grid; returns {case: plan} for the combinations some kernel takes."""
    out = {}
    for case in GRID:
        algo, K, n, nblocks, nsplit, conv_mode, penalised, variant, coop = case
        try:
            plan = _plan(algo, K, n, nblocks, nsplit=nsplit, conv_mode=conv_mode,
                         penalised=penalised, variant=variant, coop=coop)
        except ValueError:
            continue
        _check(case, plan)
        out[case] = plan
    return out


def test_solve_plan_grid_invariants(env):
    """Every combination plans a known kernel or raises ValueError; the table's rules hold;
    ops.pipe_slices is the plan's slice count; every kernel is reached."""
    plans = _sweep()
    assert {p.kernel for p in plans.values()} == {"any", *ops._hip.SOLVE_KERNEL_IDS}
    assert 0.5 * len(GRID) < len(plans) < len(GRID)
    dev = torch.device("cuda", torch.cuda.current_device())
    for (algo, K, n, nblocks, nsplit, conv_mode, penalised, variant, coop), plan in plans.items():
        if (algo, nsplit, conv_mode, penalised, variant, coop) == ("mu", 1, 1, False, "auto", "auto"):
            assert ops.pipe_slices(n, nblocks, K, dev) == (
                plan.slices if plan.kernel == "pipe" else None), (K, n, nblocks, plan)
    # the errors are those of combinations no kernel takes
    for bad in (dict(variant="mfma"), dict(fused=True)):
        with pytest.raises(ValueError):
            _plan("mu", 40, 777, 3, conv_mode=1, penalised=True, **bad)
    with pytest.raises(ValueError, match="rank-general"):
        _plan("mu", 37, 777, 3, variant="mfma")
    with pytest.raises(ValueError, match="co-resident"):
        _plan("hals", 10, 2600, 100, coop=3)
    with pytest.raises(ValueError):
        _plan("mu", 10, 777, 3, variant="fastest")


def test_solve_plan_env_knobs(env):
    """CNMF_SOLVE_PIPE=0 never plans the pipelined kernel (the solves it took run
    solve_mfma.hip or a VALU kernel); CNMF_SOLVE_COOP=0 never splits a replicate on its own
    (an explicit ``coop`` and ``nsplit`` are the caller's)."""
    base = _sweep()
    env(PIPE=0)
    off = _sweep()
    assert "pipe" not in {p.kernel for p in off.values()}
    for case, plan in base.items():
        if plan.kernel != "pipe":
            assert off[case] == plan, case
        elif case in off:
            assert off[case].kernel in ("mfma", *VALU), case
        if plan.kernel == "pipe" and case[1] <= 16 and not plan.reps_per_launch:
            assert off[case] == ("mfma", plan.slices, 0, 0), case    # the same slices
    env(COOP=0)
    for case, plan in _sweep().items():
        if case[4] == 1 and case[8] == "auto":
            assert plan.slices == 1, (case, plan)


def test_solve_plan_named_cases(env):
    """The solves tests/test_penalties_gpu.py names its kernels by (three replicates)."""
    pen = dict(penalised=True)
    assert _plan("mu", 10, 777, 3, **pen).kernel == "mfma"
    assert _plan("mu", 10, 777, 3, conv_mode=1).kernel == "pipe"
    assert _plan("mu", 10, 2600, 3, coop=3, **pen)[:2] == ("resident", 3)
    assert _plan("hals", 10, 2600, 3, coop=3, **pen)[:2] == ("resident", 3)
    assert _plan("mu", 10, 2600, 3, coop=4, **pen)[:2] == ("mfma", 4)
    for algo in ("mu", "hals"):
        assert _plan(algo, 40, 777, 3, **pen).kernel == "wide"
    assert _plan("mu", 96, 777, 3, **pen).kernel == "wmfma_bf16"
    assert _plan("mu", 80, 777, 3, **pen).kernel == "wmfma_f32"
    assert _plan("mu", 96, 777, 3, variant="stream", **pen).kernel == "wmfma_f32"
    assert _plan("mu", 37, 777, 3, **pen).kernel == "any"
    assert _plan("hals", 80, 777, 3, **pen).kernel == "any"
    assert _plan("mu", 10, 2100, 3, nsplit=3, **pen)[:2] == ("mfma", 3)
    assert _plan("mu", 10, 2600, 3, nsplit=3, **pen)[:2] == ("resident", 3)
    assert _plan("mu", 10, 777, 3, gram_of=True, conv_mode=1).kernel == "mfma"
    assert _plan("mu", 20, 777, 3, gram_of=True, conv_mode=1).kernel == "pipe"


def test_launcher_obeys_the_plan():
    """cnmf_solve told to run solve_mfma.hip at K = 20, outside that kernel's ranks, fails
    on the host -- it does not pick another kernel -- and x is untouched."""
    R, K, n = 3, 20, 64
    g = torch.Generator().manual_seed(0)
    x = (torch.rand((R, K, n), generator=g) + 0.1).cuda()
    numer = torch.rand((R, K, n), generator=g).cuda()
    gram = (torch.eye(K) + 0.1).repeat(R, 1, 1).cuda()
    x0 = x.clone()
    h = ops._hip
    assert h.solve_mfma_max_cols(K) == 0 and _plan("mu", K, n, R).kernel == "resident"

    def launch(kernel):
        h.solve(0, K, x.data_ptr(), x.stride(0), x.stride(1), numer.data_ptr(), numer.stride(0),
                numer.stride(1), gram.data_ptr(), K * K, 0, R, n, 3, -1.0, 0.0, 0.0, 0.0, 1e-16,
                0, 0, 0, 1, 0, 5, 64, h.SOLVE_KERNEL_IDS[kernel], 0, 1, 0, 0, 0, 0,
                0, 0, 0, 0, 0, 0, 0,                       # planes
                0, 0, 0, 0,                                # gram_of
                1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,     # fused operands
                0, 0, 0, 0, ops._stream_ptr(x))
    with pytest.raises(RuntimeError, match="cnmf_solve"):
        launch("mfma")
    torch.cuda.synchronize()
    assert torch.equal(x, x0)
