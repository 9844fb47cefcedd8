"""The pipelined MU solve's fixed-cost paths (csrc/kernels/solve_pipe.h): the initial
objective folded into sweep 0, the four-value cooperative exchange (solve_core.h
coop_sum4_tag_s) whose totals a converged solve reuses for lin / quad, and the publish-only
epilogue exchange of a solve stopped by max_iter -- bit for bit against solve_mfma.hip
(K <= 16), against the float64 reference and the explicitly reduced operands (K > 16),
under HIP-graph replay with the device-side generation, and with inactive replicates."""
import pytest
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.ops import reference

pytestmark = pytest.mark.gpu


def _problem(R, K, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    W = torch.rand((R, K, 96), generator=g, dtype=torch.float64) + 0.05
    gram = torch.bmm(W, W.transpose(1, 2))
    x_true = torch.rand((R, K, n), generator=g, dtype=torch.float64)
    numer = torch.bmm(gram, x_true) * (1 + 0.05 * torch.rand((R, K, n), generator=g,
                                                             dtype=torch.float64))
    x0 = torch.rand((R, K, n), generator=g, dtype=torch.float64) + 0.1
    return x0.float(), numer.float(), gram.float()


def _run(x0, numer_d, gram_d, R, **kw):
    dev = numer_d.device
    xg = x0.clone().to(dev)
    lin = torch.full((R,), 7.0, device=dev)
    quad = torch.full((R,), 7.0, device=dev)
    it = torch.zeros(R, dtype=torch.int32, device=dev)
    S = ops.solve("mu", xg, numer_d, gram_d, lin_out=lin, quad_out=quad, iters_out=it,
                  conv_mode=1, **kw)
    return S, (xg.cpu(), lin.cpu(), quad.cpu(), it.cpu())


# (slices, columns): one workgroup, two slices, and the exchange's lane layouts -- 4 S =
# 64 granules (one per lane), 68 (the first past one per lane) and 128 (every lane two)
# -- on whole tiles and with a ragged last tile and one short slice
_SLICES = [(1, 40), (2, 200), (16, 2048), (17, 2048), (32, 2048), (16, 2041), (17, 2041),
           (32, 2041)]
STOP_FIRST, NEVER = 1e30, -1.0


@pytest.mark.parametrize("K", [3, 10, 16])
@pytest.mark.parametrize("S,n", _SLICES)
def test_solve_pipe_stops_and_exchanges_bitwise_equal_mfma(monkeypatch, K, S, n):
    """x, lin, quad and the iteration counts equal solve_mfma_kernel's bit for bit for
    every way a solve ends: max_iter 0 (the it = 0 check is exchanged, nothing deferred),
    a stop at the first real check (lin / quad come from that check's exchange), a check
    that falls on it == max_iter, and a stop by max_iter between checks (one more product
    and the publish-only epilogue exchange)."""
    R = 3
    x0, numer, gram = _problem(R, K, n, seed=900 + 7 * K + S)
    dev = torch.device("cuda")
    numer_d, gram_d = numer.to(dev), gram.to(dev)
    cases = [(every, mi, tol) for every in (1, 10) for mi in (0, 1, 7, 10, 25)
             for tol in (STOP_FIRST, NEVER)]
    out = {}
    for pipe in ("1", "0"):
        monkeypatch.setenv("CNMF_SOLVE_PIPE", pipe)
        ops.refresh_env()
        assert ops.solve_plan("mu", K, n, R, conv_mode=1, coop=S, device=dev).kernel == (
            "pipe" if pipe == "1" else "mfma")
        for every, mi, tol in cases:
            got, res = _run(x0, numer_d, gram_d, R, max_iter=mi, tol=tol, check_every=every,
                            coop=S)
            assert got == S
            out[pipe, every, mi, tol] = res
    monkeypatch.delenv("CNMF_SOLVE_PIPE")
    ops.refresh_env()
    ops.coop_check(dev)
    for every, mi, tol in cases:
        a, b = out["1", every, mi, tol], out["0", every, mi, tol]
        for name, u, v in zip(("x", "lin", "quad", "iters"), a, b):
            assert torch.equal(u, v), (name, every, mi, tol)
        # the iteration count the stop rule gives: the first check past it = 0, or max_iter
        first = every if every <= mi else mi
        assert a[3].tolist() == [first if tol == STOP_FIRST else mi] * R, (every, mi, tol)


@pytest.mark.parametrize("K", [20, 32, 48, 64])
def test_solve_pipe_wide_k_float64_and_fused_operands_bitwise(K):
    """K > 16 (no solve_mfma oracle): fixed steps equal the float64 reference solve in x,
    lin and quad (the tolerances of test_solve_pipe_wide_k_matches_reference), and the
    fused operands -- 1, 2 or 4 raw slabs, with and without scale + base in / out, 1, 9 or
    20 partial Grams (more than one staging chunk) -- reproduce the explicitly reduced
    operands bit for bit in x, lin, quad and the iteration counts, for a solve that
    converges at a check and one that max_iter stops."""
    R, n = 3, 700
    x0, numer, gram = _problem(R, K, n, seed=600 + K)
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(K)
    # fixed steps against float64
    S, (xm, lm, qm, im) = _run(x0, numer.to(dev), gram.to(dev), R, max_iter=6, tol=-1.0,
                               check_every=4)
    assert S > 1 and ops.solve_plan("mu", K, n, R, conv_mode=1, device=dev).kernel == "pipe"
    xr = x0.clone().double()
    lr = torch.zeros(R, dtype=torch.float64)
    qr = torch.zeros(R, dtype=torch.float64)
    reference.solve(0, xr, numer.double(), gram.double(), None, 6, -1.0, 0.0, 0.0, 0.0, 1e-16,
                    lr, qr, None, 1, 1, 4)
    assert im.tolist() == [6] * R
    torch.testing.assert_close(xm.double(), xr, rtol=3e-4, atol=1e-5)
    torch.testing.assert_close(lm.double(), lr, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(qm.double(), qr, rtol=1e-4, atol=1e-3)
    # fused operands against the reduce path
    slabs = (torch.rand((4, R, K, n), generator=g) * numer.unsqueeze(0) / 4).to(dev)
    scale = (torch.rand(n, generator=g) + 0.5).to(dev)
    base = (torch.rand((R, K, n), generator=g) * numer.mean()).to(dev)
    parts = (torch.rand((R, 20, K, K), generator=g) * gram.unsqueeze(1) / 20).to(dev)
    gbase = (gram * 0.5).to(dev)
    flat = slabs.reshape(-1)
    for ns in (1, 2, 4):
        for extras in (False, True):
            for npart in (1, 9, 20):
                nref = slabs[0].clone()
                for q in range(1, ns):
                    nref = nref + slabs[q]
                if extras:
                    nref = base + nref * scale
                t = parts[:, 0].clone()
                for q in range(1, npart):
                    t = t + parts[:, q]
                gref = gbase + t
                nout = torch.zeros_like(nref) if extras else None
                gout = torch.zeros_like(gref)
                for kw in (dict(max_iter=300, tol=1e-3, check_every=5),
                           dict(max_iter=7, tol=-1.0, check_every=5)):
                    S1, plain = _run(x0, nref, gref, R, **kw)
                    S2, fused = _run(
                        x0, flat[:R * K * n].view(R, K, n), gbase, R, numer_slabs=ns,
                        numer_slab_stride=R * K * n, numer_scale=scale if extras else None,
                        numer_base=base if extras else None, numer_out=nout,
                        gram_parts=parts, gram_parts_n=npart, gram_out=gout, **kw)
                    assert S1 == S2 and S2 > 1
                    for name, u, v in zip(("x", "lin", "quad", "iters"), plain, fused):
                        assert torch.equal(u, v), (name, ns, extras, npart, kw)
                    assert torch.equal(gout, gref)
                    if extras:
                        assert torch.equal(nout, nref)
    ops.coop_check(dev)


def test_solve_pipe_graph_replay_device_generation_bitwise_eager():
    """K = 10 in 17 slices (68 granules per exchange) tagged from the device-side
    generation: two eager launches agree bit for bit, and three replays of the captured
    launch reproduce them -- each replay's exchanges carry a fresh tag, the four-value
    slots of the previous one are never mistaken for arrivals."""
    R, K, n, S = 3, 10, 2041, 17
    x0, numer, gram = _problem(R, K, n, seed=41)
    dev = torch.device("cuda")
    numer_d, gram_d = numer.to(dev), gram.to(dev)
    kw = dict(max_iter=200, tol=1e-4, check_every=10, coop=S, coop_device_gen=True)
    _, eager = _run(x0, numer_d, gram_d, R, **kw)
    _, again = _run(x0, numer_d, gram_d, R, **kw)
    for u, v in zip(eager, again):
        assert torch.equal(u, v)
    assert (eager[3] > 0).all()
    xs = x0.clone().to(dev)
    lin = torch.zeros(R, device=dev)
    quad = torch.zeros(R, device=dev)
    it = torch.zeros(R, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)
    ops.coop_reserve(dev, side.cuda_stream, R, 200, 10)
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            ops.solve("mu", xs, numer_d, gram_d, lin_out=lin, quad_out=quad, iters_out=it,
                      conv_mode=1, **kw)
        finally:
            graph.capture_end()
    torch.cuda.current_stream(dev).wait_stream(side)
    for _ in range(3):
        xs.copy_(x0)
        it.zero_()
        lin.fill_(7.0)
        quad.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(eager, (xs, lin, quad, it)):
            assert torch.equal(u, v.cpu())
    ops.coop_check(dev)


@pytest.mark.parametrize("K,S,n", [(10, 17, 2041), (20, 5, 1300)])
def test_solve_pipe_inactive_and_rep_index_second_launch_completes(K, S, n):
    """Replicates that are inactive or not in rep_index keep x, lin, quad and their
    iteration counts; every workgroup (theirs and the padding of the last group of 8
    included) still arrives, so the last one resets the arrival counter and advances the
    device-side generation by one per launch -- and a second launch completes and
    repeats the first bit for bit."""
    R = 6
    x0, numer, gram = _problem(R, K, n, seed=70 + K)
    dev = torch.device("cuda")
    numer_d, gram_d = numer.to(dev), gram.to(dev)
    active = torch.tensor([1, 1, 0, 1, 1, 1], dtype=torch.int32, device=dev)
    ri = torch.tensor([0, 2, 3, 5], dtype=torch.int32, device=dev)
    kw = dict(max_iter=200, tol=1e-4, check_every=10, coop=S, coop_device_gen=True,
              rep_index=ri, active=active)
    _run(x0, numer_d, gram_d, R, **kw)           # (allocates the workspace)
    ws = ops._COOP_WS[str(numer_d.device), torch.cuda.current_stream(dev).cuda_stream]
    gen0 = int(ws["gen_dev"].item()) & 0xFFFFFFFF
    rounds = -(-4 // (ops.solve_plan("mu", K, n, 4, conv_mode=1, coop=S,
                                     device=dev).reps_per_launch or 4))
    _, first = _run(x0, numer_d, gram_d, R, **kw)
    _, second = _run(x0, numer_d, gram_d, R, **kw)
    ops.coop_check(dev)
    assert int(ws["arrive"].item()) == 0
    assert (int(ws["gen_dev"].item()) & 0xFFFFFFFF) == gen0 + 2 * rounds
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    xg, lin, quad, it = first
    for r in (1, 2, 4):
        assert torch.equal(xg[r], x0[r]) and it[r].item() == 0
        assert lin[r].item() == 7.0 and quad[r].item() == 7.0
    for r in (0, 3, 5):
        assert it[r].item() > 0 and not torch.equal(xg[r], x0[r])
