"""The Harmony kernels (harmony.hip) against plain float64 torch on the host, at the ranks,
wave counts and loop trip counts production reaches.

``run_harmony`` takes min(round(N / 30), 100) clusters, so real data runs K = 100: lanes
that own two clusters, a centroid kernel whose waves own one or two cluster tiles, and --
with many batch levels -- block kernels of 3, 2 or 1 waves.  Every case below runs the
remove step, the assign step (distances formed in the kernel, and read from a matrix) and
the round objective, each compared with the host formula of ``Harmony._update_R`` for one
block, never GPU against GPU.  ``sigma`` differs per cluster and ``theta`` per level, so a
transposed table or a wrong index cannot pass; ``sigma[0] = 0.002`` drives part of the new
R to denormals and exact zeros (the entropy guard), ``theta[0] = 0`` is the flat penalty.

Bounds: rtol 1e-10 with atol 1e-13 (R) and 1e-12 (everything else), those of
test_harmony_fused_round_matches_float64_reference.  The float64 sums here have at most
9000 terms; summing the cells of the host reference below in another (random) order moved
E1 and O1 by at most 3.6e-15 over all cases (9e-16 after the full cancellation of the
``maxkb`` case), so the bounds leave the kernels' own summation order ample room and a
wrong term none.
"""
import functools

import numpy as np
import pytest
import torch

from cnmf_torch_amd import ops

pytestmark = pytest.mark.gpu

RTOL = 1e-10
ATOL_R = 1e-13
ATOL = 1e-12
# O1 = O - R Phi^T and E1 of ``maxkb`` (every cell removed) are differences of equal numbers
# of size ~2 and come out near 0, where a relative bound means nothing; 1e-10 absolute is
# 5e-11 of the numbers subtracted.  After the remove step only.
ATOL_CANCEL = 1e-10

# id: K, levels per covariate, d, N, nb, (waves of the fused-distance variant, of the
# distT variant).  nb = 2077: 130 workgroups of 16 cells, three ragged trips of the
# reduce loop; 9000: chunk = 18, and every cell removed first (O1 ~ 0, Pen ~ 1); 17: a
# second workgroup with one cell; 1: three idle waves.
CASES = {
    "prod": (100, (3, 2), 50, 3000, 2077, (4, 4)),
    "maxkb": (128, (32,), 64, 9000, 9000, (1, 3)),
    "mid": (100, (16, 14), 50, 3000, 2077, (2, 4)),
    "k65": (65, (2, 2, 3), 1, 500, 17, (4, 4)),
    "k64": (64, (2,), 8, 500, 1, (4, 4)),
    "k48": (48, (4, 5), 33, 1500, 1041, (4, 4)),
    "k1": (1, (1,), 3, 40, 40, (4, 4)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the host float64 reference of one block update (computed once per case;
    the tests only read it)."""
    K, levels, d, N, nb, _ = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    f64 = torch.float64
    Z = torch.randn((d, N), generator=g, dtype=f64)
    Zc = Z / torch.linalg.vector_norm(Z, dim=0)
    Y = Zc[:, torch.randperm(N, generator=g)[:K]].contiguous()       # distances over [0, 4)
    R = torch.rand((K, N), generator=g, dtype=f64)
    R = R / R.sum(dim=0)
    labels = [torch.randint(0, b, (N,), generator=g) for b in levels]
    Phi = torch.cat([torch.nn.functional.one_hot(l, b).t().to(f64)
                     for l, b in zip(labels, levels)])
    offs = np.concatenate([[0], np.cumsum(levels)[:-1]])
    bidx = torch.stack([l + int(o) for l, o in zip(labels, offs)]).to(torch.int32)
    B = Phi.shape[0]
    sigma = 0.05 + 0.15 * torch.rand(K, generator=g, dtype=f64)
    sigma[0] = 0.002
    theta = 2 * torch.rand(B, generator=g, dtype=f64)
    theta[0] = 0.0
    Pr_b = Phi.sum(dim=1) / N
    E = torch.outer(R.sum(dim=1), Pr_b)
    O = R @ Phi.t()
    cells = torch.randperm(N, generator=g)[:nb]                        # no repeats
    dist = 2 * (1 - Y.t() @ Zc)
    # the host branch of Harmony._update_R for this block
    Rb, Pb = R[:, cells], Phi[:, cells]
    E1 = E - torch.outer(Rb.sum(dim=1), Pr_b)
    O1 = O - Rb @ Pb.t()
    Pen = ((E1 + 1) / (O1 + 1)) ** theta[None, :]
    sd = -dist[:, cells] / sigma[:, None]
    sd = sd - sd.max(dim=0).values
    Rn = torch.exp(sd) * (Pen @ Pb)
    Rn = Rn / Rn.abs().sum(dim=0)
    E2 = E1 + torch.outer(Rn.sum(dim=1), Pr_b)
    O2 = O1 + Rn @ Pb.t()
    km = (Rn * dist[:, cells]).sum()
    ent = (sigma[:, None] * torch.where(Rn > 0, Rn * torch.log(Rn), torch.zeros((), dtype=f64))
           ).sum()
    cross = (sigma[:, None] * theta[None, :] * O2 * torch.log((O2 + 1) / (E2 + 1))).sum()
    return dict(K=K, B=B, d=d, N=N, nb=nb, Zt=Zc.t().contiguous(), Y=Y,
                Rt=R.t().contiguous(), bidx=bidx.contiguous(), sigma=sigma, theta=theta,
                Pr_b=Pr_b, E=E, O=O, cells=cells, distT=dist.t().contiguous(), E1=E1, O1=O1,
                Pen=Pen, Rn=Rn, E2=E2, O2=O2, km=km, ent=ent, cross=cross)


def _run_block(c, fused, with_obj=True):
    """Step 0, then step 1 on that state, on the GPU from the case's inputs; a fresh
    workspace.  Returns the host copies after each step."""
    dev = torch.device("cuda")
    Rt, E, O = c["Rt"].to(dev), c["E"].to(dev), c["O"].to(dev)
    obj = torch.tensor([0.25, -0.5], dtype=torch.float64, device=dev) if with_obj else None
    ws = {}
    args = (c["sigma"].to(dev), c["cells"].to(torch.int32).to(dev), c["bidx"].to(dev), E, O,
            c["Pr_b"].to(dev), c["theta"].to(dev), ws)
    if fused:
        kw = dict(Y=c["Y"].to(dev), Zt=c["Zt"].to(dev), obj=obj)
        distT = None
    else:
        kw = dict(obj=obj) if with_obj else {}
        distT = c["distT"].to(dev)
    ops.harmony_block_update(Rt, distT, *args, steps=(0,), **kw)
    torch.cuda.synchronize()
    s0 = dict(Rt=Rt.cpu(), E=E.cpu(), O=O.cpu(), pen=ws["pen"].cpu(),
              obj=obj.cpu() if with_obj else None)
    ops.harmony_block_update(Rt, distT, *args, steps=(1,), **kw)
    torch.cuda.synchronize()
    s1 = dict(Rt=Rt.cpu(), E=E.cpu(), O=O.cpu(), pen=ws["pen"].cpu(),
              obj=obj.cpu() if with_obj else None, E_dev=E, O_dev=O, obj_dev=obj)
    return s0, s1


def test_cases_cover_every_wave_count_and_rank():
    """The wave counts are the launcher's own answer (harmony_block_waves), not arithmetic
    in a comment: W = 1, 2, 3 and 4 all run, and K = 1, 48, 64, 65, 100 and 128."""
    seen = set()
    for name, (K, levels, d, _, _, want) in CASES.items():
        B = sum(levels)
        got = (ops._hip.harmony_block_waves(K, B, d), ops._hip.harmony_block_waves(K, B, 0))
        assert got == want, (name, got, want)
        assert ops.harmony_native_ok(torch.zeros(1, device="cuda"), K, B), name
        assert ops.harmony_centroids_ok(d, K), name
        seen.update(got)
    assert seen == {1, 2, 3, 4}
    assert {c[0] for c in CASES.values()} == {1, 48, 64, 65, 100, 128}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "distT"])
@pytest.mark.parametrize("name", list(CASES))
def test_block_update_matches_host_reference(name, fused):
    """Remove step, then assign step, each against the host float64 formula; the round
    objective from that state; and the whole sequence a second time, bitwise equal."""
    c = _case(name)
    K, B, nb = c["K"], c["B"], c["nb"]
    assert ops._hip.harmony_block_waves(K, B, c["d"] if fused else 0) == CASES[name][5][not fused]
    s0, s1 = _run_block(c, fused)
    close = functools.partial(torch.testing.assert_close, rtol=RTOL)
    cl = c["cells"]
    # ---- after the remove step alone
    # (every cell of ``maxkb`` is removed: O1 and E1 are differences of equal numbers)
    a_rm = ATOL_CANCEL if name == "maxkb" else ATOL
    close(s0["E"], c["E1"], atol=a_rm)
    close(s0["O"], c["O1"], atol=a_rm)
    close(s0["pen"], c["Pen"], atol=ATOL)
    assert torch.equal(s0["Rt"], c["Rt"])                       # R is only read
    assert torch.equal(s0["obj"], torch.tensor([0.25, -0.5], dtype=torch.float64))
    # ---- after the assign step on that state
    close(s1["Rt"][cl], c["Rn"].t(), atol=ATOL_R)
    close(s1["E"], c["E2"], atol=ATOL)
    close(s1["O"], c["O2"], atol=ATOL)
    rest = torch.ones(c["N"], dtype=torch.bool)
    rest[cl] = False
    assert torch.equal(s1["Rt"][rest], c["Rt"][rest])           # other cells' rows untouched
    close(s1["Rt"][cl].sum(dim=1), torch.ones(nb, dtype=torch.float64), rtol=0, atol=1e-12)
    assert torch.equal(s1["pen"], s0["pen"])                    # the assign only reads it
    start = torch.tensor([0.25, -0.5], dtype=torch.float64)
    if fused:      # the objective terms are added to what obj held
        close(s1["obj"] - start, torch.stack([c["km"], c["ent"]]), atol=ATOL)
    else:          # an assign from a distance matrix reports none
        assert torch.equal(s1["obj"], start)
    # the new R holds exact zeros and/or denormals wherever the host reference does (the
    # entropy guard's case); K = 1 has a single cluster of weight 1
    if K > 1 and nb > 1:
        assert int((c["Rn"] < torch.finfo(torch.float64).tiny).sum()) > 0
    # ---- the round objective from this state (K * B = 4096 in ``maxkb``: 16 trips)
    dev = torch.device("cuda")
    obj = torch.stack([c["km"], c["ent"]]).to(dev)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    ops.harmony_objective(s1["O_dev"], s1["E_dev"], c["sigma"].to(dev), c["theta"].to(dev),
                          obj, out)
    close(out.cpu()[0], c["km"] + c["ent"] + c["cross"], atol=ATOL)
    assert torch.equal(obj.cpu(), torch.zeros(2, dtype=torch.float64))
    # ---- a second run from the same inputs: bitwise the same
    t0, t1 = _run_block(c, fused)
    for k in ("Rt", "E", "O", "pen", "obj"):
        assert torch.equal(s0[k], t0[k]), k
        assert torch.equal(s1[k], t1[k]), k


def test_block_update_without_obj_for_distance_matrix():
    """The distT variant takes no obj at all (as Harmony._update_R calls it)."""
    c = _case("k65")
    _, s1 = _run_block(c, fused=False, with_obj=False)
    torch.testing.assert_close(s1["Rt"][c["cells"]], c["Rn"].t(), rtol=RTOL, atol=ATOL_R)
    torch.testing.assert_close(s1["E"], c["E2"], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(s1["O"], c["O2"], rtol=RTOL, atol=ATOL)


# (N, d, K) in growing order of the partial-sum workspace, which the cases share: every
# one finds the cached ``cpart`` too small.  N < 4: one partial MFMA step; K = 100: wave 3
# has no second cluster tile; 64 x 128: all 4 x 8 tiles; K = 48: wave 3 exits; 66001:
# chunk = 68, 971 workgroups (16 trips of the sum_rows loop), a ragged last chunk.
CENTROID_SHAPES = [(1027, 1, 1), (3, 5, 7), (1027, 16, 48), (1027, 17, 49), (1027, 50, 100),
                   (1027, 64, 128), (66001, 17, 70)]
_CEN_WS: dict = {}


@pytest.mark.parametrize("N,d,K", CENTROID_SHAPES)
def test_centroids_match_host_reference(N, d, K):
    g = torch.Generator().manual_seed(N + 64 * d + K)
    Z = torch.randn((d, N), generator=g, dtype=torch.float64)
    Zc = Z / torch.linalg.vector_norm(Z, dim=0)
    R = torch.rand((K, N), generator=g, dtype=torch.float64)
    R = R / R.sum(dim=0)
    assert ops.harmony_centroids_ok(d, K)
    dev = torch.device("cuda")
    Zt, Rt = Zc.t().contiguous().to(dev), R.t().contiguous().to(dev)
    chunk = -(-max(64, -(-N // 1024)) // 4) * 4
    need = -(-N // chunk) * d * K
    had = _CEN_WS["cpart"].numel() if "cpart" in _CEN_WS else 0
    Y1 = ops.harmony_centroids(Zt, Rt, _CEN_WS).cpu()
    assert _CEN_WS["cpart"].numel() >= need and (had >= need or _CEN_WS["cpart"].numel() == need)
    Y2 = ops.harmony_centroids(Zt, Rt, _CEN_WS).cpu()
    torch.testing.assert_close(Y1, Zc @ R.t(), rtol=1e-10, atol=1e-12)
    assert torch.equal(Y1, Y2)


def test_run_harmony_at_production_rank_matches_cpu():
    """run_harmony on 3000 cells (K = 100, the production rank) on the GPU == the torch
    block loop on the host, same seed and block order, to the bounds of
    test_harmony_native_matches_cpu.  On the host this problem took 0.9 s and ran [19, 6]
    k-means rounds; moving every input up by one ulp left the rounds as they were and moved
    R by 8.0e-16 and Z_corr by 2.2e-14, six to seven orders below the bounds, so a flipped
    convergence test is not expected."""
    import pandas as pd

    from cnmf_torch_amd.models.harmony import run_harmony

    rs = np.random.default_rng(0)
    n, d = 3000, 20
    types = rs.integers(0, 3, n)
    batch = rs.integers(0, 3, n)
    donor = rs.integers(0, 2, n)
    Z = rs.normal(size=(3, d))[types] * 3 + rs.normal(size=(3, d))[batch] * 2 + \
        0.3 * rs.normal(size=(n, d))
    meta = pd.DataFrame({"batch": pd.Categorical(batch.astype(str)),
                         "donor": pd.Categorical(donor.astype(str))})
    kw = dict(theta=[2.0, 0.5], max_iter_harmony=2, random_state=0)
    gpu = run_harmony(Z, meta, ["batch", "donor"], device="cuda", **kw)
    cpu = run_harmony(Z, meta, ["batch", "donor"], device="cpu", **kw)
    assert gpu.K == 100 and cpu.K == 100
    assert ops.harmony_native_ok(torch.zeros(1, device="cuda"), gpu.K, gpu.Phi.shape[0])
    assert ops.harmony_centroids_ok(d, 100)
    np.testing.assert_allclose(gpu.R, cpu.R, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(gpu.Z_corr, cpu.Z_corr, rtol=1e-6, atol=1e-8)
    assert gpu.kmeans_rounds == cpu.kmeans_rounds


def _raw_block(K, B, d, fused):
    """The raw launcher call of an assign step on zero-filled buffers of the right sizes."""
    dev = torch.device("cuda")
    N = 4

    def z(*s, dt=torch.float64):
        return torch.zeros(s, dtype=dt, device=dev)

    Rt, distT, sigma = z(N, K), z(N, K), z(K) + 1
    cells = torch.arange(N, dtype=torch.int32, device=dev)
    bidx = z(1, N, dt=torch.int32)
    E, O, Pr_b, theta, pen = z(K, B), z(K, B), z(B), z(B), z(K, B)
    part = z(K * (B + 1) + 2)
    Y, Zt, obj = z(max(d, 1), K), z(N, max(d, 1)), z(2)
    ops._hip.harmony_block(1, Rt.data_ptr(), 0 if fused else distT.data_ptr(), sigma.data_ptr(),
                           cells.data_ptr(), bidx.data_ptr(), N, N, K, B, 1, 16, E.data_ptr(),
                           O.data_ptr(), Pr_b.data_ptr(), theta.data_ptr(), pen.data_ptr(),
                           part.data_ptr(), Y.data_ptr(), Zt.data_ptr(), d, obj.data_ptr(),
                           ops._stream_ptr(Rt))


@pytest.mark.parametrize("K,B,d,fused", [(129, 1, 8, False), (129, 1, 8, True),
                                         (17, 241, 8, False), (17, 241, 8, True),
                                         (100, 5, 65, True)])
def test_block_sizes_beyond_the_kernel_are_rejected(K, B, d, fused):
    """K > 128, K * B > 4096 and (fused distances) d > 64: the predicates say no, the wave
    query returns 0 and the launcher raises before anything is launched."""
    t = torch.zeros(1, device="cuda")
    if d > 64:
        assert not ops.harmony_centroids_ok(d, K)
        assert ops.harmony_native_ok(t, K, B)        # the distT variant still takes it
        assert ops._hip.harmony_block_waves(K, B, 0) > 0
    else:
        assert not ops.harmony_native_ok(t, K, B)
    assert ops._hip.harmony_block_waves(K, B, d if fused else 0) == 0
    with pytest.raises(RuntimeError, match="harmony_block"):
        _raw_block(K, B, d, fused)
    torch.cuda.synchronize()


@pytest.mark.parametrize("d,K", [(65, 100), (20, 129)])
def test_centroid_sizes_beyond_the_kernel_are_rejected(d, K):
    dev = torch.device("cuda")
    assert not ops.harmony_centroids_ok(d, K)
    Zt = torch.zeros((8, d), dtype=torch.float64, device=dev)
    Rt = torch.zeros((8, K), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="beyond the kernel"):
        ops.harmony_centroids(Zt, Rt, {})
    part = torch.zeros(d * K, dtype=torch.float64, device=dev)
    Y = torch.zeros((d, K), dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="harmony_centroid"):
        ops._hip.harmony_centroid(Zt.data_ptr(), Rt.data_ptr(), 8, d, K, 64, part.data_ptr(),
                                  Y.data_ptr(), ops._stream_ptr(Zt))
    torch.cuda.synchronize()


def _good_args():
    """Valid arguments of harmony_block_update (distT variant) and harmony_objective."""
    dev = torch.device("cuda")
    N, K, B = 8, 5, 3

    def z(*s, dt=torch.float64):
        return torch.zeros(s, dtype=dt, device=dev)

    return dict(Rt=z(N, K) + 1.0 / K, distT=z(N, K), sigma=z(K) + 0.1,
                cells=torch.arange(N, dtype=torch.int32, device=dev),
                bidx=z(1, N, dt=torch.int32), E=z(K, B), O=z(K, B), Pr_b=z(B) + 1.0 / B,
                theta=z(B) + 1, ws={})


def _call_block(a):
    ops.harmony_block_update(a["Rt"], a["distT"], a["sigma"], a["cells"], a["bidx"], a["E"],
                             a["O"], a["Pr_b"], a["theta"], a["ws"])


BAD_BLOCK_ARGS = {
    "sigma float32": lambda a: a.update(sigma=a["sigma"].float()),
    "sigma length": lambda a: a.update(sigma=a["sigma"][:-1].contiguous()),
    "sigma strided": lambda a: a.update(sigma=a["sigma"].repeat_interleave(2)[::2]),
    "sigma on the host": lambda a: a.update(sigma=a["sigma"].cpu()),
    "theta length": lambda a: a.update(theta=a["theta"][:-1].contiguous()),
    "theta float32": lambda a: a.update(theta=a["theta"].float()),
    "Pr_b length": lambda a: a.update(Pr_b=torch.cat([a["Pr_b"], a["Pr_b"]])),
    "Pr_b float32": lambda a: a.update(Pr_b=a["Pr_b"].float()),
    "E shape": lambda a: a.update(E=a["E"][:-1].contiguous()),
    "E strided": lambda a: a.update(E=a["E"].t().contiguous().t()),
    "pen shape": lambda a: a["ws"].update(pen=torch.zeros((3, 5), dtype=torch.float64,
                                                          device="cuda")),
    "pen float32": lambda a: a["ws"].update(pen=torch.zeros((5, 3), device="cuda")),
    "pen on the host": lambda a: a["ws"].update(pen=torch.zeros((5, 3), dtype=torch.float64)),
}


@pytest.mark.parametrize("what", list(BAD_BLOCK_ARGS))
def test_block_update_rejects_bad_arguments(what):
    """A table of another dtype, length, layout or device raises before any launch: R, E
    and O keep their bits."""
    a = _good_args()
    BAD_BLOCK_ARGS[what](a)
    keep = {k: a[k].clone() for k in ("Rt", "E", "O")}
    with pytest.raises(ValueError):
        _call_block(a)
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(a[k], v), k


def test_block_update_keeps_a_matching_penalty_table():
    """ws["pen"] of the right shape is the caller's (Harmony._init_fused sets it): an
    assign step alone reads it and does not replace it."""
    a = _good_args()
    pen = torch.full((5, 3), 0.5, dtype=torch.float64, device="cuda")
    a["ws"]["pen"] = pen
    ops.harmony_block_update(a["Rt"], a["distT"], a["sigma"], a["cells"], a["bidx"], a["E"],
                             a["O"], a["Pr_b"], a["theta"], a["ws"], steps=(1,))
    torch.cuda.synchronize()
    assert a["ws"]["pen"] is pen
    assert torch.equal(pen.cpu(), torch.full((5, 3), 0.5, dtype=torch.float64))
    # zero distances, a flat table: R = 1 / K whatever the penalty's value
    torch.testing.assert_close(a["Rt"].cpu(), torch.full((8, 5), 0.2, dtype=torch.float64),
                               rtol=0, atol=1e-15)


BAD_OBJECTIVE_ARGS = {
    "E shape": lambda a: a.update(E=a["E"].t().contiguous()),
    "O strided": lambda a: a.update(O=a["O"].t().contiguous().t()),
    "sigma float32": lambda a: a.update(sigma=a["sigma"].float()),
    "sigma length": lambda a: a.update(sigma=a["sigma"][:-1].contiguous()),
    "theta length": lambda a: a.update(theta=a["theta"][:-1].contiguous()),
    "theta on the host": lambda a: a.update(theta=a["theta"].cpu()),
    "obj length": lambda a: a.update(obj=torch.zeros(1, dtype=torch.float64, device="cuda")),
    "obj float32": lambda a: a.update(obj=torch.zeros(2, device="cuda")),
    "out empty": lambda a: a.update(out=torch.zeros(0, dtype=torch.float64, device="cuda")),
    "out float32": lambda a: a.update(out=torch.zeros(1, device="cuda")),
}


@pytest.mark.parametrize("what", list(BAD_OBJECTIVE_ARGS))
def test_objective_rejects_bad_arguments(what):
    a = _good_args()
    a["obj"] = torch.ones(2, dtype=torch.float64, device="cuda")
    a["out"] = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    BAD_OBJECTIVE_ARGS[what](a)
    with pytest.raises(ValueError):
        ops.harmony_objective(a["O"], a["E"], a["sigma"], a["theta"], a["obj"], a["out"])
    torch.cuda.synchronize()
    if a["obj"].numel() == 2 and a["obj"].dtype == torch.float64:
        assert torch.equal(a["obj"].cpu(), torch.ones(2, dtype=torch.float64))   # not reset
