"""gemm_tiles.hip -- the data-side products on tile storage (models.nmf.SparseTilesX) --
against the float64 product and the dense-plane kernel, and the solver on the holder."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.models.nmf import NMFBatchSolver, NMFOptions, SparseTilesX, _XPlanes

from sparse_tiles_inputs import count_matrix, float_matrix

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _input(kind: str, N: int, G: int):
    """(holder on the GPU, the float64 matrix the value planes hold: counts, or X itself)."""
    if kind == "float":
        X = float_matrix(N, G, blocks=True)
        D = X.astype(np.float64)
    else:
        X, C = count_matrix(N, G, two_planes=kind == "count2", blocks=True)
        D = C.astype(np.float64)
    h = SparseTilesX.from_scipy(sp.csr_matrix(X), device="cuda", rows=128)
    assert h.pb == {"count1": 1, "count2": 2, "float": _XPlanes._float_planes(G)}[kind]
    # the stored planes are exactly D: what is checked below is the product alone
    dense = ops.reference.planes_to_f64(ops.reference.tiles_to_planes(h.tiles)).sum(0)
    assert torch.equal(dense.cpu(), torch.from_numpy(D))
    assert not D[:, 64:128].any() and D[64:128, :64].all()      # an empty and a full tile
    return h, torch.from_numpy(D)


def _operands(h, side, r0, r1, M, seed):
    """fp32 A for the product, its three planes, and A as float64 the way the planes hold
    it (side n: times the unit, in fp32 as split_planes multiplies)."""
    g = torch.Generator().manual_seed(seed)
    k = h.shape[1] if side == "n" else r1 - r0
    kd = h.Gp if side == "n" else -(-k // 64) * 64
    A = torch.rand((M, k), generator=g).cuda()
    pl = torch.zeros((3, M + 3, kd), dtype=torch.int16, device="cuda")   # rows beyond M
    mul = h.unit if side == "n" else None
    ops.split_planes(A, pl, col_mul=mul)
    A64 = (A * mul if mul is not None else A).double().cpu()
    return pl, A64


def _check(h, D, side, r0, r1, M):
    pl, A64 = _operands(h, side, r0, r1, M, seed=M + r0)
    G = h.shape[1]
    unit = h.unit.double().cpu() if h.unit is not None else torch.ones(G, dtype=torch.float64)
    if side == "n":
        K, ncol = G, r1 - r0
        ref = A64 @ D[r0:r1].t()
        scale = None
    else:
        K, ncol = r1 - r0, G
        ref = (A64 @ D[r0:r1]) * unit
        scale = h.unit
    tol = 1e-6 * max(1.0, K / 256)      # the bound of test_gemm_planes_matches_fp64
    # plain store
    C = torch.full((M, ncol + 5), -7.0, device="cuda")
    ops.gemm_tiles(C, pl, h.tiles, side, r0, r1, M, col_scale=scale)
    err = float((C[:, :ncol].cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"{side} pb={h.pb} rows [{r0}, {r1}) M={M}: store err {err:.3e} (tol {tol:.1e})")
    assert err < tol
    assert bool((C[:, ncol:] == -7.0).all())               # nothing beyond the columns
    # accumulate with a column scale (side n has no unit to fold: a random one)
    g = torch.Generator().manual_seed(1)
    C0 = torch.rand((M, ncol), generator=g)
    sc = h.unit if side == "s" and h.unit is not None else \
        (torch.rand(ncol, generator=g) + 0.5).cuda()
    raw = A64 @ (D[r0:r1].t() if side == "n" else D[r0:r1])
    ref2 = C0.double() + raw * sc.double().cpu()
    C2 = C0.clone().cuda()
    ops.gemm_tiles(C2, pl, h.tiles, side, r0, r1, M, accumulate=True, col_scale=sc)
    err2 = float((C2.cpu().double() - ref2).abs().max() / ref2.abs().max())
    print(f"   accumulate err {err2:.3e}")
    assert err2 < tol
    # repeatable bit for bit
    C3 = torch.full((M, ncol + 5), -7.0, device="cuda")
    ops.gemm_tiles(C3, pl, h.tiles, side, r0, r1, M, col_scale=scale)
    assert torch.equal(C, C3)
    # the gate at 0 leaves C untouched
    gate = torch.zeros(1, dtype=torch.int32, device="cuda")
    C4 = C0.clone().cuda()
    ops.gemm_tiles(C4, pl, h.tiles, side, r0, r1, M, gate=gate)
    assert torch.equal(C4.cpu(), C0)
    # against the dense-plane kernel on the same operands (k order may differ), also with
    # two A planes
    xp = _dense_planes(h)
    for pa in (3, 2):
        a = torch.empty((M, ncol), device="cuda")
        b = torch.empty((M, ncol), device="cuda")
        ops.gemm_tiles(a, pl[:pa], h.tiles, side, r0, r1, M, col_scale=scale)
        if side == "n":
            ops.gemm_planes(b, pl[:pa], xp.x[:, r0:], M, ncol, h.Gp)
        else:
            ops.gemm_planes(b, pl[:pa], xp.xt[:, :, r0:], M, ncol, pl.shape[2], col_scale=scale)
        d = float((a - b).abs().max() / b.abs().max())
        print(f"   vs gemm_planes, {pa} A planes: {d:.3e}")
        assert d < 2 * tol


_PLANES: dict = {}


def _dense_planes(h):
    if id(h) not in _PLANES:
        _PLANES[id(h)] = _XPlanes(h.to_dense())
        assert _PLANES[id(h)].pb == h.pb
    return _PLANES[id(h)]


@pytest.mark.parametrize("rows", [(0, 250), (104, 208)])
@pytest.mark.parametrize("side", ["n", "s"])
@pytest.mark.parametrize("kind", ["count1", "count2", "float"])
def test_gemm_tiles_matches_fp64(kind, side, rows):
    h, D = _input(kind, 250, 150)
    _check(h, D, side, rows[0], rows[1], 37)


@pytest.mark.parametrize("rows", [(0, 700), (104, 680)])
@pytest.mark.parametrize("side", ["n", "s"])
def test_gemm_tiles_across_workgroup_tiles(side, rows):
    """More than one workgroup tile in M, in the cells and in the genes."""
    h, D = _input("count1", 700, 330)
    _check(h, D, side, rows[0], rows[1], 300)


_SOLVE = dict(online_chunk_size=400, online_max_pass=30)
_SEEDS, _KS = [5, 6, 7, 8, 9, 10], [5, 6, 7, 9, 5, 7]


@functools.lru_cache(maxsize=None)
def _solver_input():
    X, _ = count_matrix(1200, 300)
    h = SparseTilesX.from_scipy(sp.csr_matrix(X), device="cuda", rows=512)
    assert h.unit is not None and h.pb == 1
    return torch.from_numpy(X).cuda(), h


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("algo", ["mu", "hals"])
def test_solver_on_tiles_matches_dense_storage(algo, fused, monkeypatch):
    """The tolerances of test_split_gemm_solver_matches_fp32_library_gemm; the dense side
    with its default fused step and with the like-for-like unfused passes."""
    X, h = _solver_input()
    opts = NMFOptions(n_components=5, algo=algo, **_SOLVE)
    got = NMFBatchSolver(h, opts).run(_SEEDS, ks=_KS)
    monkeypatch.setenv("CNMF_FUSED_STEP", fused)
    ref = NMFBatchSolver(X, opts).run(_SEEDS, ks=_KS)
    print(algo, fused, got.n_iter, ref.n_iter, np.abs(got.err / ref.err - 1).max())
    np.testing.assert_allclose(got.err, ref.err, rtol=1e-4)
    assert np.abs(got.n_iter - ref.n_iter).max() <= 1


def test_tiles_pass_graph_replay_matches_eager(monkeypatch):
    """As test_online_pass_graph_replay_matches_eager, on the holder."""
    _, h = _solver_input()
    opts = NMFOptions(n_components=7, tol=1e-6, online_chunk_size=400, online_max_pass=8)
    seeds = list(range(40, 52))
    monkeypatch.setenv("CNMF_GRAPHS", "1")
    g = NMFBatchSolver(h, opts).run(seeds)
    monkeypatch.setenv("CNMF_GRAPHS", "0")
    e = NMFBatchSolver(h, opts).run(seeds)
    np.testing.assert_array_equal(g.W.cpu().numpy(), e.W.cpu().numpy())
    np.testing.assert_array_equal(g.err, e.err)
    np.testing.assert_array_equal(g.n_iter, e.n_iter)
    assert (g.n_iter >= 1).all() and (g.n_iter <= 8).all()
