"""The NI != 4 tile family of the split-plane GEMM (gemm_planes.h: variants 6 = 128 x 160,
7 = 128 x 320, 8 = 128 x 64, 9 = 128 x 32) against the fp64 product and, bitwise, against
variant 0: with k unsplit every output element is accumulated over k in the same order
whatever the tile shape, k-step depth or stage count, and at an equal k-step depth the
k slices of a split are the same, so the slice-order sum is too.

(k-step depth, stages) pairs a tile does not support are remapped by the launcher, never
rejected: a 64-deep step whose two stages exceed the 160 KB of LDS runs 32 deep (here:
variant 7 with three A planes), a third stage that does not fit runs as two.  A 32-deep
step whose B tile does not divide over the threads (variants 6, 7: 2.5 chunks per thread;
variant 9: half a chunk) runs with the ragged last staging round and per-wave counts.
"""
import contextlib
import os

import pytest
import torch

from cnmf_torch_amd import ops

pytestmark = pytest.mark.gpu

NEW = sorted(v for v in ops._GEMM_TILES if v >= 6)


@contextlib.contextmanager
def _knobs(bk, stages):
    keys = {"CNMF_GEMM_BK": bk, "CNMF_GEMM_STAGES": stages}
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k, v in keys.items():
            os.environ[k] = str(v)
        ops.refresh_env()
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ops.refresh_env()


def _operands(M, N, K, pb, seed, top=200):
    """(Ap 3 planes, Bp pb planes, Kd, fp64 product); plane rows == M / N exactly, so tiles
    past the edge exercise the row clamp."""
    g = torch.Generator().manual_seed(seed)
    Kd = -(-K // ops.planes_bk(pb)) * ops.planes_bk(pb)
    A = torch.rand((M, K), generator=g)
    B = torch.randint(0, top if pb == 1 else 60000, (N, K), generator=g).float()
    Ap = torch.zeros((3, M, Kd), dtype=torch.int16, device="cuda")
    Bp = torch.zeros((pb, N, Kd), dtype=torch.int16, device="cuda")
    ops.split_planes(A.cuda(), Ap)
    ops.split_planes(B.cuda(), Bp)
    return Ap, Bp, Kd, A.double() @ B.double().t()


@pytest.fixture(scope="module")
def ragged():
    """The shape of test_gemm_planes_every_tile_variant: ragged in M and N, N no multiple
    of 16, k padded (1000 -> 1024)."""
    return (301, 650, 1000) + _operands(301, 650, 1000, 1, 11)


def _run(Ap, Bp, M, N, Kd, v, ks, **kw):
    C = torch.full((M, N), float("nan"), device="cuda")
    ops.gemm_planes(C, Ap, Bp, M, N, Kd, plan=(v, ks), **kw)
    torch.cuda.synchronize()
    return C


def _err(C, ref):
    return float((C.cpu().double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("variant", NEW)
@pytest.mark.parametrize("bk,stages", [(32, 2), (32, 3), (64, 2)])
def test_new_variants_match_fp64(ragged, variant, bk, stages):
    M, N, K, Ap, Bp, Kd, ref = ragged
    with _knobs(bk, stages):
        for ks in (1, 3):
            err = _err(_run(Ap, Bp, M, N, Kd, variant, ks), ref)
            print(f"variant {variant} bk {bk} stages {stages} ksplit {ks}: err {err:.3e}")
            assert err < 1e-6 * K / 256, (variant, bk, stages, ks, err)


@pytest.mark.parametrize("pa,pb", [(2, 1), (3, 1), (2, 2), (3, 2)])
def test_unsplit_is_bitwise_variant0(pa, pb):
    M, N, K = 301, 650, 1000
    Ap, Bp, Kd, _ = _operands(M, N, K, pb, 20 + pb)
    with _knobs(32, 2):
        want = _run(Ap[:pa], Bp, M, N, Kd, 0, 1)
    for bk in (32, 64):
        with _knobs(bk, 2):
            for v in NEW:
                assert torch.equal(_run(Ap[:pa], Bp, M, N, Kd, v, 1), want), (v, bk, pa, pb)


@pytest.mark.parametrize("bk", [32, 64])
def test_split3_is_bitwise_variant0_at_equal_kstep(ragged, bk):
    # two A planes: every variant's 64-deep stage pair fits, so no k-step is remapped and
    # the three k slices are the same k ranges in every variant
    M, N, K, Ap, Bp, Kd, _ = ragged
    with _knobs(bk, 2):
        want = _run(Ap[:2], Bp, M, N, Kd, 0, 3)
        for v in NEW:
            assert torch.equal(_run(Ap[:2], Bp, M, N, Kd, v, 3), want), (v, bk)


@pytest.mark.parametrize("M,N", [(5, 20), (129, 161), (128, 160)])
def test_degenerate_extents(M, N):
    K = 1000
    Ap, Bp, Kd, ref = _operands(M, N, K, 1, M + N)
    assert Ap.shape[1] == M and Bp.shape[1] == N
    for v in NEW:
        for bk in (32, 64):
            with _knobs(bk, 3):
                err = _err(_run(Ap, Bp, M, N, Kd, v, 1), ref)
                assert err < 1e-6 * K / 256, (v, bk, M, N, err)


@pytest.mark.parametrize("variant", NEW)
def test_raw_slabs_and_gate(ragged, variant):
    M, N, K, Ap, Bp, Kd, ref = ragged
    ks = 3
    reduced = _run(Ap, Bp, M, N, Kd, variant, ks)
    slab = torch.full((ks * M * N,), float("nan"), device="cuda")
    assert ops.gemm_planes(None, Ap, Bp, M, N, Kd, raw_slab=slab, plan=(variant, ks)) == ks
    parts = slab.view(ks, M, N)
    total = torch.zeros((M, N), device="cuda")
    for s in range(ks):             # slice order, from zero: what gemm_reduce does
        total = total + parts[s]
    assert torch.equal(total, reduced)
    one = torch.full((M * N,), float("nan"), device="cuda")
    assert ops.gemm_planes(None, Ap, Bp, M, N, Kd, raw_slab=one, plan=(variant, 1)) == 1
    assert torch.equal(one.view(M, N), _run(Ap, Bp, M, N, Kd, variant, 1))
    # gate 0: a poisoned output stays; gate 1: computed
    C = torch.full((M, N), -7.0, device="cuda")
    ops.gemm_planes(C, Ap, Bp, M, N, Kd, plan=(variant, 1),
                    gate=torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert bool((C == -7.0).all())
    ops.gemm_planes(C, Ap, Bp, M, N, Kd, plan=(variant, 1),
                    gate=torch.ones(1, dtype=torch.int32, device="cuda"))
    assert _err(C, ref) < 1e-6 * K / 256


@pytest.mark.parametrize("variant", NEW)
def test_accumulate_with_col_scale(ragged, variant):
    M, N, K, Ap, Bp, Kd, ref = ragged
    g = torch.Generator().manual_seed(3)
    scale = torch.rand(N, generator=g) + 0.5
    base = torch.rand((M, N), generator=g) * 1000.0
    want = base.double() + ref * scale.double()
    for ks in (1, 3):
        C = base.clone().cuda()
        ops.gemm_planes(C, Ap, Bp, M, N, Kd, accumulate=True, col_scale=scale.cuda(),
                        plan=(variant, ks))
        err = float((C.cpu().double() - want).abs().max())
        # the product to the project's bound (times the largest scale), plus one fp32
        # rounding each of the scaling and of the addition
        bound = 1e-6 * K / 256 * float(ref.abs().max() * scale.max()) \
            + 2 * 2.0 ** -24 * float(want.abs().max())
        assert err < bound, (variant, ks, err, bound)
