"""ops.gemm_plan (host side, no GPU), for raw-slab consumers (the fused pass: RAW slabs) and
for self-reduced products (raw_max None): known variants, admissible k splits, the
environment overrides, slab sizing of the fused step, and the tile table of the original
variants."""
import itertools

import pytest

from cnmf_torch_amd import ops
from cnmf_torch_amd.models.nmf_base import _FUSED_MAX_SLABS as RAW

# the shapes of tools/gemm_plan_sweep.py: numerator rows x 5000 x 2048, statistics rows x
# 2000 x 5056, for the K = 10 layouts (1000 ... 20 rows) and the K = 20 / 30 main passes
SWEPT = [(M, N, Kd, 1) for M in (1000, 640, 320, 100, 20, 2000, 3000)
         for N, Kd in ((5000, 2048), (2000, 5056))]
GRID = SWEPT + [(M, N, Kd, pb) for M, N, Kd, pb in itertools.product(
    (1, 7, 128, 129, 500, 5000, 20000), (16, 300, 2000, 5008), (64, 320, 1024, 10048),
    (1, 2, 3))]


@pytest.fixture
def env(monkeypatch):
    def set_(**kw):
        for k in ("CNMF_GEMM_VARIANT", "CNMF_GEMM_KSPLIT", "CNMF_GEMM_BK", "CNMF_GEMM_STAGES"):
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            monkeypatch.setenv("CNMF_GEMM_" + k, str(v))
        ops.refresh_env()
    set_()
    yield set_
    monkeypatch.undo()
    ops.refresh_env()


def test_plan_returns_known_variant_and_admissible_split(env):
    for (M, N, Kd, pb), raw in itertools.product(GRID, (RAW, None)):
        v, ks = ops.gemm_plan(M, N, Kd, pb, raw)
        assert v in ops._GEMM_TILES, (M, N, Kd, pb, v)
        assert 1 <= ks <= Kd // ops.planes_bk(pb), (M, N, Kd, pb, ks)
        assert (v, ks) == ops.gemm_plan(M, N, Kd, pb, raw)
        if raw is None:         # the self-reduced path keeps the original six tiles
            assert v <= 5
        assert ops.gemm_kstep(v) in (32, 64) and ops.gemm_stages(v) in (2, 3)
        # 128 x 320 with three planes each side does not fit in LDS, and the caller
        # chooses the A planes: never planned with three B planes
        assert not (v == 7 and pb == 3)


def test_headline_plans(env):
    """The measured choices the constants were fitted to reproduce: one wave of workgroups
    and no k split for the 1000 / 2000 x 5000 numerators, the parent's plan for the
    statistics products, and at most _FUSED_MAX_SLABS slices (no gemm_reduce launch) for
    the shrunken layouts down to 100 rows."""
    assert ops.gemm_plan(1000, 5000, 2048, 1, RAW) == (6, 1)
    assert ops.gemm_plan(2000, 5000, 2048, 1, RAW) == (7, 1)
    assert ops.gemm_plan(1000, 2000, 5056, 1, RAW) == (1, 4)
    assert ops.gemm_plan(2000, 2000, 5056, 1, RAW) == (1, 2)
    assert ops.gemm_plan(3000, 5000, 2048, 1, RAW) == (1, 1)
    assert ops.gemm_plan(5000, 5000, 2048, 1, RAW) == (7, 1)      # no k split above 4096 rows
    assert ops.gemm_plan(5000, 2000, 5056, 1, RAW) == (1, 1)
    for M, N, Kd, pb in SWEPT:
        if M >= 100:
            assert ops.gemm_plan(M, N, Kd, pb, RAW)[1] <= RAW, (M, N)


def test_env_overrides_win(env):
    M, N, Kd = 1000, 5000, 2048
    for v in ops._GEMM_TILES:
        for raw in (RAW, None):
            env(VARIANT=v)
            assert ops.gemm_plan(M, N, Kd, 1, raw)[0] == v
            env(VARIANT=v, KSPLIT=3)
            assert ops.gemm_plan(M, N, Kd, 1, raw) == (v, 3)
    for raw in (RAW, None):
        env(KSPLIT=2)
        assert ops.gemm_plan(M, N, Kd, 1, raw)[1] == 2
        env(KSPLIT=1000)                      # clamped to the k-steps there are
        assert ops.gemm_plan(M, N, Kd, 1, raw)[1] == Kd // ops.planes_bk(1)
    env(BK=32, STAGES=3)
    assert all(ops.gemm_kstep(v) == 32 and ops.gemm_stages(v) == 3 for v in ops._GEMM_TILES)
    env()
    assert ops.gemm_kstep(6) == 64 and ops.gemm_kstep(4) == 32 and ops.gemm_stages(1) == 3


@pytest.mark.parametrize("rows", [1000, 640, 320, 100, 20, 2000, 3000])
@pytest.mark.parametrize("cws", [[5000, 5000], [4096, 4096, 1808], [10000]])
def test_fused_slabs_cover_every_chunk(env, rows, cws):
    """The slab sizes models.nmf._fused_bufs allocates (the largest k split over the chunk
    widths times rows x the widest chunk / x G) hold ksplit x M x N of every chunk's plan,
    which gemm_planes(raw_slab=..., raw_max=RAW) computes from the same arguments."""
    G, pb = 2000, 1
    Gp = -(-G // 64) * 64
    bk = ops.planes_bk(pb)
    ks_n = max(ops.gemm_plan(rows, cw, Gp, pb, RAW)[1] for cw in cws)
    ks_b = max(ops.gemm_plan(rows, G, -(-cw // bk) * bk, pb, RAW)[1] for cw in cws)
    slab_n, slab_b = ks_n * rows * max(cws), ks_b * rows * G
    for cw in cws:
        assert ops.gemm_plan(rows, cw, Gp, pb, RAW)[1] * rows * cw <= slab_n
        assert ops.gemm_plan(rows, G, -(-cw // bk) * bk, pb, RAW)[1] * rows * G <= slab_b


def test_original_tile_table_unchanged():
    want = {0: (128, 128), 1: (128, 256), 2: (256, 128), 3: (64, 128), 4: (64, 128),
            5: (128, 128)}
    assert {v: ops._GEMM_TILES[v] for v in range(6)} == want
    assert sorted(ops._GEMM_TILES) == list(range(len(ops._GEMM_TILES))) and \
        len(ops._GEMM_TILES) <= 12
    if ops.native_available():     # the kernel's own table, every id
        for v, (tm, tn) in ops._GEMM_TILES.items():
            assert (ops._hip.gemm_planes_tile(v, 0), ops._hip.gemm_planes_tile(v, 1)) == (tm, tn)
        assert ops._hip.gemm_planes_tile(len(ops._GEMM_TILES), 0) == 0
