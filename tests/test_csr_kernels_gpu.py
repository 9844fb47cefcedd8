"""The HIP kernels of csrc/kernels/sparse.hip against the float64 oracle of csr_cases.py at
their tile, wave, trip, block-cap and rank edges (test_csr_kernels_cpu.py runs the same
cases through the torch paths).  Every check first asserts ``ops.use_native`` on its GPU
input, so a fallback to torch fails the test; the tolerances are derived in csr_cases.py,
one comment per assertion.

Edges reached (kernel constant -> case id):
  csr_col_stats  kCsTile = 1536: colstats-nout{1535,1536,1537}, third tile colstats-nout3073,
                 entries in columns 1535|1536 and 3071|3072 (rows 3, 4 of those cases);
                 kCsU = 4 second trip and its partial tail: the 257- and 513-entry rows of
                 rows-n* and colstats-nout*; 64 rows per block: colstats-n{63,64,65};
                 512-block cap with blocks that own no rows: colstats-n33000.
  csr_tspmm      KB = 16/32/64 edges and the 64-column blocks: tspmm-K{16,17,32,33,64,65,130};
                 tile width tc = 4608 // K: tspmm-K{7,17,64}-{tc-1,tc,tc+1,2tc+1};
                 256-block cap: tspmm-n66000; the four <data, B> types: tspmm-f{32,64}-B{32,64}.
  csr_spmm       the same K list with float32 and float64 data (K = 64: every lane stores).
  radix_hist     second grid-stride trip: radix-m1048833; ties across the rank, low-byte
                 differences, denormals, +inf, an all-dropped input, a stored -0.0.
"""
import numpy as np
import pytest
import torch

import csr_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = {"f32": torch.float32, "f64": torch.float64}


@pytest.mark.parametrize("n", [1, 3, 4, 5, 130], ids=lambda n: f"rows-n{n}")
def test_every_op_at_row_lengths(n):
    cc.check_all_ops(cc.rows_case(n), DEV)


@pytest.mark.parametrize("mapped", [False, True], ids=["nomap", "map"])
@pytest.mark.parametrize("n_out", [1, 1535, 1536, 1537, 3073], ids=lambda v: f"colstats-nout{v}")
def test_col_stats_tile_edges(n_out, mapped):
    case = cc.colstats_nout_case(n_out, mapped)
    cc.check_col_stats(case, DEV)
    cc.check_mean_var(case, DEV)


@pytest.mark.parametrize("n", [63, 64, 65, 33000], ids=lambda v: f"colstats-n{v}")
def test_col_stats_block_edges(n):
    case = cc.colstats_n_case(n)
    cc.check_col_stats(case, DEV)
    cc.check_mean_var(case, DEV, ddof=1)


def test_col_stats_explicit_center():
    case = cc.rows_case(130)
    center = np.linspace(-2.0, 3.0, case.n_out) + 0.125
    cc.check_col_stats(case, DEV, center=center)


def test_mean_var_large_mean_and_constant_column():
    case = cc.special_case()
    cc.check_col_stats(case, DEV)
    for ddof in (0, 1):
        cc.check_mean_var(case, DEV, ddof=ddof)
    mean, var = cc.sops.mean_var(case.csr(DEV))
    assert float(var[2]) == 0.0 and float(mean[2]) == 3.0      # constant column: exactly 0
    assert float(var[9]) == 0.0 and float(mean[9]) == 0.0      # empty column
    assert float(var[5]) > 0.0                                 # mean = 1.2e6 std


@pytest.mark.parametrize("K", cc.K_LIST, ids=lambda k: f"tspmm-K{k}")
def test_tspmm_rank_edges(K):
    cc.check_tspmm(cc.rows_case(130), DEV, K)


@pytest.mark.parametrize("which", ["tc-1", "tc", "tc+1", "2tc+1"])
@pytest.mark.parametrize("K", [7, 17, 64], ids=lambda k: f"tspmm-K{k}")
def test_tspmm_tile_edges(K, which):
    cc.check_tspmm(cc.tspmm_tile_case(K, which), DEV, K)


def test_tspmm_block_cap_n66000():
    cc.check_tspmm(cc.tspmm_cap_case(), DEV, 7)


@pytest.mark.parametrize("b", ["B32", "B64"])
@pytest.mark.parametrize("data", ["float32", "float64"], ids=["tspmm-f32", "tspmm-f64"])
def test_tspmm_dtypes(data, b):
    cc.check_tspmm(cc.rows_case(130, dtype=data), DEV, 17,
                   b_dtype=np.float32 if b == "B32" else np.float64)


@pytest.mark.parametrize("data", ["float32", "float64"], ids=["f32", "f64"])
@pytest.mark.parametrize("K", cc.K_LIST, ids=lambda k: f"spmm-K{k}")
def test_spmm_rank_edges(K, data):
    cc.check_spmm(cc.rows_case(130, dtype=data), DEV, K)      # unsorted col_map, col_div, ...


@pytest.mark.parametrize("pair", ["f32-f32", "f32-f64", "f64-f32", "f64-f64"])
@pytest.mark.parametrize("col_map", ["nomap", "subset", "perm", "alldropped"])
@pytest.mark.parametrize("factor", ["none", "row_scale", "row_scale+round", "round_only",
                                    "col_div", "clip", "max_finite", "max_inf", "all"])
def test_transform_densify_factors(factor, col_map, pair):
    i, o = pair.split("-")
    case = cc.factor_case(factor, col_map, {"f32": "float32", "f64": "float64"}[i])
    cc.check_transform(case, DEV, F[o])
    cc.check_densify(case, DEV, F[o])
    if col_map == "alldropped":
        cc.check_col_stats(case, DEV)                          # counts (and sums) all 0


def test_round_mid_without_row_scale_is_no_transform():
    a = cc.factor_case("round_only", "nomap", "float64")
    b = cc.factor_case("none", "nomap", "float64")
    A = a.csr(DEV)
    assert torch.equal(cc.sops.transform(A, out_dtype=torch.float64, round_mid=True),
                       cc.sops.transform(b.csr(DEV), out_dtype=torch.float64))
    assert torch.equal(cc.sops.transform(A, out_dtype=torch.float64, round_mid=True), A.data)


@pytest.mark.parametrize("name", cc.RADIX_NAMES, ids=lambda s: f"radix-{s}")
def test_kth_nonneg(name):
    cc.check_kth(name, DEV)


@pytest.mark.parametrize("name", cc.RADIX_NAMES[:-1], ids=lambda s: f"quantile-{s}")
def test_quantile_with_zeros(name):
    cc.check_quantile(name, DEV)


@pytest.mark.parametrize("which", ["norows", "nonnz"], ids=lambda s: f"empty-{s}")
def test_empty_input_gives_exact_zeros(which):
    cc.check_empty(cc.empty_case(which), DEV)
