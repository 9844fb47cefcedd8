"""loess.hip through ops.loess against the float64 reference (ops.reference.loess), which
tests/test_loess_cpu.py ties to the direct fit of models/pp.py.

Window starts and the sort order are integers and are compared exactly.  Fitted values are
compared at 1e-11 * max(1, max|y|): the kernel and the reference add the same products in a
different order (64 strided lane sums and a butterfly against numpy's pairwise sum), which
was modelled at 5.4e-14 of max|y| on these series, and every semantic mistake (no ridge, no
1.0000001 factor on h, a window off by one, ``<=`` for ``<`` on ties) moves the fit by
6.7e-11 of max|y| or more.

Largest deviation observed on an MI355X over all cases of this file: 8.4e-14 absolute,
1.9e-14 of max|y| (the near-tie series at degree 2); 4.8e-14 (1.1e-14 of max|y|) on the
sampled positions of the 30,000-point series, which used 44 bytes per point."""
import numpy as np
import pytest
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.models import pp
from cnmf_torch_amd.ops import reference
from loess_cases import HVG_TOP, ISSUE_SERIES, hvg_adata, series, tol

pytestmark = pytest.mark.gpu

_seen = {"rel": 0.0}

# n = 63, 64, 65: k < 64, most lanes idle; 640: k = 192, three full trips; 700 (smooth):
# k = 210, a ragged last trip; 214: k = 65, one full trip and one element
SHAPES = ("n63", "n64", "n65", "n640", "n214")


def _check(x, y, what, offsets=None, degree=2):
    want, starts, order = reference.loess(x, y, offsets=offsets, degree=degree,
                                          return_windows=True)
    got, gs, go = ops.loess(torch.tensor(x).cuda(), torch.tensor(y).cuda(), offsets=offsets,
                            degree=degree, return_windows=True)
    assert got.is_cuda and got.dtype == torch.float64
    assert np.array_equal(go.cpu().numpy(), order), what
    assert np.array_equal(gs.cpu().numpy(), starts), what
    d = float(np.abs(got.cpu().numpy() - want).max()) if want.size else 0.0
    rel = d / max(1.0, float(np.abs(y).max())) if want.size else 0.0
    _seen["rel"] = max(_seen["rel"], rel)
    print(f"{what}: max |fit - reference| = {d:.3e}, {rel:.3e} of max|y| "
          f"(largest so far {_seen['rel']:.3e})")
    assert d <= tol(y), (what, d)
    return got


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", ISSUE_SERIES + SHAPES)
def test_matches_reference(name, degree):
    x, y = series(name)
    _check(x, y, f"{name} degree {degree}", degree=degree)


@pytest.mark.parametrize("degree", [1, 2])
def test_one_ragged_launch_of_four_series(degree):
    parts = [series("n1"), series("n65"), series("smooth")]
    x = np.concatenate([p[0] for p in parts])
    y = np.concatenate([p[1] for p in parts])
    off = np.array([0, 1, 1, 66, 766])                      # lengths 1, 0, 65, 700
    got = _check(x, y, f"ragged degree {degree}", offsets=off, degree=degree)
    # a series fitted alone gives the same bits as inside the ragged launch
    alone = ops.loess(torch.tensor(parts[2][0]).cuda(), torch.tensor(parts[2][1]).cuda(),
                      degree=degree)
    assert torch.equal(got[66:], alone)


def test_two_runs_give_the_same_bits():
    for name in ("smooth", "ties"):
        x, y = series(name)
        xd, yd = torch.tensor(x).cuda(), torch.tensor(y).cuda()
        assert torch.equal(ops.loess(xd, yd), ops.loess(xd, yd))


def test_cuda_input_runs_the_kernel_not_the_reference(monkeypatch):
    monkeypatch.delenv("CNMF_FORCE_TORCH_OPS", raising=False)
    ops.refresh_env()
    x, y = series("n214")
    want = reference.loess(x, y)

    def boom(*a, **k):
        raise AssertionError("the reference ran on a CUDA tensor")

    monkeypatch.setattr(reference, "loess", boom)
    got = ops.loess(torch.tensor(x).cuda(), torch.tensor(y).cuda())
    assert got.is_cuda and float(np.abs(got.cpu().numpy() - want).max()) <= tol(y)


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(ops._hip, "loess_windows", boom, raising=True)
    monkeypatch.setattr(ops._hip, "loess_fit", boom, raising=True)
    x, y = series("n64")
    xd, yd = torch.tensor(x).cuda(), torch.tensor(y).cuda()
    two = torch.stack([xd, xd], dim=1)
    for args, kw in (((xd.float(), yd.float()), {}),
                     ((xd, yd.float()), {}),
                     ((two[:, 0], yd), {}),                  # not contiguous
                     ((xd, torch.tensor(y)), {}),            # CPU and GPU mixed
                     ((torch.tensor(x), yd), {}),
                     ((xd, yd), {"degree": 3}),
                     ((xd, yd), {"offsets": np.array([0, 30, 65])}),     # past the end
                     ((xd, yd), {"offsets": np.array([0, 40, 30, 64])}),
                     ((xd, yd[:63]), {})):
        with pytest.raises(ValueError):
            ops.loess(*args, **kw)


def test_30000_points_stay_under_1_kb_per_point():
    n = 30000
    rs = np.random.default_rng(11)
    c = rs.poisson(rs.gamma(0.3, 20.0, n)) + 1               # count-like means: many ties
    x = np.log10(c / 5000.0)
    y = 1.3 * x + 0.1 * x * x + 0.2 * rs.normal(size=n)
    xd, yd = torch.tensor(x).cuda(), torch.tensor(y).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    got = ops.loess(xd, yd)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    print(f"n = {n}: {used} bytes over the call, {used / n:.1f} per point")
    assert used < 1024 * n
    # against the reference on 200 positions of the sorted series only
    order = np.argsort(x, kind="stable")
    xs, ys = x[order], y[order]
    k = reference.loess_k(n, 0.3, 2)
    pos = np.unique(np.r_[0, n - 1, rs.integers(0, n, 198)])
    starts = reference.loess_windows(xs, k)
    want = reference._loess_sorted(xs, ys, k, starts, 2, 64, points=pos)
    d = float(np.abs(got.cpu().numpy()[order][pos] - want).max())
    rel = d / max(1.0, float(np.abs(y).max()))
    _seen["rel"] = max(_seen["rel"], rel)
    print(f"n = {n}: max |fit - reference| on {pos.size} positions = {d:.3e}, {rel:.3e} of "
          f"max|y|")
    assert d <= tol(y)


def test_hvg_on_resident_counts_matches_cpu_direct():
    from cnmf_torch_amd.ops import sparse as sops

    direct = pp.highly_variable_genes(hvg_adata(), n_top_genes=HVG_TOP, inplace=False)
    ad = hvg_adata()
    dX = sops.DeviceCSR.from_scipy(ad.X, torch.device("cuda"))
    native = pp.highly_variable_genes(ad, n_top_genes=HVG_TOP, inplace=False, device_csr=dX,
                                      loess="native")
    np.testing.assert_allclose(native["variances_norm"].values,
                               direct["variances_norm"].values, rtol=1e-9, atol=0)
    assert np.array_equal(native["highly_variable"].values, direct["highly_variable"].values)
    # batches: host statistics, one ragged fit on the device of the counts
    direct_b = pp.highly_variable_genes(hvg_adata(), n_top_genes=HVG_TOP, inplace=False,
                                        batch_key="batch")
    native_b = pp.highly_variable_genes(hvg_adata(), n_top_genes=HVG_TOP, inplace=False,
                                        batch_key="batch", loess="native", device="cuda")
    np.testing.assert_allclose(native_b["variances_norm"].values,
                               direct_b["variances_norm"].values, rtol=1e-9, atol=0)
    assert np.array_equal(native_b["highly_variable"].values,
                          direct_b["highly_variable"].values)
