"""The float64 LOESS reference (ops.reference.loess, also the CPU path of ops.loess and the
oracle of loess.hip) against the direct fit of models/pp.py ``loess_fit``, and the
``loess=`` / ``hvg_loess=`` switches of the HVG selection.

Fitted values are compared at 1e-11 * max(1, max|y|): a 64-lane strided sum followed by a
tree differs from the direct fit by at most 5.4e-14 of max|y| on these series, and every
semantic mistake (no ridge, no 1.0000001 factor on h, a window off by one, ``<=`` for ``<``
on ties) moves the fit by 6.7e-11 of max|y| or more."""
import numpy as np
import pytest
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.models import pp
from cnmf_torch_amd.ops import reference
from cnmf_torch_amd.preprocess import Preprocess
from loess_cases import (HVG_TOP, ISSUE_SERIES, hvg_adata, series, sliding_starts, tol)


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", ISSUE_SERIES)
def test_windows_equal_the_sliding_loop(name, degree):
    x, _ = series(name)
    xs = np.sort(x, kind="stable")
    k = reference.loess_k(xs.shape[0], 0.3, degree)
    got = reference.loess_windows(xs, k)
    assert got.dtype == np.int64
    assert np.array_equal(got, sliding_starts(xs, k))


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", ISSUE_SERIES)
def test_reference_matches_direct_fit(name, degree):
    x, y = series(name)
    got = reference.loess(x, y, degree=degree)
    want = pp.loess_fit(x, y, degree=degree, backend="direct")
    d = float(np.abs(got - want).max())
    print(f"{name} degree {degree}: max |reference - direct| = {d:.3e} (tol {tol(y):.3e})")
    assert got.dtype == np.float64 and d <= tol(y)


def test_ragged_offsets_give_the_per_series_bits():
    parts = [series(nm) for nm in ("n1", "n7", "ties", "n65", "smooth")]
    lens = [1, 0, 7, 900, 0, 65, 700]                 # two empty series among them
    x = np.concatenate([p[0] for p in parts])
    y = np.concatenate([p[1] for p in parts])
    off = np.concatenate([[0], np.cumsum(lens)])
    for degree in (1, 2):
        got, starts, order = reference.loess(x, y, offsets=off, degree=degree,
                                             return_windows=True)
        a = 0
        for px, py in parts:
            one, s1, o1 = reference.loess(px, py, degree=degree, return_windows=True)
            b = a + px.shape[0]
            assert np.array_equal(got[a:b], one)
            assert np.array_equal(starts[a:b], s1) and np.array_equal(order[a:b], a + o1)
            a = b


@pytest.mark.parametrize("name", ["smooth", "ties", "near", "n7"])
def test_result_does_not_depend_on_block(name):
    x, y = series(name)
    for degree in (1, 2):
        base = reference.loess(x, y, degree=degree)
        for block in (1, 7, 64, 10 ** 6):
            assert np.array_equal(base, reference.loess(x, y, degree=degree, block=block))


def test_op_on_cpu_tensors_is_the_reference():
    x, y = series("ties")
    got, starts, order = ops.loess(torch.tensor(x), torch.tensor(y), return_windows=True)
    want, s, o = reference.loess(x, y, return_windows=True)
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want)
    assert np.array_equal(starts.numpy(), s) and np.array_equal(order.numpy(), o)
    fit = pp.loess_fit(x, y, backend="native", device="cpu")
    assert np.array_equal(fit, want)


def test_bad_arguments_raise():
    x, y = series("n7")
    with pytest.raises(ValueError):
        reference.loess(x, y, degree=3)
    bad = x.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError):
        reference.loess(bad, y)
    with pytest.raises(ValueError):
        reference.loess(x, bad)
    for off in ([0, 5, 3, 7], [0, 3, 8], [1, 7], [0, 3]):
        with pytest.raises(ValueError):
            reference.loess(x, y, offsets=np.array(off))
    with pytest.raises(ValueError):
        ops.loess(torch.tensor(x), torch.tensor(y), degree=3)
    with pytest.raises(ValueError):
        ops.loess(torch.tensor(x).float(), torch.tensor(y).float())
    with pytest.raises(ValueError):
        pp.loess_fit(x, y, backend="fast")


@pytest.mark.parametrize("batch_key", [None, "batch"])
@pytest.mark.parametrize("sparse", [True, False])
def test_hvg_native_matches_direct(batch_key, sparse):
    direct = pp.highly_variable_genes(hvg_adata(sparse), n_top_genes=HVG_TOP,
                                      batch_key=batch_key, inplace=False)
    native = pp.highly_variable_genes(hvg_adata(sparse), n_top_genes=HVG_TOP,
                                      batch_key=batch_key, inplace=False, loess="native",
                                      device="cpu")
    # the comparison of the masks means something only if the cut-off is not a tie
    nv = np.sort(direct["variances_norm"].values)[::-1]
    gap = (nv[HVG_TOP - 1] - nv[HVG_TOP]) / nv[HVG_TOP - 1]
    print(f"relative gap at the cut-off rank: {gap:.3e}")
    assert gap > 1e-6
    assert direct["highly_variable"].sum() == HVG_TOP
    assert (direct["variances_norm"].values[[5, 17, 40, 41]] == 0).all()
    np.testing.assert_allclose(native["variances_norm"].values,
                               direct["variances_norm"].values, rtol=1e-9, atol=0)
    assert np.array_equal(native["highly_variable"].values, direct["highly_variable"].values)
    assert np.array_equal(native["highly_variable_nbatches"].values,
                          direct["highly_variable_nbatches"].values)


def test_hvg_rejects_unknown_loess():
    with pytest.raises(ValueError):
        pp.highly_variable_genes(hvg_adata(), n_top_genes=HVG_TOP, loess="skmisc")


def test_normalize_batchcorrect_hvg_loess():
    p = Preprocess(random_seed=0)
    _, hv_default = p.normalize_batchcorrect(hvg_adata(), n_top_genes=HVG_TOP, makeplots=False,
                                             device="cpu")
    _, hv_native = p.normalize_batchcorrect(hvg_adata(), n_top_genes=HVG_TOP, makeplots=False,
                                            device="cpu", hvg_loess="native")
    assert len(hv_default) == HVG_TOP and list(hv_native) == list(hv_default)
    with pytest.raises(ValueError):
        p.normalize_batchcorrect(hvg_adata(), n_top_genes=HVG_TOP, makeplots=False,
                                 device="cpu", hvg_loess="fast")
    with pytest.raises(ValueError):
        p.preprocess_for_cnmf(hvg_adata(), n_top_rna_genes=HVG_TOP, makeplots=False,
                              device="cpu", hvg_loess="fast")
