"""The float64 reference of the mutual-information estimator (ops.reference.mi_prepare /
mi_cd) against scikit-learn's mutual_info_classif, and the ``backend`` switch of
Preprocess.select_features_MI on the CPU.

Tolerance against scikit-learn: 1e-12 absolute (the two can differ by the order of float64
means of digamma values, below 1e-15; with the means taken in row order as scikit-learn
takes them the difference seen in these cases is 0).  Every non-singleton
class has >= 8 members, where scikit-learn's neighbour search takes its tree path; classes
of 3 to 7 points go through its brute-force path, whose cancellation the reference does not
imitate (docs/ARCHITECTURE.md "Mutual information").
"""
import numpy as np
import pandas as pd
import pytest
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.ops import reference
from cnmf_torch_amd.preprocess import Preprocess
from cnmf_torch_amd.utils.anndata_lite import AnnData
from cnmf_torch_amd.utils.synthetic import simulate_counts

TOL = 1e-12


def _case(n, G, n_classes, zero_frac, seed, singleton=False):
    """Class-dependent gamma features with a share of exact zeros; every class >= 8 rows."""
    rs = np.random.default_rng(seed)
    y = rs.integers(0, n_classes, n)
    y[:8 * n_classes] = np.repeat(np.arange(n_classes), 8)
    if singleton:
        y[-1] = n_classes
    shift = 1.0 + 2.0 * rs.random((n_classes + 1, G)) * (np.arange(G) % 3 > 0)
    X = rs.gamma(2.0, 1.0, (n, G)) * shift[y] * (rs.random((n, G)) >= zero_frac)
    sizes = np.bincount(y)
    assert ((sizes >= 8) | (sizes <= 1)).all()
    return X, y


def _brute_m(Xp, codes, n_neighbors):
    """m by definition, O(n^2): the k-th same-class distance, nextafter, squared count."""
    n, G = Xp.shape
    keep = np.bincount(codes)[codes] > 1
    m = np.zeros((n, G), dtype=np.int32)
    for f in range(G):
        c = Xp[:, f]
        for i in np.flatnonzero(keep):
            same = keep & (codes == codes[i])
            d = np.sort(np.abs(c[same] - c[i]))         # d[0] is the point itself
            rad = np.nextafter(d[min(n_neighbors, same.sum() - 1)], 0.0)
            dd = c[keep] - c[i]
            m[i, f] = np.sum(dd * dd <= rad * rad)
    return m


@pytest.mark.parametrize("n,G,n_classes,zero_frac,seed,singleton",
                         [(3000, 12, 7, 0.7, 3, False), (500, 8, 5, 0.5, 1, True)])
def test_reference_matches_sklearn(n, G, n_classes, zero_frac, seed, singleton):
    from sklearn.feature_selection import mutual_info_classif

    X, y = _case(n, G, n_classes, zero_frac, seed, singleton)
    want = mutual_info_classif(X, y, discrete_features="auto", n_neighbors=3, copy=True,
                               random_state=seed)
    assert want.max() > 0.05                 # the labels carry information
    codes = np.unique(y, return_inverse=True)[1]
    mi, m = reference.mi_cd(reference.mi_prepare(X, seed), codes, 3)
    diff = np.abs(np.maximum(mi, 0.0) - want).max()
    print(f"n={n} G={G}: max |reference - sklearn| = {diff:.3e}")
    assert diff <= TOL
    if singleton:
        assert (m[-1] == 0).all() and (m[:-1] > 0).all()


def test_prepare_equals_sklearn_bits():
    from sklearn.preprocessing import scale

    X, _ = _case(500, 8, 5, 0.5, 1)
    X[:, 2] = 4.0                            # a constant column: its std is replaced by 1
    # as _estimate_mi writes it: the statistics are taken on X[:, mask], a column-major copy
    mask = np.ones(X.shape[1], dtype=bool)
    want = X.astype(np.float64, copy=True)
    want[:, mask] = scale(want[:, mask], with_mean=False, copy=False)
    means = np.maximum(1, np.mean(np.abs(want[:, mask]), axis=0))
    want[:, mask] += 1e-10 * means * np.random.RandomState(11).standard_normal(size=want.shape)
    assert np.array_equal(reference.mi_prepare(X, 11), want)
    assert np.array_equal(reference.mi_prepare(X, 11, row_block=64), want)
    assert np.array_equal(reference.mi_prepare(X, 11, row_block=10 ** 6), want)
    assert np.array_equal(reference.mi_prepare(X.astype(np.float32), 11),
                          reference.mi_prepare(X.astype(np.float32).astype(np.float64), 11))


@pytest.mark.parametrize("n_neighbors", [1, 3, 8])
def test_reference_counts_match_the_definition(n_neighbors):
    rs = np.random.default_rng(4)
    n = 90
    codes = np.r_[np.zeros(40), np.ones(30), np.full(9, 2), 3, 3, 4, 4, 4, 5, 5, 5, 5,
                  6, 7].astype(np.int64)[rs.permutation(n)]
    Xp = np.stack([rs.normal(size=n), rs.integers(0, 4, n).astype(np.float64),
                   np.ones(n)], axis=1)     # continuous, exact ties (r = 0), all equal
    mi, m = reference.mi_cd(Xp, codes, n_neighbors)
    assert np.array_equal(m, _brute_m(Xp, codes, n_neighbors))
    assert (m[np.bincount(codes)[codes] == 1] == 0).all()
    assert (m[np.bincount(codes)[codes] > 1, 2] == 88).all()    # all equal: every kept point
    # the op on CPU tensors is the reference
    got, gm = ops.mi_cd(torch.from_numpy(Xp), codes, n_neighbors, return_counts=True)
    assert np.array_equal(got.numpy(), mi) and np.array_equal(gm.numpy(), m)


def test_all_singletons_give_zero():
    Xp = np.random.default_rng(0).normal(size=(7, 3))
    mi, m = reference.mi_cd(Xp, np.arange(7), 3)
    assert (mi == 0).all() and (m == 0).all()


def test_op_rejects_bad_input():
    Xp = torch.from_numpy(np.random.default_rng(0).normal(size=(20, 2)))
    codes = np.arange(20) % 2
    for k in (0, 9):
        with pytest.raises(ValueError):
            ops.mi_cd(Xp, codes, n_neighbors=k)
    with pytest.raises(ValueError):
        ops.mi_cd(Xp.float(), codes)
    bad = Xp.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError):
        ops.mi_cd(bad, codes)
    bad[3, 1] = float("inf")
    with pytest.raises(ValueError):
        ops.mi_cd(bad, codes)
    with pytest.raises(ValueError):
        ops.mi_cd(Xp, codes[:-1])


def _mi_input():
    """The 200 x 60 input of test_preprocess.test_select_features_mi, built anew for every
    call: the method's normalisation works on the matrix it is given."""
    Xc, cells, genes = simulate_counts(200, 60, 3, seed=5, sparse=False)
    labels = np.random.default_rng(0).integers(0, 3, 200)
    assert np.bincount(labels).min() >= 8
    ad = AnnData(X=Xc.astype(np.float64), var=pd.DataFrame(index=genes),
                 obs=pd.DataFrame(index=cells))
    return ad, labels


def test_native_backend_matches_sklearn_backend():
    p = Preprocess(random_seed=0)
    ad, labels = _mi_input()
    want = p.select_features_MI(ad, labels, n_top_features=10, makeplots=False)
    ad, labels = _mi_input()
    got = p.select_features_MI(ad, labels, n_top_features=10, makeplots=False,
                               backend="native", device="cpu")
    assert list(got.var.columns) == list(want.var.columns)
    assert list(got.var.index) == list(want.var.index)
    diff = np.abs(got.var["MI"].values - want.var["MI"].values).max()
    print(f"max |native - sklearn| MI per gene = {diff:.3e}")
    assert diff <= TOL
    assert got.var["highly_variable"].sum() == want.var["highly_variable"].sum() == 10


def test_default_backend_is_the_direct_sklearn_call():
    from sklearn.feature_selection import mutual_info_classif

    from cnmf_torch_amd.models import pp
    from cnmf_torch_amd.preprocess import stdscale_quantile_celing
    from cnmf_torch_amd.utils.anndata_lite import to_lite

    ad, labels = _mi_input()
    out = Preprocess(random_seed=0).select_features_MI(ad, labels, n_top_features=10,
                                                       makeplots=False)
    ad, labels = _mi_input()
    pre = stdscale_quantile_celing(pp.normalize_total(to_lite(ad)), max_value=None,
                                   quantile_thresh=.9999)
    want = mutual_info_classif(pre.X, labels, discrete_features="auto", n_neighbors=3,
                               copy=True, random_state=0)
    assert np.array_equal(out.var["MI"].values, want)


def test_bad_backend_and_neighbours_raise():
    from cnmf_torch_amd.models.mi import mutual_info_classif_native

    ad, labels = _mi_input()
    with pytest.raises(ValueError):
        Preprocess(random_seed=0).select_features_MI(ad, labels, makeplots=False,
                                                     backend="torch")
    with pytest.raises(ValueError):
        mutual_info_classif_native(np.asarray(ad.X), labels, n_neighbors=9, device="cpu")
