"""mi_cd.hip through ops.mi_cd against the float64 reference (ops.reference.mi_cd) on
hand-built input; scikit-learn is not involved (tests/test_mi_cpu.py ties the reference to
it).

The neighbour counts ``m`` are integers and are compared exactly.  ``mi`` is compared to
1e-11 absolute: both sides add the same digamma table values, so only the order of a float64
sum of <= 5,000 terms of size <= psi(5,000) ~ 8.5 differs, which is bounded by
(n - 1) * 2^-53 * 8.5 ~ 4.7e-12 on each side.

Largest distance observed on an MI355X over all cases of this file: 2.7e-15 in ``mi``
(4.4e-16 for select_features_MI, GPU against CPU), 0 in ``m``."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.ops import reference

pytestmark = pytest.mark.gpu

TOL = 1e-11
_seen = {"mi": 0.0}


def _codes(n, layout, seed):
    """Class codes (n,) in a fixed shuffled order."""
    rs = np.random.default_rng(seed)
    if layout == "one" or n < 32:
        return np.zeros(n, dtype=np.int64)
    if layout == "singletons":
        return rs.permutation(n).astype(np.int64)
    # classes of 1 (dropped), 2, 3, 4 and the rest in classes of >= 8 points
    small = np.repeat([0, 1, 2, 3], [1, 2, 3, 4])
    rest = n - small.size
    big = 4 + (np.arange(rest) % max(1, min(3, rest // 8)))
    return np.concatenate([small, big]).astype(np.int64)[rs.permutation(n)]


def _features(n, F, codes, seed):
    """Columns cycling through: continuous with a class shift; integer-valued (exact ties,
    r = 0); mostly zeros under noise of the prepared scale; all equal."""
    rs = np.random.default_rng(seed + 1)
    X = np.empty((n, F), dtype=np.float64)
    for f in range(F):
        kind = f % 4
        if kind == 0:
            X[:, f] = rs.normal(size=n) + 0.7 * codes
        elif kind == 1:
            X[:, f] = rs.integers(0, 5, n) + (codes % 2)
        elif kind == 2:
            X[:, f] = rs.gamma(2.0, 1.0, n) * (rs.random(n) > 0.7) + 1e-10 * rs.normal(size=n)
        else:
            X[:, f] = 2.5
    return X


@functools.lru_cache(maxsize=None)
def _case(n, F, layout, n_neighbors, seed=0):
    codes = _codes(n, layout, seed)
    X = _features(n, F, codes, seed)
    mi, m = reference.mi_cd(X, codes, n_neighbors)
    for a in (codes, X, mi, m):
        a.setflags(write=False)
    return codes, X, mi, m


def _check(X, codes, n_neighbors, mi, m, what, **kw):
    got, gm = ops.mi_cd(torch.tensor(X).cuda(), codes, n_neighbors, return_counts=True,
                        **kw)
    assert gm.is_cuda and gm.dtype == torch.int32
    gm = gm.cpu().numpy()
    assert np.array_equal(gm, m), (what, np.argwhere(gm != m)[:5])
    d = float(np.abs(got.cpu().numpy() - mi).max()) if mi.size else 0.0
    _seen["mi"] = max(_seen["mi"], d)
    print(f"{what}: max |mi - reference| = {d:.3e} (largest so far {_seen['mi']:.3e})")
    assert d <= TOL, (what, d)
    return got


@pytest.mark.parametrize("F", [1, 5, 16])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 257, 1000, 5000])
def test_mixed_classes_match_reference(n, F):
    for k in (1, 3, 8):
        codes, X, mi, m = _case(n, F, "mixed", k)
        _check(X, codes, k, mi, m, f"mixed n={n} F={F} k={k}")


@pytest.mark.parametrize("n_neighbors", [1, 3, 8])
def test_one_class_only(n_neighbors):
    codes, X, mi, m = _case(300, 5, "one", n_neighbors)
    _check(X, codes, n_neighbors, mi, m, f"one class k={n_neighbors}")
    assert (m[:, 3] == 300).all()            # the all-equal column counts every point


def test_every_row_a_singleton():
    codes, X, mi, m = _case(65, 5, "singletons", 3)
    assert (mi == 0).all() and (m == 0).all()
    got = _check(X, codes, 3, mi, m, "singletons")
    assert (got == 0).all()


@pytest.mark.parametrize("n_neighbors", [1, 3, 8])
def test_class_of_8_spans_half_of_4000_points(n_neighbors):
    """A class of 8 spread evenly over 4,000 sorted points, its first and last members at the
    two ends of the array: at k = 3 the radius covers about half the array (far beyond one
    256-point tile), and the searches run into both array ends."""
    n = 4000
    rs = np.random.default_rng(7)
    codes = 1 + (np.arange(n) % 3)
    codes[np.linspace(0, n - 1, 8).astype(int)] = 0          # positions in sorted order
    vals = np.sort(rs.normal(size=n))
    shuffle = rs.permutation(n)
    X = np.stack([vals[shuffle], np.round(vals * 2.0)[shuffle]], axis=1)
    codes = codes[shuffle]
    mi, m = reference.mi_cd(X, codes, n_neighbors)
    if n_neighbors == 3:
        assert m[codes == 0, 0].min() > n // 4 and m[codes == 0, 0].max() > n // 2
    if n_neighbors == 8:
        assert m[codes == 0, 0].max() >= n - 1               # k = 7: end to end
    _check(X, codes, n_neighbors, mi, m, f"class of 8 in 4000, k={n_neighbors}")


def test_feature_blocks_and_repeats_give_the_same_bits():
    codes, X, mi, m = _case(1000, 16, "mixed", 3)
    Xd = torch.tensor(X).cuda()
    one = ops.mi_cd(Xd, codes, 3)
    again = ops.mi_cd(Xd, codes, 3)
    by3, m3 = ops.mi_cd(Xd, codes, 3, return_counts=True, feature_block=3)
    by1 = ops.mi_cd(Xd, codes, 3, feature_block=1)
    assert torch.equal(one, again)
    assert torch.equal(one, by3) and torch.equal(one, by1)
    assert np.array_equal(m3.cpu().numpy(), m)


def test_cuda_input_runs_the_kernel_not_the_reference(monkeypatch):
    monkeypatch.delenv("CNMF_FORCE_TORCH_OPS", raising=False)
    ops.refresh_env()

    def boom(*a, **k):
        raise AssertionError("the reference ran on a CUDA tensor")

    codes, X, mi, m = _case(257, 5, "mixed", 3)
    monkeypatch.setattr(reference, "mi_cd", boom)
    got, gm = ops.mi_cd(torch.tensor(X).cuda(), codes, 3, return_counts=True)
    assert got.is_cuda and gm.is_cuda
    assert np.array_equal(gm.cpu().numpy(), m)


def test_op_rejects_bad_input_on_the_gpu():
    codes, X, _, _ = _case(64, 5, "mixed", 3)
    Xd = torch.tensor(X).cuda()
    with pytest.raises(ValueError):
        ops.mi_cd(Xd, codes, n_neighbors=9)
    with pytest.raises(ValueError):
        ops.mi_cd(Xd.float(), codes)
    bad = Xd.clone()
    bad[5, 0] = float("nan")
    with pytest.raises(ValueError):
        ops.mi_cd(bad, codes)


def test_select_features_native_gpu_matches_cpu():
    from cnmf_torch_amd.preprocess import Preprocess
    from cnmf_torch_amd.utils.anndata_lite import AnnData
    from cnmf_torch_amd.utils.synthetic import simulate_counts

    def run(device):
        Xc, cells, genes = simulate_counts(300, 40, 3, seed=2, sparse=False)
        labels = np.random.default_rng(1).integers(0, 4, 300)
        ad = AnnData(X=Xc.astype(np.float64), var=pd.DataFrame(index=genes),
                     obs=pd.DataFrame(index=cells))
        return Preprocess(random_seed=0).select_features_MI(
            ad, labels, n_top_features=10, makeplots=False, backend="native", device=device)

    cpu, gpu = run("cpu"), run("cuda")
    d = float(np.abs(gpu.var["MI"].values - cpu.var["MI"].values).max())
    print(f"select_features_MI native: max |gpu - cpu| = {d:.3e}")
    assert d <= TOL
    assert cpu.var["MI"].values.max() > 0
    assert gpu.var["highly_variable"].sum() == cpu.var["highly_variable"].sum() == 10
