"""Inputs shared by test_loess_cpu.py and test_loess_gpu.py: the (x, y, degree) series the
LOESS reference and loess.hip are checked on, and the count matrix of the HVG tests."""
import functools

import numpy as np
import pandas as pd
import scipy.sparse as sp

RTOL = 1e-11        # fitted values: RTOL * max(1, max|y|)


def tol(y) -> float:
    return RTOL * max(1.0, float(np.abs(y).max())) if len(y) else RTOL


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def series(name: str):
    """(x, y) float64 in a fixed shuffled order."""
    rs = np.random.default_rng(sum(map(ord, name)))
    if name == "smooth":                      # log10 of gamma(0.3) means, quadratic trend
        x = np.log10(rs.gamma(0.3, 1.0, 700) + 1e-4)
        y = 0.15 * x * x + 1.2 * x + 0.3 + 0.1 * rs.normal(size=700)
    elif name == "ties":                      # count-like means c / 200
        x = np.log10((rs.poisson(1.5, 900) + 1) / 200.0)
        y = 1.1 * x + 0.2 * rs.normal(size=900)
    elif name == "equal":
        x = np.full(50, -1.5)
        y = rs.normal(size=50)
    elif name == "near":                      # 300 points within 1e-13 of -2, 100 normal
        x = np.concatenate([-2.0 + 1e-13 * rs.random(300), rs.normal(size=100) - 2.0])
        x = x[rs.permutation(400)]
        y = x + 0.1 * rs.normal(size=400)
    elif name == "degree1":
        x = rs.normal(size=1000)
        y = 2.0 * x + 0.1 * rs.normal(size=1000)
    elif name.startswith("n"):                # n1, n2, n3, n7, n63, ...: plain series of n
        n = int(name[1:])
        x = rs.normal(size=n)
        y = 0.5 * x * x - x + 0.1 * rs.normal(size=n)
    else:
        raise KeyError(name)
    return _frozen(x, y)


ISSUE_SERIES = ("smooth", "ties", "equal", "n1", "n2", "n3", "n7", "near", "degree1")


def sliding_starts(xs, k):
    """The window loop of models/pp.py ``loess_fit``, written out."""
    n = xs.shape[0]
    starts = np.zeros(n, dtype=np.int64)
    lo = 0
    for i in range(n):
        if lo > i:
            lo = i
        while lo + k < n and (xs[lo + k] - xs[i]) < (xs[i] - xs[lo]):
            lo += 1
        lo = min(lo, n - k)
        starts[i] = lo
    return starts


HVG_SEED = 3
HVG_TOP = 60


@functools.lru_cache(maxsize=None)
def count_matrix():
    """400 cells x 300 genes of Poisson counts as float32 CSR, with genes 5 and 17 all zero
    and genes 40 and 41 constant, and a 3-level batch label."""
    rs = np.random.default_rng(HVG_SEED)
    rate = rs.gamma(0.5, 2.0, 300)
    boost = 1.0 + 4.0 * (rs.random((400, 300)) < 0.05) * (rs.random(300) < 0.4)
    X = rs.poisson(rate[None, :] * boost).astype(np.float32)
    X[:, [5, 17]] = 0
    X[:, 40] = 2
    X[:, 41] = 1
    batch = rs.integers(0, 3, 400)
    X.setflags(write=False)
    batch.setflags(write=False)
    return X, batch


def hvg_adata(sparse=True):
    from cnmf_torch_amd.utils.anndata_lite import AnnData

    X, batch = count_matrix()
    obs = pd.DataFrame({"batch": pd.Categorical([f"b{v}" for v in batch])},
                       index=[f"c{i}" for i in range(400)])
    var = pd.DataFrame(index=[f"g{j}" for j in range(300)])
    return AnnData(X=sp.csr_matrix(X) if sparse else X.copy(), obs=obs, var=var)
