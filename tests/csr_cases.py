"""Cases, float64 oracle and checks shared by test_csr_kernels_cpu.py and
test_csr_kernels_gpu.py: the CSR preprocessing ops of ops/sparse.py (csrc/kernels/sparse.hip)
at their tile, wave, trip, block-cap and rank edges.

The oracle is numpy / scipy only and never calls ops/sparse.py.  It applies the transform

    v' = min(round32?(data * row_scale) / col_div[c'], clip[c'], max_value),  c' = col_map[c]

(c' = -1 drops the entry; round32 only acts on a row-scaled value) to every stored entry in
float64, densifies with scipy and computes every op the obvious way on the dense matrix.

Matrices are built from per-row entry counts; values are small positive integers, or such
integers times a float scale, so every sum is well conditioned.  Tolerances (one comment per
assertion below) come from the number formats and the term counts, never from a run:

  u = 2^-53, gamma(t) = t u / (1 - t u).  A float64 sum of t terms in ANY order (adding an
  exact zero rounds nothing, so the empty per-wave / per-workgroup partials do not count)
  is within gamma(t) * sum|terms| of the exact sum when each term carries at most one
  rounding of its own (a product, a square) -- with an fma that rounding is the add's.  The
  oracle's own float64 sum obeys the same bound, hence |got - oracle| <= 2 gamma(t) sum|terms|.

mean_var (sklearn's two-pass scheme): with c the computed mean (any c works: the identity
sum (x-c)^2 - (sum (x-c))^2 / n = sum (x-mu)^2 is exact), n*var = q + (n-k) c^2 - corr^2/n,
q = sum over the k stored of (v-c)^2, corr = s - n c.  Roundings: v-c, the square and the
sum give q (1 + gamma(k+2)); (n-k) c^2 carries 3; the two adds, the division by n and the
ddof factor 4 more; every such term is non-negative and q + (n-k) c^2 = S := sum over all n
of (x-c)^2, so these amount to gamma(k+9) * S.  corr is the rounding residue of the mean:
|corr| <= E := 2 gamma(k) sum|v| + 2 u |s| (error of s, rounding of s/n and of n c), so
corr^2/n and its own error stay below 2 E^2 / n.  The oracle evaluates the same identity on
the dense column, where all n squares are non-zero: gamma(n+9) S + 2 E^2 / n.  Hence
|got - oracle| <= ((gamma(k+9) + gamma(n+9)) S + 4 E^2 / n) / (n - ddof), S taken at the
oracle's mean.  The mean itself: |got - oracle| <= (2 gamma(k) sum|v| + 2 u |s|) / n (the
zeros of the dense column add exactly).
"""
import functools
import math

import numpy as np
import scipy.sparse as sp
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.ops import sparse as sops

U = 2.0 ** -53
ROW_LENS = (0, 1, 63, 64, 65, 129, 255, 256, 257, 513)
K_LIST = (1, 7, 16, 17, 32, 33, 64, 65, 130)
CS_TILE = 1536          # kCsTile of csr_col_stats
TS_LDS = 4608           # kTsLds of csr_tspmm: columns per tile = TS_LDS // K
RATIOS: dict = {}       # op -> largest error / bound seen (reported by the CPU test)


def gamma(t):
    t = np.asarray(t, dtype=np.float64)
    return t * U / (1.0 - t * U)


def _note(op, err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    pos = bound > 0
    r = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    RATIOS[op] = max(RATIOS.get(op, 0.0), r)


def _frozen(X):
    for a in (X.data, X.indices, X.indptr):
        a.setflags(write=False)
    return X


# ------------------------------------------------------------------------------ matrices
def csr_from_lens(n, m, lens, seed, dtype=np.float32, scale=None, forced=None, avoid=()):
    """(n x m) CSR whose row i holds lens[i] entries at distinct random columns (never one
    of ``avoid``), the columns of forced[i] among them; values 1..9 (times ``scale``)."""
    rs = np.random.default_rng(seed)
    allowed = np.setdiff1d(np.arange(m), np.asarray(avoid, dtype=np.int64))
    indptr, idx = [0], []
    for i in range(n):
        must = np.asarray(sorted((forced or {}).get(i, ())), dtype=np.int64)
        k = max(int(lens[i]), must.size)
        rest = rs.choice(np.setdiff1d(allowed, must), k - must.size, replace=False)
        idx.append(np.sort(np.concatenate([must, rest])))
        indptr.append(indptr[-1] + k)
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    data = rs.integers(1, 10, idx.size).astype(np.float64)
    if scale is not None:
        data = data * scale
    X = sp.csr_matrix((data.astype(dtype), idx.astype(np.int32), np.asarray(indptr, np.int64)),
                      shape=(n, m))
    return _frozen(X)


def csr_three(n, m, seed, dtype=np.float32):
    """(n x m) CSR with about three entries per row (two on every 5th row, none on every
    97th), built without a Python loop: for the block-cap cases."""
    rs = np.random.default_rng(seed)
    c0 = rs.integers(0, m, n)
    a = rs.integers(1, m // 3, n)
    b = a + rs.integers(1, m // 3, n)
    cols = np.sort(np.stack([c0, (c0 + a) % m, (c0 + b) % m], axis=1), axis=1)
    cnt = np.full(n, 3)
    cnt[::5] = 2
    cnt[::97] = 0
    keep = np.arange(3)[None, :] < cnt[:, None]
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    data = rs.integers(1, 10, (n, 3)).astype(dtype)
    return _frozen(sp.csr_matrix((data[keep], cols[keep].astype(np.int32), indptr), shape=(n, m)))


def make_xf(n, m, seed, what=("row_scale", "round_mid", "col_div", "clip", "max_value"),
            col_map="subset"):
    """A transform over an (n x m) matrix.  col_map: None, 'subset' (sorted, every 4th column
    dropped), 'perm' (an unsorted permutation of a subset) or 'none_kept'."""
    rs = np.random.default_rng(seed)
    xf = {}
    if col_map is None:
        n_out = m
    elif col_map == "none_kept":
        xf["col_map"], n_out = np.full(m, -1, np.int32), 5
    else:
        cm = np.where(np.arange(m) % 4 == 1, -1, 0).astype(np.int32)
        n_out = int((cm == 0).sum())
        cm[cm == 0] = rs.permutation(n_out) if col_map == "perm" else np.arange(n_out)
        xf["col_map"] = cm
    xf["n_out"] = n_out
    if "row_scale" in what:
        xf["row_scale"] = rs.random(n) + 0.5
    if "round_mid" in what:
        xf["round_mid"] = True
    if "col_div" in what:
        xf["col_div"] = rs.random(n_out) + 0.5
    if "clip" in what:                # ceilings below and above the data (1..9, scaled)
        xf["clip"] = rs.random(n_out) * 12.0 + 0.5
    if "max_value" in what:
        xf["max_value"] = 6.5
    if "max_inf" in what:
        xf["max_value"] = float("inf")
    return xf


# -------------------------------------------------------------------------------- oracle
def entries(X, xf):
    """(row, output column or -1, transformed float64 value) of every stored entry."""
    n = X.shape[0]
    rows = np.repeat(np.arange(n), np.diff(X.indptr))
    c = X.indices.astype(np.int64)
    if xf.get("col_map") is not None:
        c = np.asarray(xf["col_map"], np.int64)[c]
    at = np.maximum(c, 0)
    v = X.data.astype(np.float64)
    if xf.get("row_scale") is not None:
        v = v * np.asarray(xf["row_scale"], np.float64)[rows]
        if xf.get("round_mid"):
            v = v.astype(np.float32).astype(np.float64)
    if xf.get("col_div") is not None:
        v = v / np.asarray(xf["col_div"], np.float64)[at]
    if xf.get("clip") is not None:
        v = np.minimum(v, np.asarray(xf["clip"], np.float64)[at])
    if xf.get("max_value") is not None:
        v = np.minimum(v, float(xf["max_value"]))
    return rows, c, v


def dense(X, xf):
    """(D, C): the transformed matrix and the stored-entry indicator, float64 (n x n_out)."""
    rows, c, v = entries(X, xf)
    shape = (X.shape[0], int(xf.get("n_out", X.shape[1])))
    keep = c >= 0
    ij = (rows[keep], c[keep])
    D = sp.csr_matrix((v[keep], ij), shape=shape).toarray()
    C = sp.csr_matrix((np.ones(int(keep.sum())), ij), shape=shape).toarray()
    return D, C


class Case:
    """A matrix and a transform, with the oracle's dense images computed once."""

    def __init__(self, name, X, xf=None):
        self.name, self.X, self.xf = name, X, dict(xf or {})
        self.xf.setdefault("n_out", X.shape[1])
        self.n, self.n_out = X.shape[0], int(self.xf["n_out"])

    @functools.cached_property
    def DC(self):
        D, C = dense(self.X, self.xf)
        D.setflags(write=False)
        C.setflags(write=False)
        return D, C

    def csr(self, dev):
        return sops.DeviceCSR.from_scipy(self.X.copy(), device=dev)   # a writable copy

    def kw(self, drop=()):
        return {k: v for k, v in self.xf.items() if k not in drop}


def _lens_for(n):
    if n == 1:
        return [65]
    if n == 3:
        return [0, 257, 64]
    if n == 4:
        return [1, 513, 0, 63]
    if n == 5:
        return [0, 256, 129, 255, 0]
    lens = [ROW_LENS[i % len(ROW_LENS)] for i in range(n)]     # n = 130: every length 13 times
    lens[0] = lens[-1] = 0                                      # empty first and last rows
    return lens


@functools.lru_cache(maxsize=None)
def rows_case(n, dtype="float32", col_map="perm"):
    """rows-n{1,3,4,5,130}: the ROW_LENS row lengths on 600 stored columns, column 7 empty,
    seen through every transform factor and a dropping, unsorted col_map."""
    X = csr_from_lens(n, 600, _lens_for(n), seed=100 + n, dtype=np.dtype(dtype), scale=0.37,
                      avoid=(7,))
    return Case(f"rows-n{n}", X, make_xf(n, 600, seed=n, col_map=col_map))


def _edge_cols(n_out, edges):
    return sorted({c for e in edges for c in (e - 1, e) if 0 <= c < n_out})


@functools.lru_cache(maxsize=None)
def colstats_nout_case(n_out, mapped):
    """colstats-nout{1,1535,1536,1537,3073}[-map]: 70 rows; rows 3 and 4 hold both columns on
    each side of every 1536-column tile edge (1535|1536, 3071|3072) that n_out reaches; with
    ``mapped`` the n_out columns are an unsorted subset of a 1.25x wider stored matrix."""
    edge = _edge_cols(n_out, (CS_TILE, 2 * CS_TILE))
    lens = [min(ROW_LENS[i % len(ROW_LENS)], n_out) for i in range(70)]
    if not mapped:
        X = csr_from_lens(70, n_out, lens, seed=n_out, forced={3: edge, 4: edge})
        return Case(f"colstats-nout{n_out}", X)
    m = n_out + n_out // 4 + 3
    rs = np.random.default_rng(n_out + 1)
    kept = rs.permutation(m)[:n_out]              # stored column of output column j
    cm = np.full(m, -1, np.int32)
    cm[kept] = np.arange(n_out)
    forced = [int(kept[c]) for c in edge]
    X = csr_from_lens(70, m, [min(x, m) for x in lens], seed=n_out, scale=0.37,
                      forced={3: forced, 4: forced})
    xf = dict(col_map=cm, n_out=n_out, col_div=rs.random(n_out) + 0.5,
              row_scale=rs.random(70) + 0.5)
    return Case(f"colstats-nout{n_out}-map", X, xf)


@functools.lru_cache(maxsize=None)
def colstats_n_case(n):
    """colstats-n{63,64,65,33000}: the rows-per-block edge (64 rows per workgroup) and the
    512-workgroup cap (33000 rows -> 65 rows per block, blocks 508..511 own no rows)."""
    if n >= 1000:
        return Case(f"colstats-n{n}", csr_three(n, 41, seed=n))
    return Case(f"colstats-n{n}", csr_from_lens(n, 41, [3 + (i % 5) for i in range(n)], seed=n))


@functools.lru_cache(maxsize=None)
def special_case():
    """130 rows x 12 columns: column 2 is constant (every row stores 3), column 5 has a mean
    1.2e6 times its standard deviation (1000000 + {0,1,2}, every row), column 9 is empty."""
    rs = np.random.default_rng(77)
    D = rs.integers(0, 4, (130, 12)).astype(np.float32)
    D[:, 2] = 3.0
    D[:, 5] = 1000000.0 + rs.integers(0, 3, 130)
    D[:, 9] = 0.0
    return Case("colstats-special", _frozen(sp.csr_matrix(D)))


def tspmm_tc(K):
    return TS_LDS // K


@functools.lru_cache(maxsize=None)
def tspmm_tile_case(K, which):
    """tspmm-K{7,17,64}-tc{-1,,+1,x2+1}: n_out around the tile width tc = 4608 // K, rows 1
    and 2 with entries on both sides of every tile edge n_out reaches."""
    tc = tspmm_tc(K)
    n_out = {"tc-1": tc - 1, "tc": tc, "tc+1": tc + 1, "2tc+1": 2 * tc + 1}[which]
    edge = _edge_cols(n_out, (tc, 2 * tc))
    lens = [min(ROW_LENS[i % len(ROW_LENS)], n_out) for i in range(40)]
    X = csr_from_lens(40, n_out, lens, seed=K * 10 + len(which), scale=0.37,
                      forced={1: edge, 2: edge})
    return Case(f"tspmm-K{K}-{which}", X)


@functools.lru_cache(maxsize=None)
def tspmm_cap_case():
    """tspmm-n66000: the 256-workgroup cap (258 rows per block)."""
    return Case("tspmm-n66000", csr_three(66000, 53, seed=66))


@functools.lru_cache(maxsize=None)
def factor_case(factor, col_map, in_dtype):
    """One transform factor alone (or 'all' / 'none') over a 9 x 40 matrix with rows of
    0..40 entries; float64 data is not float32-representable (scale 0.37)."""
    what = {"row_scale": ("row_scale",), "row_scale+round": ("row_scale", "round_mid"),
            "round_only": ("round_mid",), "col_div": ("col_div",), "clip": ("clip",),
            "max_finite": ("max_value",), "max_inf": ("max_inf",), "none": (),
            "all": ("row_scale", "round_mid", "col_div", "clip", "max_value")}[factor]
    X = csr_from_lens(9, 40, [0, 1, 5, 40, 17, 0, 33, 2, 0], seed=9, dtype=np.dtype(in_dtype),
                      scale=0.37)
    cm = {"nomap": None, "subset": "subset", "perm": "perm", "alldropped": "none_kept"}[col_map]
    return Case(f"xform-{factor}-{col_map}", X, make_xf(9, 40, seed=len(factor), what=what,
                                                        col_map=cm))


def empty_case(which):
    """empty-norows: a (0 x 30) CSR; empty-nonnz: a (6 x 30) CSR with no stored entries."""
    n = 0 if which == "norows" else 6
    return Case(f"empty-{which}", _frozen(sp.csr_matrix((n, 30), dtype=np.float32)))


# -------------------------------------------------------------------------------- checks
def _native(dev, t):
    if torch.device(dev).type == "cuda":
        assert ops.use_native(t), "a GPU input must take the HIP kernel"


def _np(t):
    return t.detach().cpu().numpy()


def check_row_sums(case, dev):
    A = case.csr(dev)
    _native(dev, A.data)
    got = _np(sops.row_sums(A))
    Xd = case.X.toarray().astype(np.float64)
    ref, absum = Xd.sum(1), np.abs(Xd).sum(1)
    t = np.diff(case.X.indptr)
    assert got.shape == ref.shape and got.dtype == np.float64
    # float64 sum of t stored values in a fixed order: 2 gamma(t) sum|v| (module docstring)
    bound = 2 * gamma(t) * absum
    _note("row_sums", np.abs(got - ref), bound)
    assert (np.abs(got - ref) <= bound).all()


def check_col_stats(case, dev, center=None):
    A = case.csr(dev)
    _native(dev, A.data)
    kw = case.kw()
    s, q, k = (_np(x) for x in sops.col_stats(A, center=center, **kw))
    D, C = case.DC
    cen = np.zeros(case.n_out) if center is None else np.asarray(center, np.float64)
    sq = ((D - cen) ** 2) * C
    # counts are sums of ones: exact
    np.testing.assert_array_equal(k, C.sum(0))
    t = C.sum(0)
    # float64 fixed-order sums of t terms: 2 gamma(t) sum|terms| per column
    bs, bq = 2 * gamma(t) * np.abs(D).sum(0), 2 * gamma(t) * sq.sum(0)
    _note("col_stats.sum", np.abs(s - D.sum(0)), bs)
    _note("col_stats.sq", np.abs(q - sq.sum(0)), bq)
    assert (np.abs(s - D.sum(0)) <= bs).all()
    assert (np.abs(q - sq.sum(0)) <= bq).all()
    # determinism: no atomics, fixed reduction order -> bitwise equal across launches
    s2, q2, k2 = sops.col_stats(A, center=center, **kw)
    assert np.array_equal(_np(s2), s) and np.array_equal(_np(q2), q) and np.array_equal(_np(k2), k)


def oracle_mean_var(D, ddof):
    n = D.shape[0]
    mean = D.sum(0) / n
    dev = D - mean
    var = ((dev ** 2).sum(0) - dev.sum(0) ** 2 / n) / n
    var = np.maximum(var, 0.0)
    return mean, (var * (n / (n - ddof)) if ddof and n > 1 else var)


def check_mean_var(case, dev, ddof=0):
    A = case.csr(dev)
    _native(dev, A.data)
    mean, var = (_np(x) for x in sops.mean_var(A, ddof=ddof, **case.kw()))
    D, C = case.DC
    n, k = case.n, C.sum(0)
    m_ref, v_ref = oracle_mean_var(D, ddof)
    absum = np.abs(D).sum(0)
    # mean = s / n: the sum's 2 gamma(k) sum|v| plus the division's rounding on both sides
    E = 2 * gamma(k) * absum + 2 * U * np.abs(D.sum(0))
    _note("mean_var.mean", np.abs(mean - m_ref), E / n)
    assert (np.abs(mean - m_ref) <= E / n).all()
    # the two-pass formula, propagated (module docstring)
    S = ((D - m_ref) ** 2).sum(0)
    d = n - ddof if (ddof and n > 1) else n
    bv = ((gamma(k + 9) + gamma(n + 9)) * S + 4 * E * E / n) / d
    _note("mean_var.var", np.abs(var - v_ref), bv)
    assert (var >= 0).all()
    assert (np.abs(var - v_ref) <= bv).all()


def _out_np(dt):
    return np.float64 if dt == torch.float64 else np.float32


def check_transform(case, dev, out_dtype):
    A = case.csr(dev)
    _native(dev, A.data)
    got = _np(sops.transform(A, out_dtype=out_dtype, **case.kw(drop=("n_out",))))
    _, c, v = entries(case.X, case.xf)
    ref = np.where(c >= 0, v, -1.0).astype(_out_np(out_dtype))
    # same operation order, IEEE float64 ops, one final rounding to the output type: bitwise
    assert got.dtype == ref.dtype
    np.testing.assert_array_equal(got.view(np.uint8), ref.view(np.uint8))
    if (c < 0).all():
        assert (got == -1).all()


def check_densify(case, dev, out_dtype):
    A = case.csr(dev)
    _native(dev, A.data)
    got = _np(sops.densify(A, out_dtype=out_dtype, **case.kw()))
    ref = case.DC[0].astype(_out_np(out_dtype))
    # bitwise, as for transform; untouched cells are +0
    assert got.dtype == ref.dtype and got.shape == ref.shape
    np.testing.assert_array_equal(got.view(np.uint8), ref.view(np.uint8))


def dense_B(rows, K, seed, dtype=np.float32):
    """A (rows x K) dense operand with signs, asymmetric in both axes."""
    rs = np.random.default_rng(seed)
    return (rs.random((rows, K)) - 0.3).astype(dtype)


def check_spmm(case, dev, K):
    A = case.csr(dev)
    _native(dev, A.data)
    V = A.view(**case.kw())
    B = dense_B(case.n_out, K, seed=K)
    got = _np(sops.spmm(V, torch.from_numpy(B).to(dev)))
    D, C = case.DC
    B64 = B.astype(np.float64)
    ref, absum = D @ B64, np.abs(D) @ np.abs(B64)
    nnz_row = C.sum(1)[:, None]
    assert got.shape == ref.shape and got.dtype == np.float32
    # float32 fma chain per lane then a 64-lane tree: (nnz_row + 8) 2^-24 sum|v b|, plus the
    # float32 rounding of v itself: one more 2^-24 sum|v b|
    bound = (nnz_row + 8 + 1) * 2.0 ** -24 * absum
    _note("spmm", np.abs(got - ref), bound)
    assert (np.abs(got - ref) <= bound).all()


def check_tspmm(case, dev, K, b_dtype=np.float64):
    A = case.csr(dev)
    _native(dev, A.data)
    V = A.view(**case.kw())
    B = dense_B(case.n, K, seed=K + 1, dtype=b_dtype)
    Bt = torch.from_numpy(B).to(dev)
    out = sops.tspmm(V, Bt)
    got = _np(out)
    D, C = case.DC
    B64 = B.astype(np.float64)
    ref, absum = D.T @ B64, np.abs(D).T @ np.abs(B64)
    t = C.sum(0)[:, None]
    assert got.shape == ref.shape and got.dtype == np.float64
    # float64 fma per stored entry, partials combined in a fixed order: 2 gamma(t) sum|v b|
    bound = 2 * gamma(t) * absum
    _note("tspmm", np.abs(got - ref), bound)
    assert (np.abs(got - ref) <= bound).all()
    # determinism: bitwise equal across two launches
    assert torch.equal(out, sops.tspmm(V, Bt))


def check_all_ops(case, dev):
    check_row_sums(case, dev)
    check_col_stats(case, dev)
    check_mean_var(case, dev, ddof=1)
    for od in (torch.float32, torch.float64):
        check_transform(case, dev, od)
        check_densify(case, dev, od)
    check_spmm(case, dev, 7)
    check_tspmm(case, dev, 7)


def check_empty(case, dev):
    """row_sums, col_stats, tspmm and spmm of a matrix without rows or without entries:
    exact zeros of the right shape."""
    A = case.csr(dev)
    if torch.device(dev).type == "cuda":
        # leave freed, non-zero device memory of the partials' sizes behind, so that
        # uninitialised partials cannot read as zeros by luck
        for shape in ((3, 1, case.n_out), (1, case.n_out, 5)):
            torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    rsum = sops.row_sums(A)
    assert tuple(rsum.shape) == (case.n,) and not rsum.any()
    for x in sops.col_stats(A):
        assert tuple(x.shape) == (case.n_out,) and x.dtype == torch.float64
        assert (_np(x) == 0).all(), _np(x)
    out = sops.tspmm(A, torch.ones((case.n, 5), dtype=torch.float64, device=dev))
    assert tuple(out.shape) == (case.n_out, 5) and out.dtype == torch.float64
    assert (_np(out) == 0).all(), _np(out)
    out = sops.spmm(A, torch.ones((case.n_out, 5), device=dev))
    assert tuple(out.shape) == (case.n, 5) and (_np(out) == 0).all()


# ------------------------------------------------------------------ radix select / quantile
RADIX_M = 1048576 + 257      # one past 4096 blocks x 256: the grid-stride second trip


@functools.lru_cache(maxsize=None)
def radix_vector(name):
    """(float32 vector, ranks to query) -- negative entries are dropped entries."""
    rs = np.random.default_rng(sum(map(ord, name)))
    if name == f"m{RADIX_M}":
        x = (rs.random(RADIX_M) * 100).astype(np.float32)
        x[::11] = -1.0
        nn = int((x >= 0).sum())
        ranks = (0, 1, nn // 2, nn - 257, nn - 2, nn - 1)
    elif name == "ties40":                 # 40 % of 1000 entries equal 3.25
        x = np.concatenate([rs.random(300) * 3, np.full(400, 3.25), 4 + rs.random(300)])
        x = x[rs.permutation(1000)].astype(np.float32)
        ranks = (299, 300, 301, 500, 698, 699, 700)   # before / inside / after the run
    elif name == "lowbytes":               # 1 + j 2^-23, j < 300: bytes 0 and 1 differ only
        x = (np.float32(1) + np.arange(300, dtype=np.float32) * np.float32(2.0 ** -23))
        x = x[rs.permutation(300)]
        ranks = (0, 1, 127, 128, 255, 256, 257, 299)
    elif name == "denormals":
        x = np.arange(0, 40, dtype=np.uint32).view(np.float32).copy()    # 0 and 39 denormals
        x = np.concatenate([x, np.float32([1e-38, 2.0 ** -126, 1.0, -1.0])])[rs.permutation(44)]
        ranks = (0, 1, 2, 39, 40, 41, 42)
    elif name == "inf":
        x = np.float32([3, np.inf, 0.5, -1, np.inf, 7, 2])[rs.permutation(7)]
        ranks = (0, 3, 4, 5)
    elif name == "negzero":                # a stored -0.0 is a zero, not the largest value
        x = np.float32([2, -0.0, 1, -1, 0.0, 3, -0.0, 5e-45])[rs.permutation(8)]
        ranks = (0, 1, 2, 3, 4, 6)
    elif name == "allnegative":
        x, ranks = np.full(500, -1.0, np.float32), ()
    else:
        raise KeyError(name)
    x.setflags(write=False)
    return x, ranks


RADIX_NAMES = (f"m{RADIX_M}", "ties40", "lowbytes", "denormals", "inf", "negzero", "allnegative")


def oracle_kth(x, k):
    v = x[x >= 0] + np.float32(0.0)        # -0.0 + 0.0 = +0.0: a zero of either sign is 0
    return float(np.partition(v, k)[k])


def check_kth(name, dev):
    x, ranks = radix_vector(name)
    t = torch.from_numpy(x.copy()).to(dev)
    _native(dev, t)
    if not ranks:                          # nothing stored: every rank is out of range
        for k in (0, 5):
            try:
                sops.kth_nonneg(t, k)
            except IndexError:
                continue
            raise AssertionError("kth_nonneg of an all-dropped input must raise IndexError")
        return
    for k in ranks:
        got, ref = sops.kth_nonneg(t, k), oracle_kth(x, k)
        # a selection, no arithmetic: exact (a zero compares equal whatever its sign)
        assert got == ref, (name, k, got, ref)
    nn = int((x >= 0).sum())
    try:
        sops.kth_nonneg(t, nn)
    except IndexError:
        return
    raise AssertionError("kth_nonneg past the last rank must raise IndexError")


def quantile_queries(x):
    """(n_total, q) pairs: q in {0, 0.5, 0.9999, 1} without and with implicit zeros, and a
    q whose ``lo`` is the last implicit zero and ``hi`` the smallest stored value."""
    ns = int((x >= 0).sum())
    out = [(ns, q) for q in (0.0, 0.5, 0.9999, 1.0)]
    nt = ns + ns // 3 + 2
    out += [(nt, q) for q in (0.0, 0.5, 0.9999, 1.0)]
    nz = nt - ns
    q = (nz - 0.5) / (nt - 1)
    pos = q * (nt - 1)
    assert math.floor(pos) == nz - 1 and math.ceil(pos) == nz
    return out + [(nt, q)]


def check_quantile(name, dev):
    x, _ = radix_vector(name)
    t = torch.from_numpy(x.copy())
    td = t.to(dev)
    _native(dev, td)
    stored = (x[x >= 0] + np.float32(0.0)).astype(np.float64)
    fulls = {}
    for n_total, q in quantile_queries(x):
        got = sops.quantile_with_zeros(td, n_total, q)
        cpu = sops.quantile_with_zeros(t, n_total, q)
        # both paths select the same two order statistics exactly and share the float64
        # interpolation: equal (NaN where the arithmetic meets inf - inf)
        assert got == cpu or (math.isnan(got) and math.isnan(cpu)), (name, n_total, q, got, cpu)
        if n_total not in fulls:
            fulls[n_total] = np.sort(np.concatenate([np.zeros(n_total - stored.size), stored]))
        full = srt = fulls[n_total]
        with np.errstate(invalid="ignore"):
            ref = float(np.quantile(full, q))
        if not math.isfinite(ref):         # numpy's lerp has no finite answer beside +inf
            continue
        pos = q * (n_total - 1)
        M = max(abs(srt[math.floor(pos)]), abs(srt[math.ceil(pos)]))
        # a + (b-a) t: roundings of b-a, of the product and of the sum, each at most u M
        # (0 <= a <= b, 0 <= t <= 1) -> 3 u M; numpy's b - (b-a)(1-t) form for t >= 0.5 the
        # same (1-t is exact there) -> 6 u M < 6 ulp(M) of float64
        assert abs(got - ref) <= 6 * np.spacing(M), (name, n_total, q, got, ref)
