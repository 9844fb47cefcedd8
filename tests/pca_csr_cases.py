"""Cases, float64 oracle and checks shared by test_pca_csr_cpu.py and test_pca_csr_gpu.py:
ops.sparse.gram / project (csrc/kernels/pca_csr.hip) and models.pp.pca_csr.

The oracle is numpy only (csr_cases.dense: the transformed matrix densified in float64, then
rounded to the value dtype) and never calls ops/sparse.py.  Bounds, from the number formats
and the term counts (csr_cases' docstring: a float64 sum of t terms in any order, each term
with at most one rounding of its own, is within gamma(t) sum|terms| of the exact sum):

  G[i][j] sums one product per row that stores both columns, t of them, split over the
  kernel's row slabs: |got - oracle| <= 2 gamma(t + slabs + 1) sum|a b|.
  A score sums one product per kept entry of the row and subtracts the shift:
  |got - oracle| <= 2 gamma(len + 2) (sum|v V| + |shift|).
"""
import functools

import numpy as np
import scipy.sparse as sp
import torch

import csr_cases as cc
from cnmf_torch_amd.models import pp
from cnmf_torch_amd.ops import sparse as sops

TILE = 64          # kGrTile: output columns per tile
MIN_ROWS = 256     # kGrMinRows: rows per slab while n is small (R of the n cases)
NH_LIST = (1, 63, 64, 65, 130, 200)
# the wave count, the 64-row chunk of a wave and the slab edge
N_LIST = (1, 3, 4, 5, 63, 64, 65, MIN_ROWS - 1, MIN_ROWS, MIN_ROWS + 1, 2 * MIN_ROWS + 3)
C_LIST = (1, 50, 64, 65, 130)
FACTORS = ("none", "row_scale", "row_scale+round", "col_div", "clip", "max_finite", "all")
VDT = {"float32": torch.float32, "float64": torch.float64}


def _np(t):
    return t.detach().cpu().numpy()


def rounded(D, vd):
    return D.astype(np.float32).astype(np.float64) if vd == "float32" else D


def slabs(dev, n, nh):
    """Row slabs of the device kernel; the CPU path adds one 4096-row block at a time."""
    if torch.device(dev).type == "cuda":
        return int(sops._hip.csr_gram_slabs(n, nh))
    return max(1, -(-n // 4096))


# ---------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def nh_case(nh):
    """gram-nh{1,63,64,65,130,200}: 70 rows of the ROW_LENS lengths (capped at nh), small
    integers, no transform: one tile, both tile edges, three tiles with a ragged last one."""
    lens = [min(cc.ROW_LENS[i % len(cc.ROW_LENS)], nh) for i in range(70)]
    return cc.Case(f"gram-nh{nh}", cc.csr_from_lens(70, nh, lens, seed=nh))


@functools.lru_cache(maxsize=None)
def n_case(n):
    """gram-n{1,3,4,5,63,64,65,255,256,257,515}: 130 columns, rows around the wave count, a
    wave's 64-row chunk and the slab edge (257 rows: two slabs; 515: three, the last one
    short), empty first and last rows."""
    lens = [min(x, 130) for x in cc._lens_for(n)]
    return cc.Case(f"gram-n{n}", cc.csr_from_lens(n, 130, lens, seed=300 + n))


@functools.lru_cache(maxsize=None)
def wide_case():
    """gram-wide: 600 x 2000, 32 tiles (528 tile pairs) and one slab, so every wave takes a
    second and a third chunk; rows of up to 513 entries."""
    lens = cc._lens_for(600)
    return cc.Case("gram-wide", cc.csr_from_lens(600, 2000, lens, seed=600))


@functools.lru_cache(maxsize=None)
def pairs_case():
    """gram-pairs: 140 stored columns, 130 kept (tiles 0..63 | 64..127 | 128, 129).  Rows with
    8 + 8, 5 + 13 and 64 + 64 entries in tiles 0 and 1 (64, 65 and 4096 pairs: one, two and
    64 lane steps), a row stored only in dropped columns, empty rows, a row in the ragged
    tile only."""
    t0, t1 = np.arange(0, 64), np.arange(64, 128)
    forced = {1: list(t0[3:11]) + list(t1[20:28]),
              2: list(t0[::13][:5]) + list(t1[1::5][:13]),
              4: list(t0) + list(t1),
              5: [131, 135, 139],
              7: [128, 129],
              8: list(t0[:2]) + [128]}
    lens = [len(forced.get(i, ())) for i in range(10)]
    X = cc.csr_from_lens(10, 140, lens, seed=5, forced=forced)
    cm = np.where(np.arange(140) < 130, np.arange(140), -1).astype(np.int32)
    return cc.Case("gram-pairs", X, dict(col_map=cm, n_out=130))


@functools.lru_cache(maxsize=None)
def full_case():
    """gram-full: a fully dense 70 x 130 matrix of small integers."""
    return cc.Case("gram-full", cc.csr_from_lens(70, 130, [130] * 70, seed=70))


def exact_cases():
    return ([nh_case(nh) for nh in NH_LIST] + [n_case(n) for n in N_LIST]
            + [pairs_case(), full_case(), wide_case()])


# -------------------------------------------------------------------------------- checks
def check_gram(case, dev, vd="float64", exact=False):
    A = case.csr(dev)
    cc._native(dev, A.data)
    V = A.view(**case.kw())
    out = sops.gram(V, value_dtype=VDT[vd])
    G = _np(out)
    D, C = case.DC
    D = rounded(D, vd)
    ref, absum = D.T @ D, np.abs(D).T @ np.abs(D)
    t = C.T @ C + slabs(dev, case.n, case.n_out) + 1
    assert G.shape == ref.shape and G.dtype == np.float64
    # float64 products of one rounding each, summed in a fixed order over rows, replicas and
    # slabs: 2 gamma(t) sum|a b| (module docstring)
    bound = 2 * cc.gamma(t) * absum
    cc._note("gram", np.abs(G - ref), bound)
    assert (np.abs(G - ref) <= bound).all(), case.name
    if exact:
        # small integers: every product and partial sum is exact in float64, so a lost or
        # doubled update shows
        np.testing.assert_array_equal(G, ref, err_msg=case.name)
    # the diagonal tile pair computes the full square and (I, J) is mirrored: bitwise
    assert np.array_equal(G, G.T), case.name
    # no atomics, fixed reduction order: bitwise equal across launches
    assert torch.equal(out, sops.gram(V, value_dtype=VDT[vd])), case.name


def check_project(case, dev, c, vd="float64", shift=False):
    A = case.csr(dev)
    cc._native(dev, A.data)
    V = A.view(**case.kw())
    B = cc.dense_B(case.n_out, c, seed=c, dtype=np.float64)
    sh = cc.dense_B(1, c, seed=c + 7, dtype=np.float64)[0] if shift else None
    Bt = torch.from_numpy(B).to(dev)
    st = torch.from_numpy(sh).to(dev) if shift else None
    out = sops.project(V, Bt, st, value_dtype=VDT[vd])
    got = _np(out)
    D, C = case.DC
    D = rounded(D, vd)
    ref, absum = D @ B, np.abs(D) @ np.abs(B)
    if shift:
        ref, absum = ref - sh, absum + np.abs(sh)
    t = C.sum(1)[:, None] + 2
    assert got.shape == ref.shape and got.dtype == np.float64
    # one fma per kept entry in stored order, then the shift: 2 gamma(len + 2) sum|terms|
    bound = 2 * cc.gamma(t) * absum
    cc._note("project", np.abs(got - ref), bound)
    assert (np.abs(got - ref) <= bound).all(), (case.name, c)
    assert torch.equal(out, sops.project(V, Bt, st, value_dtype=VDT[vd])), (case.name, c)


# ------------------------------------------------------------------------------------ PCA
PCA_CASES = ((257, 130, 5, 1, 0.08), (1000, 200, 6, 2, 0.08))


@functools.lru_cache(maxsize=None)
def pca_counts(n, g, k, seed, depth):
    rs = np.random.default_rng(seed)
    W = rs.gamma(0.3, 1.0, (k, g)) * (1 + np.arange(k))[:, None]
    U = rs.dirichlet(np.full(k, 0.3), n)
    lam = U @ W
    lam *= depth * g / lam.sum(1, keepdims=True)
    X = sp.csr_matrix(rs.poisson(lam).astype(np.float32))
    return cc._frozen(X)


@functools.lru_cache(maxsize=None)
def pca_case(i, vd):
    """Generator case i as the TP10K-scaled, std-scaled view, zero-variance columns dropped
    through col_map; with float32 values the row-scaled value is rounded too, as the
    pipeline does."""
    X = pca_counts(*PCA_CASES[i])
    n, g = X.shape
    rs = 1e4 / np.maximum(np.asarray(X.sum(1)).reshape(-1).astype(np.float64), 1.0)
    xf = dict(row_scale=rs, round_mid=vd == "float32")
    Dn, _ = cc.dense(X, xf)
    std = Dn.std(0, ddof=1)
    kept = np.flatnonzero(std > 0)
    cm = np.full(g, -1, np.int32)
    cm[kept] = np.arange(kept.size)
    xf.update(col_map=cm, n_out=int(kept.size), col_div=std[kept])
    return cc.Case(f"pca-{i}-{vd}", X, xf)


@functools.lru_cache(maxsize=None)
def pca_oracle(i, vd):
    """pca_tensor of the dense float64 image of the view (rounded to the value dtype) on the
    CPU, and the first ten relative eigenvalue gaps of its covariance."""
    D = rounded(pca_case(i, vd).DC[0], vd)
    res = pp.pca_tensor(torch.from_numpy(D.copy()), 10, zero_center=True)
    Dc = D - D.mean(0)
    lam = np.sort(np.linalg.eigvalsh(Dc.T @ Dc))[::-1]
    gaps = (lam[:10] - lam[1:11]) / lam[0]
    for a in res:
        a.setflags(write=False)
    return res, gaps


def _aligned(got, ref, axis):
    s = np.sign((got * ref).sum(axis=axis, keepdims=True))
    s[s == 0] = 1
    return got * s


def assert_pca_close(got, ref):
    """Scores and components within 1e-8 of the oracle's largest |entry| after per-component
    sign alignment, variances at rtol 1e-10 (eigenvector error |dC| / gap with |dC| / lambda_1
    about n u (1 + mu^2 / sigma^2) ~ 1e-12 and gaps >= 1e-4)."""
    (xs, vh, var, ratio), (xs0, vh0, var0, ratio0) = got, ref
    assert xs.shape == xs0.shape and vh.shape == vh0.shape
    e_s = np.abs(_aligned(xs, xs0, 0) - xs0).max() / np.abs(xs0).max()
    e_v = np.abs(_aligned(vh, vh0, 1) - vh0).max() / np.abs(vh0).max()
    print(f"pca_csr: score error {e_s:.3g}, component error {e_v:.3g} of the largest entry")
    assert e_s <= 1e-8 and e_v <= 1e-8, (e_s, e_v)
    np.testing.assert_allclose(var, var0, rtol=1e-10, atol=0)
    np.testing.assert_allclose(ratio, ratio0, rtol=1e-10, atol=0)


def check_pca_csr(i, vd, dev):
    ref, gaps = pca_oracle(i, vd)
    assert (gaps >= 1e-4).all(), gaps          # the tolerances below assume separated components
    case = pca_case(i, vd)
    A = case.csr(dev)
    cc._native(dev, A.data)
    got = pp.pca_csr(A.view(**case.kw()), n_comps=10, zero_center=True, value_dtype=VDT[vd])
    assert_pca_close(got, ref)
    # the sign rule: the largest |score| of every component is positive
    xs = got[0]
    assert (xs[np.abs(xs).argmax(0), np.arange(xs.shape[1])] > 0).all()
