"""scanpy-equivalent preprocessing primitives used by cNMF and Preprocess.

The reference calls scanpy for these (SURVEY.md §2.3 "scanpy functions"); scanpy is
not a dependency here, so each is re-implemented with the same numerics:

* ``normalize_total`` -- per-cell scaling to ``target_sum`` (int input -> float32,
  zero-count cells left at zero), preprocess.py:224, cnmf.py:246.
* ``scale`` with ``zero_center=False`` -- divide genes by their ddof=1 std (zero std
  -> 1), optional ``max_value`` clip, cnmf.py:675, preprocess.py:22.
* ``filter_genes`` / ``filter_cells`` -- min_cells / min_counts, preprocess.py:92,105.
* ``highly_variable_genes(flavor='seurat_v3')`` -- variance-stabilised ranking with a
  local quadratic (loess, span 0.3) fit of log10 variance on log10 mean; skmisc's
  loess is not installed, so a direct tricube-weighted local regression is used
  (``surface='direct'`` equivalent; parity with skmisc's interpolated surface is
  within loess smoothing noise -- "parity unpinned").  ``loess="native"`` computes the
  same fit in O(genes) memory through ``ops.loess`` (loess.hip on the GPU).
* ``pca`` -- zero-centred truncated PCA from the (genes x genes) covariance, preprocess.py:310;
  ``backend="csr"`` / ``pca_csr`` compute it from a device CSR without a dense copy.
"""
from __future__ import annotations

import numpy as np
import pandas as pd
import scipy.sparse as sp
import torch

from ..utils.anndata_lite import AnnData, to_lite


def _row_sums(X) -> np.ndarray:
    return np.asarray(X.sum(axis=1)).reshape(-1)


def normalize_total(adata, target_sum: float | None = None, copy: bool = False, inplace=True):
    adata = to_lite(adata)
    ad = adata.copy() if copy else adata
    X = ad.X
    if np.issubdtype(X.dtype, np.integer):
        X = X.astype(np.float32)
    counts = _row_sums(X).astype(np.float64)
    after = np.median(counts[counts > 0]) if target_sum is None else float(target_sum)
    counts = counts + (counts == 0)
    scale = (after / counts)
    if sp.issparse(X):
        X = sp.csr_matrix(X) if not sp.isspmatrix_csr(X) else X
        X = X.copy() if X is ad.X and not copy else X
        from ..utils.io import _npzio
        if _npzio is not None and X.dtype in (np.float32, np.float64) and X.data.flags.c_contiguous:
            # native threaded row scaling, the same float ops as the numpy line below
            _npzio.csr_scale_rows(X.data, X.indptr, np.ascontiguousarray(scale, dtype=np.float64))
        else:
            X.data = (X.data * np.repeat(scale, np.diff(X.indptr)).astype(X.dtype)).astype(X.dtype)
    else:
        X = np.array(X, copy=True) if X is ad.X and not copy else X
        X = (X / (counts / after)[:, None].astype(X.dtype)).astype(X.dtype)
    ad.X = X
    return ad


def _mean_var_ddof1(X):
    n = X.shape[0]
    from .hvg import exact_mean_var

    ex = exact_mean_var(X, 1)          # exact moments, one rounding (models.hvg)
    if ex is not None:
        return ex
    if sp.issparse(X):
        # scanpy's sparse path: sklearn's centred two-pass variance (exact 0 for constant
        # genes; models.hvg.sparse_mean_var, the same float64 operations in the same
        # order); the dense path below is scanpy's E[x^2] - E[x]^2
        from .hvg import sparse_mean_var

        mean, var = sparse_mean_var(sp.csr_matrix(X, dtype=np.float64))
    else:
        mean = np.mean(X, axis=0, dtype=np.float64)
        mean_sq = np.mean(np.multiply(X, X, dtype=np.float64), axis=0)
        var = mean_sq - mean ** 2
    if n > 1:
        var *= n / (n - 1)
    return mean, var


def scale(adata, zero_center: bool = False, max_value: float | None = None, copy: bool = False):
    if zero_center:
        raise NotImplementedError("only zero_center=False is used by cNMF")
    adata = to_lite(adata)
    ad = adata.copy() if copy else adata
    X = ad.X
    if np.issubdtype(X.dtype, np.integer):
        X = X.astype(np.float64)
    _, var = _mean_var_ddof1(X)
    std = np.sqrt(var)
    std[std == 0] = 1.0
    if sp.issparse(X):
        X = sp.csr_matrix(X, copy=True)
        X.data = (X.data / std[X.indices]).astype(X.data.dtype)
        if max_value is not None:
            X.data[X.data > max_value] = max_value
    else:
        X = (X / std.astype(X.dtype) if X.dtype == np.float32 else X / std)
        if max_value is not None:
            X = np.minimum(X, max_value)
    ad.X = X
    return ad


def filter_genes(adata, min_cells: int | None = None, min_counts: float | None = None):
    adata = to_lite(adata)
    X = adata.X
    if min_cells is not None:
        n_cells = np.asarray((X > 0).sum(axis=0)).reshape(-1)
        keep = n_cells >= min_cells
        adata.var["n_cells"] = n_cells
    else:
        tot = np.asarray(X.sum(axis=0)).reshape(-1)
        keep = tot >= min_counts
        adata.var["n_counts"] = tot
    sub = adata[:, keep]
    adata.X, adata.var = sub.X, sub.var
    adata.varm = sub.varm
    return adata


def filter_cells(adata, min_counts: float | None = None, min_genes: int | None = None):
    adata = to_lite(adata)
    X = adata.X
    if min_counts is not None:
        tot = _row_sums(X)
        keep = tot >= min_counts
        adata.obs["n_counts"] = tot
    else:
        ng = np.asarray((X > 0).sum(axis=1)).reshape(-1)
        keep = ng >= min_genes
        adata.obs["n_genes"] = ng
    sub = adata[keep, :]
    adata.X, adata.obs, adata.obsm = sub.X, sub.obs, sub.obsm
    adata.layers = sub.layers
    return adata


# ----------------------------------------------------------------------------- loess
def _loess_device(device, device_csr=None) -> torch.device:
    """Where the native fit runs: with the resident counts, else ``device``, else the GPU
    when one is visible."""
    if device_csr is not None:
        return torch.device(device_csr.device)
    if device is not None:
        return torch.device(device)
    from ..utils.gpu import visible

    return torch.device("cuda") if visible() else torch.device("cpu")


def loess_fit(x: np.ndarray, y: np.ndarray, span: float = 0.3, degree: int = 2,
              device=None, backend: str = "direct") -> np.ndarray:
    """Direct local polynomial regression (tricube weights, nearest span*n points).

    Batched on the device: for each evaluation point the k nearest neighbours are
    found by sorting x once and sliding a window, then a weighted least-squares fit of
    the given degree is solved for all points at once.

    ``backend="native"`` computes the same fit with ``ops.loess`` in O(n) memory on
    ``device`` (None: the GPU when one is visible; loess.hip there, the float64 reference
    on the CPU); ``"direct"`` (default) holds (n, k) windows."""
    if backend not in ("direct", "native"):
        raise ValueError(f"loess_fit: backend must be 'direct' or 'native', not {backend!r}")
    if backend == "native":
        from .. import ops

        dev = _loess_device(device)
        xt = torch.from_numpy(np.array(x, dtype=np.float64)).to(dev)
        yt = torch.from_numpy(np.array(y, dtype=np.float64)).to(dev)
        return ops.loess(xt, yt, span=span, degree=degree).cpu().numpy()
    n = x.shape[0]
    k = max(degree + 1, int(np.ceil(span * n)))
    k = min(k, n)
    order = np.argsort(x, kind="mergesort")
    xs, ys = x[order].astype(np.float64), y[order].astype(np.float64)
    # window start for each point: nearest-k contiguous window in sorted order
    starts = np.zeros(n, dtype=np.int64)
    lo = 0
    for i in range(n):
        if lo > i:
            lo = i
        while lo + k < n and (xs[lo + k] - xs[i]) < (xs[i] - xs[lo]):
            lo += 1
        lo = min(lo, n - k)
        starts[i] = lo
    dev = torch.device(device) if device is not None else torch.device("cpu")
    X = torch.as_tensor(xs, device=dev)
    Y = torch.as_tensor(ys, device=dev)
    idx = torch.as_tensor(starts, device=dev)[:, None] + torch.arange(k, device=dev)[None, :]
    xw = X[idx]                                   # (n, k)
    yw = Y[idx]
    d = torch.abs(xw - X[:, None])
    h = d.max(dim=1, keepdim=True).values
    h = torch.where(h > 0, h * 1.0000001, torch.ones_like(h))
    w = torch.clamp(1 - (d / h) ** 3, min=0) ** 3
    cols = [torch.ones_like(xw)]
    for p in range(1, degree + 1):
        cols.append((xw - X[:, None]) ** p)
    V = torch.stack(cols, dim=2)                  # (n, k, degree+1)
    Vw = V * w[..., None]
    A = Vw.transpose(1, 2) @ V
    b = (Vw.transpose(1, 2) @ yw[..., None])
    A = A + 1e-10 * torch.eye(degree + 1, device=dev, dtype=A.dtype)
    coef = torch.linalg.solve(A, b)[..., 0]
    fitted_sorted = coef[:, 0].cpu().numpy()
    out = np.empty(n)
    out[order] = fitted_sorted
    return out


def _loess_ragged(stats, span: float, dev: torch.device) -> list:
    """The fits of log10 variance on log10 mean over the genes of non-zero variance of every
    batch in ``stats`` ((mean, var) per batch), as one ragged ``ops.loess`` call on ``dev``."""
    from .. import ops

    xs = [np.log10(mean[var > 0]) for mean, var in stats]
    ys = [np.log10(var[var > 0]) for _, var in stats]
    off = np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])]).astype(np.int64)
    fit = ops.loess(torch.from_numpy(np.concatenate(xs)).to(dev),
                    torch.from_numpy(np.concatenate(ys)).to(dev), offsets=off,
                    span=span).cpu().numpy()
    return [fit[a:b] for a, b in zip(off[:-1], off[1:])]


def _norm_var_resident(device_csr, m_t: torch.Tensor, v_t: torch.Tensor, span: float):
    """Normalised variance of every gene of one batch held as a DeviceCSR, from its device
    mean ``m_t`` and variance ``v_t``: the fit (``ops.loess``), the clip and the clipped
    moments stay on the device; the result comes back as a numpy array."""
    from .. import ops
    from ..ops import sparse as sops

    N = device_csr.shape[0]
    not_const = v_t > 0
    est = torch.zeros_like(m_t)
    est[not_const] = ops.loess(torch.log10(m_t[not_const]), torch.log10(v_t[not_const]),
                               span=span)
    reg_std = torch.sqrt(10 ** est)
    s1, sq, _ = sops.col_stats(device_csr, clip=reg_std * np.sqrt(N) + m_t)
    nv = (1.0 / ((N - 1) * reg_std ** 2)) * (N * m_t ** 2 + sq - 2 * s1 * m_t)
    return torch.nan_to_num(nv, nan=0.0).cpu().numpy()


def highly_variable_genes(adata, flavor: str = "seurat_v3", n_top_genes: int = 2000,
                          batch_key: str | None = None, span: float = 0.3, inplace: bool = True,
                          device_csr=None, loess: str = "direct", device=None):
    """Seurat v3 HVG selection on raw counts (preprocess.py:295).

    ``device_csr``: the same counts already resident on the GPU as an
    :class:`ops.sparse.DeviceCSR` -- the per-gene mean/variance and the clipped second
    moments are then column-statistics kernels over the stored entries (one batch).

    ``loess``: ``"direct"`` (default) fits with :func:`loess_fit` as it stands, one call per
    batch on the CPU.  ``"native"`` fits all batches in one ragged ``ops.loess`` call in O(n)
    memory, on the device of ``device_csr`` when that is given (the means, variances and the
    clip then stay there), else on ``device`` (None: the GPU when one is visible)."""
    if flavor != "seurat_v3":
        raise NotImplementedError("only flavor='seurat_v3' is used by Preprocess")
    if loess not in ("direct", "native"):
        raise ValueError(f"highly_variable_genes: loess must be 'direct' or 'native', "
                         f"not {loess!r}")
    adata = to_lite(adata)
    X = adata.X
    batches = (pd.Series(np.zeros(adata.n_obs, dtype=int)) if batch_key is None
               else adata.obs[batch_key].astype("category").cat.codes.reset_index(drop=True))
    norm_vars = []
    dev_stats = device_csr is not None and batch_key is None
    if dev_stats:
        from ..ops import sparse as sops

        m_t, v_t = sops.mean_var(device_csr, ddof=1)
        means_all, vars_all = m_t.cpu().numpy(), v_t.cpu().numpy()
    else:
        means_all, vars_all = _mean_var_ddof1(X)
    batch_ids = np.unique(batches.values)
    stats = fits = None
    if loess == "native" and dev_stats:
        # one batch on the resident counts: statistics, fit and clip stay on the device
        norm_vars.append(_norm_var_resident(device_csr, m_t, v_t, span))
        batch_ids = batch_ids[:0]
    elif loess == "native":
        stats = [_mean_var_ddof1(X[np.flatnonzero(batches.values == b)]) for b in batch_ids]
        fits = _loess_ragged(stats, span, _loess_device(device, device_csr))
    for bi, b in enumerate(batch_ids):
        rows = np.flatnonzero(batches.values == b)
        Xb = X if dev_stats else X[rows]
        if stats is not None:
            mean, var = stats[bi]
        else:
            mean, var = (means_all, vars_all) if dev_stats else _mean_var_ddof1(Xb)
        not_const = var > 0
        est = np.zeros(X.shape[1], dtype=np.float64)
        if fits is not None:
            est[not_const] = fits[bi]
        else:
            est[not_const] = loess_fit(np.log10(mean[not_const]), np.log10(var[not_const]),
                                       span=span)
        reg_std = np.sqrt(10 ** est)
        N = Xb.shape[0]
        clip = reg_std * np.sqrt(N) + mean
        if dev_stats:
            s1_t, sq_t, _ = sops.col_stats(device_csr, clip=clip)
            s1, sq = s1_t.cpu().numpy(), sq_t.cpu().numpy()
        elif sp.issparse(Xb):
            Xc = sp.csr_matrix(Xb, dtype=np.float64, copy=True)
            Xc.data = np.minimum(Xc.data, clip[Xc.indices])
            sq = np.asarray(Xc.multiply(Xc).sum(axis=0)).reshape(-1)
            s1 = np.asarray(Xc.sum(axis=0)).reshape(-1)
        else:
            Xc = np.minimum(np.asarray(Xb, dtype=np.float64), clip[None, :])
            sq = (Xc ** 2).sum(axis=0)
            s1 = Xc.sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            nv = (1.0 / ((N - 1) * reg_std ** 2)) * (N * mean ** 2 + sq - 2 * s1 * mean)
        norm_vars.append(np.nan_to_num(nv, nan=0.0))
    norm_vars = np.vstack(norm_vars)
    ranked = np.argsort(np.argsort(-norm_vars, axis=1, kind="stable"), axis=1, kind="stable").astype(float)
    ranked[ranked >= n_top_genes] = np.nan
    n_batches = (~np.isnan(ranked)).sum(axis=0)
    with np.errstate(all="ignore"):
        median_rank = np.nanmedian(ranked, axis=0)
    df = pd.DataFrame({"means": means_all, "variances": vars_all,
                       "variances_norm": norm_vars.mean(axis=0),
                       "highly_variable_rank": median_rank,
                       "highly_variable_nbatches": n_batches}, index=adata.var.index)
    srt = df.sort_values(["highly_variable_nbatches", "highly_variable_rank"],
                         ascending=[False, True], na_position="last")
    hv = np.zeros(len(df), dtype=bool)
    hv[df.index.get_indexer(srt.index[:n_top_genes])] = True
    df["highly_variable"] = hv
    for c in df.columns:
        adata.var[c] = df[c].values
    return adata if inplace else df


def pca(adata, n_comps: int = 50, zero_center: bool = True, use_highly_variable: bool = False,
        device=None, random_state: int = 0, backend: str = "dense"):
    """Zero-centred PCA -> obsm['X_pca'], varm['PCs'], uns['pca'] (preprocess.py:310).

    ``backend="dense"`` (default) densifies ``X`` into a float64 tensor on ``device``;
    ``"csr"`` keeps a sparse ``X`` as a CSR on ``device`` (the HVG subset a col_map) and
    factorises it with :func:`pca_csr` -- no dense copy anywhere."""
    if backend not in ("dense", "csr"):
        raise ValueError(f"pca: backend must be 'dense' or 'csr', not {backend!r}")
    adata = to_lite(adata)
    X = adata.X
    cols = np.arange(adata.n_vars)
    if use_highly_variable and "highly_variable" in adata.var:
        cols = np.flatnonzero(adata.var["highly_variable"].values)
    dev = torch.device(device) if device is not None else torch.device("cpu")
    if backend == "csr":
        if not sp.issparse(X):
            raise ValueError("pca: backend='csr' needs a sparse X")
        from ..ops import sparse as sops

        A = sops.DeviceCSR.from_scipy(X, device=dev)
        if cols.size != adata.n_vars:
            cmap = np.full(adata.n_vars, -1, np.int32)
            cmap[cols] = np.arange(cols.size, dtype=np.int32)
            A = A.view(col_map=cmap, n_out=int(cols.size))
        Xp, Vh, var, ratio = pca_csr(A, n_comps, zero_center)
    else:
        Xs = X[:, cols]
        Xd = Xs.toarray() if sp.issparse(Xs) else np.asarray(Xs)
        T = torch.as_tensor(Xd, dtype=torch.float64, device=dev)
        Xp, Vh, var, ratio = pca_tensor(T, n_comps, zero_center)
    adata.obsm["X_pca"] = Xp
    PCs = np.zeros((adata.n_vars, Vh.shape[0]))
    PCs[cols] = Vh.T
    adata.varm["PCs"] = PCs
    adata.uns["pca"] = {"variance": var, "variance_ratio": ratio}
    return adata


def _clamp_comps(n_comps: int, shape) -> int:
    return min(n_comps, min(shape) - 1) if min(shape) > 1 else 1


def _pca_from_cov(C: torch.Tensor, n: int, n_comps: int, scores, total):
    """The tail pca_tensor and pca_csr share: top ``n_comps`` eigenpairs of the (features x
    features) matrix ``C`` = T^T T of the centred data, ``scores(Vh)`` = T @ Vh^T, the sign
    rule and the variances (``total()`` = sum of squares of T).  Returns numpy (scores,
    components, variance, variance_ratio)."""
    dev = C.device
    evals, evecs = torch.linalg.eigh(C)
    order = torch.argsort(evals, descending=True)[:n_comps]
    S = torch.sqrt(torch.clamp(evals[order], min=0.0))
    Vh = evecs[:, order].t()
    XS = scores(Vh)                                     # = U * S
    # deterministic sign: largest |score| positive (sklearn svd_flip u-based)
    sign = torch.sign(XS[torch.argmax(torch.abs(XS), dim=0), torch.arange(XS.shape[1], device=dev)])
    sign[sign == 0] = 1
    XS, Vh = XS * sign, Vh * sign[:, None]
    var = (S ** 2 / max(n - 1, 1)).cpu().numpy()
    total = total() / max(n - 1, 1)
    return XS.cpu().numpy(), Vh.cpu().numpy(), var, (var / total if total > 0 else var)


def pca_tensor(T: torch.Tensor, n_comps: int = 50, zero_center: bool = True):
    """Zero-centred PCA of a (cells x features) tensor on its device (float64):
    returns numpy (scores (n, c), components (c, features), variance, variance_ratio)."""
    T = T.to(torch.float64)
    if zero_center:
        T = T - T.mean(dim=0, keepdim=True)
    n_comps = _clamp_comps(n_comps, T.shape)
    # top components from the (genes x genes) Gram matrix: one GEMM + a small eigh instead
    # of a thin SVD of the whole (cells x genes) matrix (3.5 s -> ~0.1 s at 100k x 2k)
    C = T.t() @ T
    return _pca_from_cov(C, T.shape[0], n_comps, lambda Vh: T @ Vh.t(),
                         lambda: float((T ** 2).sum().cpu()))


def pca_csr(A, n_comps: int = 50, zero_center: bool = True, value_dtype=torch.float64):
    """:func:`pca_tensor` of the matrix a :class:`ops.sparse.DeviceCSR` view stands for
    (``densify(A, out_dtype=value_dtype)``) without building it: the covariance
    T^T T - n mu mu^T from ``ops.sparse.gram`` and the column sums, the scores
    T V - mu V from ``ops.sparse.project`` (pca_csr.hip on the GPU; docs/ARCHITECTURE.md
    "Sparse PCA").  Same return value, sign rule and ``n_comps`` clamp."""
    from ..ops import sparse as sops

    n = A.shape[0]
    B = sops.valued(A, value_dtype)          # the transform applied once, O(nnz)
    C = sops.gram(B)
    mu = None
    if zero_center:
        mu = sops.col_stats(B)[0] / n
        C = C - n * torch.outer(mu, mu)
    return _pca_from_cov(
        C, n, _clamp_comps(n_comps, A.shape),
        lambda Vh: sops.project(B, Vh.t(), None if mu is None else Vh @ mu),
        lambda: float(torch.trace(C).cpu()))
