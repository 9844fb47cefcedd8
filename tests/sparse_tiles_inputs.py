"""Inputs shared by test_sparse_tiles_cpu.py and test_gemm_tiles_gpu.py (no tests here)."""
import numpy as np


def count_matrix(N: int, G: int, two_planes: bool = False, blocks: bool = False):
    """(X float32, C int64): sparse Poisson counts over a per-gene std, the shape of cNMF's
    normalised counts.  Column 5 is empty.  ``two_planes``: column 7 holds counts up to
    3000 (two bf16 planes).  ``blocks``: genes 64..127 are empty and the tile of cells
    64..127 x genes 0..63 is completely filled."""
    rs = np.random.default_rng(0)
    C = rs.poisson(rs.gamma(0.3, 0.3, (1, G)), (N, G)).astype(np.int64)
    C[:, 5] = 0
    if two_planes:
        C[:, 7] = rs.integers(0, 3001, N)
        C[0, 7] = 3000
    if blocks:
        C[:, 64:128] = 0
        C[64:128, 0:64] = rs.integers(1, 9, (64, 64))
    sd = C.std(axis=0, ddof=1)
    sd[sd == 0] = 1.0
    return (C / sd).astype(np.float32), C


def float_matrix(N: int, G: int, blocks: bool = False) -> np.ndarray:
    """Non-count data: normalised counts thresholded to 10 % non-zero (no per-gene unit
    survives, so the holder takes the float planes)."""
    from cnmf_torch_amd.utils.synthetic import normalized_counts_matrix

    X = normalized_counts_matrix(N, G, n_programs=4, seed=2).astype(np.float32)
    X[X < np.quantile(X, 0.9)] = 0.0
    if blocks:
        rs = np.random.default_rng(1)
        X[:, 64:128] = 0.0
        X[64:128, 0:64] = rs.uniform(0.5, 3.0, (64, 64)).astype(np.float32)
    return X
