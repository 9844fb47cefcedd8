"""Tile storage against dense storage on the bench shape, and the two data-side kernels
alone.

    python tools/bench_sparse_x.py                      # replicates/s, 3 densities, 3 rounds
    python tools/bench_sparse_x.py --kernels tiles      # the kernels alone, for a profiler
    python tools/bench_sparse_x.py --kernels dense

Default mode: 10,000 cells x 2,000 genes, K = 10, 100 replicates of sparse Poisson counts
over the per-gene std at about 3 %, 8 % and 15 % non-zero; one process runs dense storage
with the fused step, dense storage with CNMF_FUSED_STEP=0 (the like-for-like unfused
passes) and tile storage (models.nmf.SparseTilesX) in alternation.  One JSON line per
density.  ``--kernels``: the numerator and statistics products at M = 1000 rows on a
5000-cell chunk of the 8 % matrix with random fp32 operands, a fixed number of calls of
one storage mode (run it under a kernel-trace profiler, one run per mode).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from cnmf_torch_amd import ops  # noqa: E402
from cnmf_torch_amd.models.nmf import (NMFBatchSolver, NMFOptions, SparseTilesX,  # noqa: E402
                                       _XPlanes)


def counts(N, G, density, seed=0):
    """X = C / std for C ~ Poisson(lambda_g), lambda_g ~ Gamma(0.3, s): the expected
    non-zero fraction 1 - (1 + s)^-0.3 solved for s."""
    rs = np.random.default_rng(seed)
    s = (1.0 - density) ** (-1.0 / 0.3) - 1.0
    C = rs.poisson(rs.gamma(0.3, s, (1, G)), (N, G))
    sd = C.std(axis=0, ddof=1)
    sd[sd == 0] = 1.0
    return (C / sd).astype(np.float32)


def timed(solver, seeds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = solver.run(seeds)
    _ = res.W.cpu()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, float(np.mean(res.n_iter)), float(np.mean(res.err))


def throughput(a):
    dev = torch.device("cuda")
    opts = NMFOptions(n_components=a.k, tol=1e-4, online_chunk_size=5000,
                      online_chunk_max_iter=1000)
    np.random.seed(14)
    seeds = [int(s) for s in np.random.randint(1, 2 ** 31 - 1, size=a.reps)]
    for density in a.densities:
        X = counts(a.cells, a.genes, density)
        nnz = float((X != 0).mean())
        Xd = torch.from_numpy(X).to(dev)
        holder = SparseTilesX.from_scipy(sp.csr_matrix(X), device=dev)
        modes = {"dense_fused": (Xd, "1"), "dense_unfused": (Xd, "0"), "tiles": (holder, "1")}
        solvers, rate, info = {}, {m: [] for m in modes}, {}
        for m, (x, fused) in modes.items():           # build + warm up (planes, workspaces)
            os.environ["CNMF_FUSED_STEP"] = fused
            solvers[m] = NMFBatchSolver(x, opts)
            timed(solvers[m], seeds)
        for _ in range(a.rounds):
            for m, (x, fused) in modes.items():
                os.environ["CNMF_FUSED_STEP"] = fused
                el, passes, err = timed(solvers[m], seeds)
                rate[m].append(a.reps / el)
                info[m] = (passes, err)
        os.environ.pop("CNMF_FUSED_STEP", None)
        med = {m: float(np.median(v)) for m, v in rate.items()}
        xp = solvers["dense_fused"]._planes()
        print(json.dumps({
            "shape": [a.cells, a.genes], "k": a.k, "replicates": a.reps,
            "nonzero_fraction": round(nnz, 4), "planes": holder.pb,
            "replicates_per_s": {m: [round(v, 1) for v in rate[m]] for m in modes},
            "median": {m: round(v, 1) for m, v in med.items()},
            "tiles_over_dense_unfused": round(med["tiles"] / med["dense_unfused"], 3),
            "tiles_over_dense_fused": round(med["tiles"] / med["dense_fused"], 3),
            "mean_passes": {m: round(info[m][0], 2) for m in modes},
            "mean_err": {m: round(info[m][1], 4) for m in modes},
            "tile_bytes": holder.nbytes,
            "plane_bytes": 2 * (xp.x.numel() + xp.xt.numel()) if xp is not None else None,
            "fp32_bytes": 4 * a.cells * a.genes}), flush=True)
        del solvers, Xd, holder


def kernels(a):
    dev = torch.device("cuda")
    N, G, M = 5000, a.genes, 1000
    X = counts(N, G, 0.08)
    g = torch.Generator().manual_seed(0)
    W = torch.rand((M, G), generator=g).to(dev)
    HT = torch.rand((M, N), generator=g).to(dev)
    if a.kernels == "tiles":
        h = SparseTilesX.from_scipy(sp.csr_matrix(X), device=dev)
        Gp, unit, pb = h.Gp, h.unit, h.pb
    else:
        h = _XPlanes(torch.from_numpy(X).to(dev))
        Gp, unit, pb = h.Gp, h.unit, h.pb
    kd = -(-N // 64) * 64
    wpl = torch.zeros((3, M, Gp), dtype=torch.int16, device=dev)
    hpl = torch.zeros((3, M, kd), dtype=torch.int16, device=dev)
    ops.split_planes(W, wpl, col_mul=unit)
    ops.split_planes(HT, hpl)
    wa, ha = wpl[:ops.gemm_a_planes(Gp)], hpl[:ops.gemm_a_planes(kd)]
    numer = torch.empty((M, N), device=dev)
    B = torch.empty((M, G), device=dev)
    for _ in range(a.calls):
        if a.kernels == "tiles":
            ops.gemm_tiles(numer, wa, h.tiles, "n", 0, N, M)
            ops.gemm_tiles(B, ha, h.tiles, "s", 0, N, M, col_scale=unit)
        else:
            ops.gemm_planes(numer, wa, h.x, M, N, Gp)
            ops.gemm_planes(B, ha, h.xt, M, G, kd, col_scale=unit)
    torch.cuda.synchronize()
    print(json.dumps({"kernels": a.kernels, "M": M, "cells": N, "genes": G, "planes": pb,
                      "calls": a.calls, "nonzero_fraction": round(float((X != 0).mean()), 4),
                      "numer_checksum": float(numer.double().sum()),
                      "stats_checksum": float(B.double().sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--densities", type=float, nargs="+", default=[0.03, 0.08, 0.15])
    ap.add_argument("--kernels", choices=["tiles", "dense"], default=None)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    (kernels if a.kernels else throughput)(a)


if __name__ == "__main__":
    main()
