"""KL on csr storage against dense storage: replicates/s, peak device bytes, tile build time.

    python tools/bench_kl_storage.py                            # 10k x 2k, 8 %, K = 10
    python tools/bench_kl_storage.py --k 80
    python tools/bench_kl_storage.py --cells 1000000 --reps 2 --passes 2 --only csr

The matrix of ``bench.py --beta-loss kullback-leibler --density D``
(utils.synthetic.normalized_counts_matrix, thresholded at the quantile).  Dense storage
(the resident fp32 matrix, CSR kernels forced: CNMF_KL_SPARSE=1) and csr storage
(models.nmf.SparseCSRX) run in alternation, each run on a fresh solver so that its peak
device bytes (max_memory_allocated over the run, including the matrix it holds) are its
own.  One JSON line per run, then one line with the time to build every chunk's transposed
tiles by csr_transpose.hip (ops.kl_csr_tiles_from_csr) and by the dense-slice builder
(ops.kl_csr_tiles).  ``--only csr`` never makes the dense matrix on the device.
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
from cnmf_torch_amd.models.nmf import NMFBatchSolver, NMFOptions, SparseCSRX  # noqa: E402
from cnmf_torch_amd.models.nmf_base import _chunks  # noqa: E402
from cnmf_torch_amd.utils.synthetic import normalized_counts_matrix  # noqa: E402


def matrix(a):
    """The host matrix as scipy CSR, made in row blocks (the threshold from the first)."""
    rows, parts, thr = 100000, [], None
    for i, r0 in enumerate(range(0, a.cells, rows)):
        X = normalized_counts_matrix(min(rows, a.cells - r0), a.genes, n_programs=a.k, seed=i)
        if thr is None:
            thr = np.quantile(X, 1.0 - a.density)
        X[X < thr] = 0.0
        parts.append(sp.csr_matrix(X))
    return sp.vstack(parts, format="csr")


def one_run(a, storage, m, opts, seeds, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    if storage == "csr":
        x = SparseCSRX.from_scipy(m, device=dev)
    else:
        x = torch.from_numpy(m.toarray()).to(dev)
    solver = NMFBatchSolver(x, opts)
    solver.run(seeds[:2])                       # warm up: CSR, tiles, workspaces
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = solver.run(seeds)
    _ = res.W.cpu()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated() - base
    print(json.dumps({
        "storage": storage, "shape": [a.cells, a.genes], "k": a.k, "replicates": a.reps,
        "nonzero_fraction": round(m.nnz / (a.cells * a.genes), 4),
        "replicates_per_s": round(a.reps / el, 2), "wall_s": round(el, 3),
        "peak_device_bytes": int(peak), "fp32_bytes": 4 * a.cells * a.genes,
        "mean_passes": round(float(np.mean(res.n_iter)), 2),
        "mean_err": round(float(np.mean(res.err)), 4)}), flush=True)
    del solver, x, res


def build_times(a, m, dev):
    """Every chunk's transposed tiles: the new kernel from the device CSR, and the
    dense-slice builder (unless --only csr)."""
    h = SparseCSRX.from_scipy(m, device=dev)
    chunks = [(c0, c1) for c0, c1 in _chunks(a.cells, a.chunk, -(-a.cells // a.chunk)) if c1 > c0]

    def timed(f, n=3):
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for c0, c1 in chunks:
                f(c0, c1)
            torch.cuda.synchronize()
            out.append(round((time.perf_counter() - t0) * 1e3, 3))
        return out

    rec = {"tile_build_ms": {"chunks": len(chunks), "tile_rows": ops.kl_tile_rows(a.k)}}
    rec["tile_build_ms"]["from_csr"] = timed(
        lambda c0, c1: ops.kl_csr_tiles_from_csr(ops.kl_csr_rows(h.csr, c0, c1), a.k))
    if a.only != "csr":
        Xd = torch.from_numpy(m.toarray()).to(dev)
        rec["tile_build_ms"]["from_dense"] = timed(lambda c0, c1: ops.kl_csr_tiles(Xd[c0:c1], a.k))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--density", type=float, default=0.08)
    ap.add_argument("--chunk", type=int, default=5000)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=["csr", "dense"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    os.environ["CNMF_KL_SPARSE"] = "1"
    opts = NMFOptions(n_components=a.k, beta_loss="kullback-leibler", tol=1e-4,
                      online_chunk_size=a.chunk, online_chunk_max_iter=1000,
                      online_max_pass=a.passes)
    np.random.seed(14)
    seeds = [int(s) for s in np.random.randint(1, 2 ** 31 - 1, size=a.reps)]
    m = matrix(a)
    for _ in range(a.rounds):
        for storage in ("dense", "csr"):
            if a.only in (None, storage):
                one_run(a, storage, m, opts, seeds, dev)
    build_times(a, m, dev)


if __name__ == "__main__":
    main()
