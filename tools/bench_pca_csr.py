"""Sparse PCA (pca_csr.hip) against the dense path, step by step, on random sparse counts.

    python tools/bench_pca_csr.py --cells 100000 --hvg 2000 --density 0.02,0.05,0.1,0.2,0.4

For each density: a random (cells x hvg) float32 CSR of small integers is built on the
device, then timed (median of --reps, device work included):

* dense:  ``densify`` (float32), the float64 centred copy and its Gram ``T.t() @ T`` (the
  library GEMM of ``pp.pca_tensor``), and ``pp.pca_tensor`` as a whole;
* csr:    the layout pre-pass (tile packing), ``csr_gram``, the reduction over the slabs,
  ``eigh``, ``csr_project``, and ``pp.pca_csr`` as a whole;

with ``torch.cuda.max_memory_allocated`` over each whole path.  Prints one JSON line per
density.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cnmf_torch_amd.models import pp  # noqa: E402
from cnmf_torch_amd.ops import _hip, _stream_ptr  # noqa: E402
from cnmf_torch_amd.ops import sparse as sops  # noqa: E402


def random_csr(n, g, density, seed, dev, block=50000):
    gen = torch.Generator(device=dev).manual_seed(seed)
    cols, counts = [], []
    for r0 in range(0, n, block):
        m = torch.rand((min(block, n - r0), g), device=dev, generator=gen) < density
        counts.append(m.sum(1))
        cols.append(m.nonzero()[:, 1].to(torch.int32))
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.cat(counts), 0, out=indptr[1:])
    indices = torch.cat(cols)
    data = torch.randint(1, 10, (indices.numel(),), device=dev, generator=gen).float()
    return sops.DeviceCSR(indptr, indices, data, (n, g))


def timed(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        out = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 2), out


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 1e9, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--hvg", type=int, default=2000)
    ap.add_argument("--density", default="0.02,0.05,0.1,0.2,0.4")
    ap.add_argument("--comps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, nh = a.cells, a.hvg
    for i, d in enumerate(float(x) for x in a.density.split(",")):
        A = random_csr(n, nh, d, i, dev)
        ms = {}
        # dense path, as pp.pca_tensor runs it
        ms["densify"], X = timed(lambda: sops.densify(A), a.reps)
        ms["center_f64"], T = timed(lambda: X.double() - X.double().mean(0, keepdim=True), a.reps)
        ms["gemm_f64"], C = timed(lambda: T.t() @ T, a.reps)
        del T, C
        ms["pca_tensor"], _ = timed(lambda: pp.pca_tensor(X, a.comps)[0], a.reps)
        del X
        dense_peak = peak_of(lambda: pp.pca_tensor(sops.densify(A), a.comps))
        # CSR path, the steps of ops.sparse.gram / pp.pca_csr one by one
        ms["layout"], (tptr, lcol, val) = timed(lambda: sops._gram_layout(A, None), a.reps)
        S = int(_hip.csr_gram_slabs(n, nh))
        part = torch.empty((S, nh, nh), dtype=torch.float64, device=dev)
        ms["csr_gram"], _ = timed(lambda: _hip.csr_gram(
            tptr.data_ptr(), lcol.data_ptr(), val.data_ptr(), n, nh, part.data_ptr(),
            _stream_ptr(val)), a.reps)
        ms["slab_sum"], G = timed(lambda: part.sum(0), a.reps)
        del tptr, lcol, val, part
        ms["gram"], _ = timed(lambda: sops.gram(A), a.reps)
        ms["eigh"], (w, V) = timed(lambda: torch.linalg.eigh(G), a.reps)
        Vc = V[:, -a.comps:].contiguous()
        ms["csr_project"], _ = timed(lambda: sops.project(A, Vc, Vc.sum(0)), a.reps)
        del G, w, V, Vc
        ms["pca_csr"], _ = timed(lambda: pp.pca_csr(A, a.comps)[0], a.reps)
        csr_peak = peak_of(lambda: pp.pca_csr(A, a.comps))
        print(json.dumps({"cells": n, "hvg": nh, "density": d, "nnz": A.nnz, "slabs": S,
                          "ms": ms, "peak_gb": {"dense": dense_peak, "csr": csr_peak},
                          "device": torch.cuda.get_device_name(0)}), flush=True)
        del A


if __name__ == "__main__":
    main()
