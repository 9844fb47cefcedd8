"""LOESS for the Seurat v3 HVG selection: the native backend (ops.loess, loess.hip) against
the direct fit of models/pp.py ``loess_fit`` on the same machine and the same input.

    python tools/bench_loess.py [--native 3000,12000,30000 --direct-cpu 3000,12000
                                 --direct-gpu 12000]

The input is a synthetic log10 mean / log10 variance series with ties: count-like means c / N
(N = 5,000 cells, c a gamma-Poisson total) and a variance following an overdispersed trend
with noise.  Every native size runs after a warm-up call at 500 points that loads the code
objects: once timed as a whole (host arrays in, host array out, upload and download
included), then 7 times on device tensors and 7 times with a device synchronise after the
sort, the windows kernel and the fit kernel (medians are reported), and
``torch.cuda.max_memory_allocated`` over the calls is reported.  ``direct`` runs on the CPU
at ``--direct-cpu`` and with ``device="cuda"`` at ``--direct-gpu`` (its temporaries are
about 5 GB at 12,000 points, so no higher).  One JSON line per run; the
native lines carry the largest |native - direct| where a direct fit of that size ran.  A GPU
is required."""
import argparse
import json
import os
import resource
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

SEED = 0
CELLS = 5000
REPEATS = 7


def make_series(n):
    rs = np.random.default_rng(SEED + n)
    c = rs.poisson(rs.gamma(0.3, 60.0, n)) + 1
    mean = c / CELLS
    var = mean * (1.0 + 0.8 * mean * CELLS ** 0.5) * np.exp(0.3 * rs.normal(size=n))
    return np.log10(mean), np.log10(var)


def sizes(text):
    return [int(v) for v in text.split(",") if v]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--native", type=sizes, default=[3000, 12000, 30000])
    ap.add_argument("--direct-cpu", type=sizes, default=[3000, 12000])
    ap.add_argument("--direct-gpu", type=sizes, default=[12000])
    a = ap.parse_args()

    import torch

    from cnmf_torch_amd import ops
    from cnmf_torch_amd.models import pp

    if not torch.cuda.is_available() or not ops.native_available():
        raise SystemExit("bench_loess: needs a GPU and the built HIP extension")
    name = torch.cuda.get_device_name(0)
    direct = {}
    for n in a.direct_cpu:
        x, y = make_series(n)
        t0 = time.perf_counter()
        direct[n] = pp.loess_fit(x, y)
        print(json.dumps({
            "bench": "loess_direct_cpu", "n": n, "k": int(np.ceil(0.3 * n)),
            "seconds": round(time.perf_counter() - t0, 4),
            "peak_rss_mb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024, 1)}),
            flush=True)
    for n in a.direct_gpu:
        x, y = make_series(n)
        pp.loess_fit(*make_series(500), device="cuda")                     # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        t0 = time.perf_counter()
        fit = pp.loess_fit(x, y, device="cuda")
        torch.cuda.synchronize()
        print(json.dumps({
            "bench": "loess_direct_gpu", "n": n, "k": int(np.ceil(0.3 * n)),
            "seconds": round(time.perf_counter() - t0, 4),
            "gpu_peak_mb": round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1),
            "max_abs_vs_direct_cpu": (float(np.abs(fit - direct[n]).max())
                                      if n in direct else None),
            "device": name}), flush=True)
        del fit
        torch.cuda.empty_cache()
    for n in a.native:
        x, y = make_series(n)
        pp.loess_fit(*make_series(500), backend="native", device="cuda")   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = pp.loess_fit(x, y, backend="native", device="cuda")
        total = time.perf_counter() - t0
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        on_device, parts = [], []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            ops.loess(xd, yd)
            torch.cuda.synchronize()
            on_device.append(time.perf_counter() - t0)
        peak = torch.cuda.max_memory_allocated() - before
        for _ in range(REPEATS):
            tm = {}
            ops.loess(xd, yd, timings=tm)
            parts.append(tm)
        on_device = float(np.median(on_device))
        tm = {key: float(np.median([p[key] for p in parts])) for key in parts[0]}
        print(json.dumps({
            "bench": "loess_native", "n": n, "k": int(np.ceil(0.3 * n)),
            "distinct_x": int(np.unique(x).size),
            "total_s": round(total, 5), "on_device_s": round(on_device, 5),
            "sort_s": round(tm["sort"], 5), "windows_kernel_s": round(tm["windows"], 5),
            "fit_kernel_s": round(tm["fit"], 5),
            "gpu_peak_bytes": int(peak), "gpu_peak_bytes_per_point": round(peak / n, 1),
            "max_abs_vs_direct_cpu": (float(np.abs(fit - direct[n]).max())
                                      if n in direct else None),
            "max_abs_y": float(np.abs(y).max()), "device": name}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
