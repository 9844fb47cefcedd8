"""Mutual-information feature ranking: the native backend (models.mi, mi_cd.hip) against
scikit-learn's mutual_info_classif on the same machine and the same input.

    python tools/bench_mi.py [--cells 100000 --features 64 --classes 20 --zeros 0.8]

The input comes from utils.synthetic.simulate_counts with ``--classes`` programs: the label
of a cell is its strongest program, the features are the first ``--features`` genes scaled
to unit variance, and everything below the ``--zeros`` quantile is set to 0.  Both backends
run once with n_neighbors = 3 and the same seed; the native one after a warm-up call at
2,000 cells that loads the code objects.  scikit-learn runs in a child process (CPU only)
under ``--sklearn-limit`` seconds.  One JSON line: the native prepare / sort / kernel
seconds (each ended by a device synchronise) and the whole native call, the scikit-learn
seconds, and the largest |MI_native - MI_sklearn| over the features.  A GPU is required."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

SEED = 0


def make_input(a):
    from cnmf_torch_amd.utils.synthetic import simulate_counts

    genes = max(a.features, 4 * a.classes)
    X, _, _, U, _ = simulate_counts(a.cells, genes, a.classes, seed=SEED, sparse=False,
                                    return_truth=True)
    X = X[:, :a.features].astype(np.float64)
    sd = X.std(axis=0)
    X /= np.where(sd > 0, sd, 1.0)
    X[X < np.quantile(X, a.zeros)] = 0.0
    return X, U.argmax(axis=1)


def sklearn_child(path):
    from sklearn.feature_selection import mutual_info_classif

    d = np.load(path + ".in.npz")
    t0 = time.perf_counter()
    mi = mutual_info_classif(d["X"], d["y"], discrete_features="auto", n_neighbors=3,
                             copy=True, random_state=SEED)
    np.savez(path + ".out.npz", mi=mi, seconds=time.perf_counter() - t0)


def run_sklearn(X, y, limit):
    """(seconds, mi) of scikit-learn in a CPU-only child process, (None, None) when it is
    skipped (``limit`` <= 0), fails or runs past ``limit`` seconds.  The parent waits for it
    before the native run, so neither is timed under the other's load."""
    if limit <= 0:
        return None, None
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "mi")
        np.savez(path + ".in.npz", X=X, y=y)
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--sklearn-child",
                                  path], env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
        try:
            child.wait(timeout=limit)
        except subprocess.TimeoutExpired:
            child.kill()
            child.wait()
            return None, None
        if child.returncode != 0:
            return None, None
        out = np.load(path + ".out.npz")
        return float(out["seconds"]), out["mi"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--zeros", type=float, default=0.8)
    ap.add_argument("--sklearn-limit", type=float, default=300.0)
    ap.add_argument("--sklearn-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.sklearn_child:
        sklearn_child(a.sklearn_child)
        return 0

    import torch

    from cnmf_torch_amd import ops
    from cnmf_torch_amd.models.mi import mutual_info_classif_native

    if not torch.cuda.is_available() or not ops.native_available():
        raise SystemExit("bench_mi: needs a GPU and the built HIP extension")
    X, y = make_input(a)
    sizes = np.bincount(y)
    sk_s, sk_mi = run_sklearn(X, y, a.sklearn_limit)
    mutual_info_classif_native(X[:2000], y[:2000], random_state=SEED, device="cuda")   # warm-up
    torch.cuda.synchronize()
    tm = {}
    t0 = time.perf_counter()
    mi = mutual_info_classif_native(X, y, n_neighbors=3, random_state=SEED, device="cuda",
                                    timings=tm)
    torch.cuda.synchronize()
    native_s = time.perf_counter() - t0
    print(json.dumps({
        "bench": "mi_native", "cells": a.cells, "features": a.features,
        "classes": int(sizes.size), "smallest_class": int(sizes.min()),
        "zero_fraction": round(float((X == 0).mean()), 4), "n_neighbors": 3,
        "native_prepare_s": round(tm["prepare"], 4), "native_sort_s": round(tm["sort"], 4),
        "native_kernel_s": round(tm["kernel"], 4), "native_total_s": round(native_s, 4),
        "sklearn_s": None if sk_s is None else round(sk_s, 3),
        "sklearn_limit_s": a.sklearn_limit,
        "max_abs_dmi": None if sk_mi is None else float(np.abs(mi - sk_mi).max()),
        "mi_max": float(mi.max()),
        "device": torch.cuda.get_device_name(0)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
