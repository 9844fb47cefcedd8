"""Mutual information between continuous features and class labels without scikit-learn.

``mutual_info_classif_native`` computes what ``sklearn.feature_selection.
mutual_info_classif`` computes for a dense matrix (every feature continuous, the target
discrete; Ross 2014): the same scaling and noise stream, the same neighbour radius and
the same squared-distance count.  In one dimension the estimator needs no tree: a sort,
the k-th same-class neighbour on either side, and a search for the last point inside the
radius (``ops.mi_cd``; mi_cd.hip on the GPU, ``ops.reference.mi_cd`` on the CPU).

One deliberate difference: for classes of 3 to 7 points scikit-learn's neighbour search
takes its brute-force path, whose distances come from the expanded square
``x^2 + y^2 - 2xy`` and cancel badly at the 1e-10 noise scale.  This backend uses exact
differences for every class size and does not imitate that cancellation; with every class
of 2 or of >= 8 points the two agree to 1e-15.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import ops
from ..ops import reference


def _device(device):
    if device is not None:
        return torch.device(device)
    env = os.environ.get("CNMF_DEVICE")
    if env:
        return torch.device(env)
    from ..utils.gpu import visible

    return torch.device("cuda") if visible() else torch.device("cpu")


def mutual_info_classif_native(X, labels, n_neighbors: int = 3, random_state=None,
                               device=None, timings: dict | None = None) -> np.ndarray:
    """(G,) float64 mutual information in nats of every column of the dense matrix ``X``
    (n, G) against ``labels`` (n,), clamped at 0 -- ``mutual_info_classif(X, labels,
    discrete_features=False, n_neighbors=n_neighbors, random_state=random_state)``.
    ``device=None``: the GPU when one is visible (``CNMF_DEVICE`` overrides)."""
    dev = _device(device)
    X = np.asarray(X)
    labels = np.asarray(labels).reshape(-1)
    if X.ndim != 2 or labels.shape[0] != X.shape[0]:
        raise ValueError("mutual_info_classif_native: X (n, G) and one label per row")
    codes = np.unique(labels, return_inverse=True)[1].reshape(-1)
    if timings is not None:
        import time
        t0 = time.perf_counter()
    Xp = reference.mi_prepare(X, random_state)
    if timings is not None:
        timings["prepare"] = time.perf_counter() - t0
    mi = ops.mi_cd(torch.from_numpy(Xp).to(dev), codes, n_neighbors=n_neighbors,
                   timings=timings if dev.type == "cuda" else None)
    return torch.clamp(mi, min=0.0).cpu().numpy()
