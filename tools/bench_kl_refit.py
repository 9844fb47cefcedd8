"""KL refit timings: chunk-batched usage step against a per-chunk loop, the spectra refit's
time per MU step, and consensus wall time with --refit-loss match against the default.

    python tools/bench_kl_refit.py usage --cells 10000 --k 10
    python tools/bench_kl_refit.py usage --cells 100000 --k 80
    python tools/bench_kl_refit.py spectra --cells 500000 --k 10
    python tools/bench_kl_refit.py consensus --cells 10000 --k 10

``usage``: the matrix of ``bench.py --beta-loss kullback-leibler --density D``
(utils.synthetic.normalized_counts_matrix, thresholded at the quantile) as a device CSR, spectra
drawn at random, usages refit from the same seeded init by (a) ops.kl_sparse_refit -- one
launch per MU step for every full chunk -- and (b) the loop that the replicate-batched op
allows without it: ops.kl_sparse_h_block(ops.kl_csr_rows(...), R = 1, nsteps = 1,
conv_mode = 0) chunk by chunk, the host reading the chunk's flag at the same cadence (every 8
launches; launches of a finished chunk return at the gate).  The two alternate; both must take
the same steps per chunk.  ``--tol 0 --max-iter M``: M steps of every chunk, all of them
working.  One JSON line.
``spectra``: ops.csr_transpose of the matrix and 8 MU steps of the spectra refit (genes as
rows, every cell's usages as the gathered operand), no host read in between.
``consensus``: prepare / factorize / combine of a KL run, then consensus with both settings in
alternation."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from cnmf_torch_amd import ops  # noqa: E402
from cnmf_torch_amd.models import refit  # noqa: E402
from cnmf_torch_amd.utils.synthetic import normalized_counts_matrix  # noqa: E402

EPS, EVERY = 1e-16, 8


def matrix(a):
    rows, parts, thr = 100000, [], None
    for i, r0 in enumerate(range(0, a.cells, rows)):
        X = normalized_counts_matrix(min(rows, a.cells - r0), a.genes, n_programs=a.k, seed=i)
        if thr is None:
            thr = np.quantile(X, 1.0 - a.density)
        X[X < thr] = 0.0
        parts.append(sp.csr_matrix(X.astype(np.float32)))
    return sp.vstack(parts, format="csr")


def loop_refit(csr, HT, W, chunk, iters, tol, max_iter):
    """The per-chunk host loop over the replicate-batched op (R = 1 per chunk)."""
    K, n = HT.shape
    W3 = W.unsqueeze(0)
    st = ops.kl_st(W3)
    den = W3.sum(dim=2, dtype=torch.float32).contiguous()
    c, full, tail = ops.kl_refit_chunks(n, chunk)
    act = torch.ones(full + (1 if tail else 0), dtype=torch.int32, device=HT.device)
    for ci, a0 in enumerate(range(0, n, c)):
        b0 = min(n, a0 + c)
        rows = ops.kl_csr_rows(csr, a0, b0)
        h3 = HT[:, a0:b0].unsqueeze(0)
        for s in range(max_iter):
            ops.kl_sparse_h_block(rows, h3, W3, EPS, 1, act=act[ci:ci + 1], tol=tol,
                                  iters=iters[ci:ci + 1], conv_mode=0, den_vec=den, st=st)
            if (s + 1) % EVERY == 0 and not bool(act[ci]):
                break


def usage(a):
    dev = torch.device("cuda")
    m = matrix(a)
    csr = refit.kl_csr_of(m, dev)
    g = torch.Generator().manual_seed(a.k)
    W = (torch.rand((a.k, a.genes), generator=g) + 0.05).to(dev)
    H0 = refit._init_HT(a.k, a.cells, None, dev, torch.float32, 0)
    nch = -(-a.cells // a.chunk)
    res, times = {}, {"batched": [], "loop": []}

    def run(kind):
        HT = H0.clone()
        it = torch.zeros(nch, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "batched":
            ops.kl_sparse_refit(csr, HT, W, a.chunk, a.max_iter, a.tol, eps=EPS, iters=it,
                                check_every=EVERY)
        else:
            loop_refit(csr, HT, W, a.chunk, it, a.tol, a.max_iter)
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) * 1e3
        return HT, it.cpu().tolist(), el

    for kind in ("loop", "batched"):           # warm up both
        res[kind] = run(kind)[:2]
    for _ in range(a.rounds):
        for kind in ("loop", "batched"):
            times[kind].append(round(run(kind)[2], 3))
    same_steps = res["loop"][1] == res["batched"][1]
    diff = float((res["loop"][0] - res["batched"][0]).abs().max())
    lo = sorted(times["loop"])
    ba = sorted(times["batched"])
    print(json.dumps({
        "what": "usage refit", "shape": [a.cells, a.genes], "k": a.k, "chunk": a.chunk,
        "chunks": nch, "tol": a.tol, "max_iter": a.max_iter,
        "nonzero_fraction": round(m.nnz / (a.cells * a.genes), 4),
        "steps_per_chunk": res["batched"][1][:8], "same_steps": same_steps,
        "max_abs_diff_usages": diff, "loop_ms": times["loop"], "batched_ms": times["batched"],
        "loop_median_ms": lo[len(lo) // 2], "batched_median_ms": ba[len(ba) // 2],
        "loop_spread_ms": round(lo[-1] - lo[0], 3),
        "batched_spread_ms": round(ba[-1] - ba[0], 3)}), flush=True)


def spectra(a):
    dev = torch.device("cuda")
    m = matrix(a)
    csr = refit.kl_csr_of(m, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    csrT = ops.csr_transpose(csr)
    torch.cuda.synchronize()
    t_first = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    csrT = ops.csr_transpose(csr)
    torch.cuda.synchronize()
    t_tr = (time.perf_counter() - t0) * 1e3
    g = torch.Generator().manual_seed(a.k)
    UT = (torch.rand((a.k, a.cells), generator=g) + 0.05).to(dev)
    S0 = refit._init_HT(a.k, a.genes, None, dev, torch.float32, 0)
    steps = []
    for _ in range(a.rounds + 1):
        ST = S0.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.kl_sparse_refit(csrT, ST, UT, a.chunk, 8, 0.0, eps=EPS, check_every=1 << 30)
        torch.cuda.synchronize()
        steps.append(round((time.perf_counter() - t0) * 1e3 / 8, 3))
    print(json.dumps({
        "what": "spectra refit", "shape": [a.cells, a.genes], "k": a.k, "chunk": a.chunk,
        "nnz": int(m.nnz), "gather_table_bytes": int(a.cells * ops._hip.sk_k4(a.k) * 4),
        "lds_variant": bool(ops._hip.sk_lds(a.cells, a.k)),
        "transpose_ms_first": round(t_first, 3), "transpose_ms": round(t_tr, 3),
        "ms_per_mu_step_warmup": steps[0], "ms_per_mu_step": steps[1:]}), flush=True)


def consensus(a):
    from cnmf_torch_amd.api import cNMF
    from cnmf_torch_amd.utils.io import save_df_to_npz
    from cnmf_torch_amd.utils.synthetic import simulate_counts

    with tempfile.TemporaryDirectory() as tmp:
        X, cells, genes = simulate_counts(a.cells, a.genes, a.k, seed=8, sparse=False)
        fn = os.path.join(tmp, "counts.df.npz")
        save_df_to_npz(pd.DataFrame(X, index=cells, columns=genes), fn)
        obj = cNMF(output_dir=tmp, name="klrefit")
        obj.prepare(fn, components=[a.k], n_iter=a.n_iter, seed=3,
                    num_highvar_genes=min(2000, a.genes), use_gpu=True, batch_size=a.chunk,
                    beta_loss="kullback-leibler")
        obj.factorize(worker_i=0, total_workers=1, verbose=False)
        obj.combine()
        times = {"frobenius": [], "match": []}
        for r in range(a.rounds + 1):
            for loss in ("frobenius", "match"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                obj.consensus(a.k, density_threshold=2.0, show_clustering=False, refit_loss=loss)
                torch.cuda.synchronize()
                if r:                                   # round 0 warms both up
                    times[loss].append(round(time.perf_counter() - t0, 3))
        print(json.dumps({"what": "consensus wall time", "shape": [a.cells, a.genes], "k": a.k,
                          "replicates": a.n_iter, "default_s": times["frobenius"],
                          "match_s": times["match"]}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("what", choices=["usage", "spectra", "consensus"])
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--density", type=float, default=0.08)
    ap.add_argument("--chunk", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-iter", type=int, default=20)
    ap.add_argument("--tol", type=float, default=0.05, help="usage: the chunk rule's h_tol")
    ap.add_argument("--max-iter", type=int, default=200,
                    help="usage: steps per chunk at most (with --tol 0: exactly)")
    a = ap.parse_args()
    {"usage": usage, "spectra": spectra, "consensus": consensus}[a.what](a)


if __name__ == "__main__":
    main()
