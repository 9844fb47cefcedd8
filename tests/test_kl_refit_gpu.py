"""KL refit on the GPU: the chunk-batched usage step of sparse_kl.hip (ops.kl_sparse_refit)
against the float64 twin, the existing sparse KL launches against arrays recorded before the
mode existed, the whole-matrix CSR transpose (csr_transpose.hip) against scipy, and the
refit layer (models.refit under beta_loss = kullback-leibler) against its CPU path."""
import functools
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.models import refit
from cnmf_torch_amd.ops import reference

gpu = pytest.mark.gpu

H_TOL = dict(rtol=1e-4, atol=1e-6)       # usages: the sparse-KL bound (test_sparse_kl_xwide_gpu)
EPS = 1e-16
N, CHUNK, TOL, MAX_ITER = 164, 48, 0.05, 200     # three full chunks and a 20-row tail
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "kl_h_block_r3_k40.npz")

# (K, G) -> seed.  LDS / L2: whether W^T (G x K4 floats) fits the 128 KB LDS stage; slices:
# the kernel bucket of the padded rank.  The seeds were picked on the CPU so that the float64
# twin keeps every stop decision >= 1e-3 (relative) away from tol (asserted in _twin).
CASES = {(5, 80): 1,        # LDS, 1 slice
         (5, 4200): 1,      # L2 gather
         (40, 80): 3,       # LDS, 4 slices
         (64, 520): 5,      # L2, 4 slices
         (80, 448): 7,      # L2, 8 slices
         (128, 80): 2}      # LDS, 8 slices
LDS = {(5, 80): True, (5, 4200): False, (40, 80): True, (64, 520): False, (80, 448): False,
       (128, 80): True}


def _ratio(got, ref, rtol, atol):
    return float(((got - ref).abs() / (rtol * ref.abs() + atol)).max())


@functools.lru_cache(maxsize=None)
def _problem(K, G):
    """float32-representable X (N x G, ~15 % non-zero, row 7 and column 3 all zero), usages
    HT (K x N) and spectra W (K x G), as float64."""
    g = torch.Generator().manual_seed(1000 * CASES[(K, G)] + K)
    X = torch.rand((N, G), generator=g, dtype=torch.float32)
    X[X < 0.85] = 0.0
    X[7] = 0.0
    X[:, 3] = 0.0
    HT = torch.rand((K, N), generator=g, dtype=torch.float32) + 0.05
    W = torch.rand((K, G), generator=g, dtype=torch.float32) + 0.05
    return X.double(), HT.double(), W.double()


def _csr64(X):
    m = sp.csr_matrix(X.numpy())
    return ops.KLCSR(torch.from_numpy(m.indptr.astype(np.int32)),
                     torch.from_numpy(m.indices.astype(np.int32)),
                     torch.from_numpy(m.data), *m.shape)


@functools.lru_cache(maxsize=None)
def _twin(K, G):
    """The float64 twin on the case -> (usages, per-chunk steps, trace).  Asserts the
    condition the comparison rests on: no step's change is within 1e-3 (relative) of tol."""
    X, HT, W = _problem(K, G)
    h = HT.clone()
    it = torch.zeros(4, dtype=torch.int32)
    trace = []
    reference.kl_refit(_csr64(X), h, W, CHUNK, MAX_ITER, TOL, eps=EPS, iters=it, trace=trace)
    margin = min(abs(r - TOL) / TOL for _, _, r in trace)
    assert margin >= 1e-3, (K, G, margin)
    return h, it, trace, margin


def _gpu_refit(K, G, max_iter=MAX_ITER):
    X, HT, W = _problem(K, G)
    dev = torch.device("cuda")
    csr = ops.kl_csr(X.float().to(dev))
    h = HT.float().to(dev)
    it = torch.zeros(4, dtype=torch.int32, device=dev)
    ops.kl_sparse_refit(csr, h, W.float().to(dev), CHUNK, max_iter, TOL, eps=EPS, iters=it)
    return h.cpu(), it.cpu()


def test_twin_condition_holds_on_every_case():
    """No GPU: the float64 twin's stop decisions keep their distance from tol on all six
    cases, and every chunk takes more than one step and stops before max_iter."""
    for K, G in CASES:
        _, it, _, margin = _twin(K, G)
        print(K, G, "steps", it.tolist(), "margin", margin)
        assert (it > 1).all() and (it < MAX_ITER).all()
        assert bool(ops.kl_refit_chunks(N, CHUNK) == (48, 3, 20))


@gpu
@pytest.mark.parametrize("K,G", list(CASES))
def test_chunk_batched_step_matches_fp64_twin(K, G):
    """ops.kl_sparse_refit (three full chunks in one launch per step, the tail in a second)
    vs the float64 twin: the step count of every chunk, the usages within the sparse KL
    bound, and a finished chunk is not touched by later launches: its usages are bit for bit
    those of a run that makes only as many launches as the chunk took steps."""
    assert bool(ops._hip.sk_lds(G, K)) == LDS[(K, G)]
    ref, it_ref, _, _ = _twin(K, G)
    h, it = _gpu_refit(K, G)
    print("steps", it.tolist(), "usages: x tolerance", _ratio(h.double(), ref, **H_TOL))
    assert it.tolist() == it_ref.tolist()
    torch.testing.assert_close(h.double(), ref, **H_TOL)
    assert bool((h[:, 7] == 0).all())                  # the empty row's usages
    for s in sorted(set(it.tolist())):
        hs, its = _gpu_refit(K, G, max_iter=s)
        for r in [r for r in range(4) if it[r] == s]:
            a, b = r * CHUNK, min(N, (r + 1) * CHUNK)
            assert its[r] == s
            assert torch.equal(hs[:, a:b], h[:, a:b]), (r, s)


def _golden_inputs():
    """Integer-formula inputs (the same on every host): R = 3, K = 40, a 24-row chunk of a
    60 x 48 matrix (~14 % non-zero)."""
    i, j = np.meshgrid(np.arange(60), np.arange(48), indexing="ij")
    X = np.where((i * 31 + j * 17) % 7 == 0, (i + 2 * j) % 5 + 1, 0).astype(np.float32)
    r, k, c = np.meshgrid(np.arange(3), np.arange(40), np.arange(60), indexing="ij")
    HT = (0.05 + ((r * 7 + k * 3 + c * 5) % 11) / 11.0).astype(np.float32)
    r, k, g = np.meshgrid(np.arange(3), np.arange(40), np.arange(48), indexing="ij")
    W = (0.05 + ((r * 5 + k * 11 + g * 3) % 13) / 13.0).astype(np.float32)
    return X, HT, W


def golden_h_block():
    """One kl_sparse_h_block call with the block-objective rule on rows [10, 34)."""
    X, HT, W = _golden_inputs()
    dev = torch.device("cuda")
    csr = ops.kl_csr(torch.from_numpy(X).to(dev))
    h = torch.from_numpy(HT).to(dev)[:, :, 10:34].contiguous()
    act = torch.ones(3, dtype=torch.int32, device=dev)
    it = torch.zeros(3, dtype=torch.int32, device=dev)
    hs = torch.zeros((3, 2), dtype=torch.float64, device=dev)
    ops.kl_sparse_h_block(ops.kl_csr_rows(csr, 10, 34), h, torch.from_numpy(W).to(dev), 1e-10, 3,
                          0.01, 0.0, act=act, tol=0.05, iters=it, hstate=hs, loss_entry=True)
    return dict(HT=h.cpu().numpy(), act=act.cpu().numpy(), iters=it.cpu().numpy(),
                hstate=hs.cpu().numpy())


@gpu
def test_existing_h_block_launch_is_bitwise_the_recorded_one():
    """The replicate-batched launch (chunk mode off: the XCD-pinned block map, row offset 0)
    gives bit for bit the usages, flags and step counts recorded from the same call before
    the chunk-batched mode was added (tests/golden/kl_h_block_r3_k40.npz)."""
    want = np.load(GOLDEN)
    got = golden_h_block()
    assert got["HT"].shape == (3, 40, 24)
    for key in ("HT", "act", "iters"):
        assert got[key].dtype == want[key].dtype
        assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), key


def _sparse(n, g, density, seed, dead=False):
    rng = np.random.default_rng(seed)
    X = rng.integers(1, 10, size=(n, g)).astype(np.float32)
    X[rng.random((n, g)) >= density] = 0.0
    if dead:
        X[::7] = 0.0
        X[:, 2] = 0.0
        X[:, g - 1] = 0.0
    return sp.csr_matrix(X)


TRANSPOSE_CASES = {"three_tiles_ragged": (20000, 37, 0.08, False), "small": (100, 5, 0.5, False),
                   "empty": (50, 9, 0.0, False), "empty_rows_cols": (300, 41, 0.2, True)}


@gpu
@pytest.mark.parametrize("name", list(TRANSPOSE_CASES))
def test_csr_transpose_is_bitwise_scipys(name):
    n, g, density, dead = TRANSPOSE_CASES[name]
    m = _sparse(n, g, density, seed=n, dead=dead)
    ref = m.T.tocsr()
    ref.sort_indices()
    dev = torch.device("cuda")
    csr = refit.kl_csr_of(m, dev)
    outs = [ops.csr_transpose(csr) for _ in range(2)]
    for t in outs:
        assert (t.n_rows, t.n_cols) == (g, n)
        assert t.rowptr.dtype == torch.int32 and t.col.dtype == torch.int32
        assert np.array_equal(t.rowptr.cpu().numpy(), ref.indptr)
        assert np.array_equal(t.col.cpu().numpy()[:m.nnz], ref.indices)
        assert np.array_equal(t.val.cpu().numpy()[:m.nnz].view(np.uint32),
                              ref.data.view(np.uint32))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][:3], outs[1][:3]))
    if name == "three_tiles_ragged":
        assert -(-n // int(ops._hip.csr_transpose_max_tile())) == 3
        # a row range of the CSR (rowptr slice with a non-zero first offset)
        sub = ops.csr_transpose(ops.kl_csr_rows(csr, 9000, 17500))
        rs = m[9000:17500].T.tocsr()
        rs.sort_indices()
        assert np.array_equal(sub.rowptr.cpu().numpy(), rs.indptr)
        assert np.array_equal(sub.col.cpu().numpy()[:rs.nnz], rs.indices)
        assert np.array_equal(sub.val.cpu().numpy()[:rs.nnz], rs.data)


@gpu
def test_csr_transpose_rejects_2g_entries_without_a_launch():
    dev = torch.device("cuda")
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    big = ops.KLCSR(torch.tensor([0, 2 ** 31], dtype=torch.int64, device=dev), one,
                    one.float(), 1, 5)
    with pytest.raises(ValueError, match="int32"):
        ops.csr_transpose(big)


E_N, E_G, E_K, E_CHUNK = 300, 90, 7, 128      # two full chunks and a 44-row tail


@functools.lru_cache(maxsize=None)
def _e2e():
    m = _sparse(E_N, 140, 0.15, seed=11)
    rng = np.random.default_rng(12)
    W = (rng.random((E_K, E_G)) + 0.05).astype(np.float32)
    U = (rng.random((E_N, E_K)) + 0.05).astype(np.float32)
    cmap = np.full(140, -1, np.int32)
    cmap[rng.permutation(140)[:E_G]] = np.arange(E_G, dtype=np.int32)
    div = torch.from_numpy(rng.random(E_G) + 0.5)
    return m, W, U, cmap, div


def _forms(dev):
    """X (300 x 90) as a dense tensor, a DeviceCSR and a scaled column-mapped DeviceCSR view
    (90 of 140 stored columns, each divided by its own factor), all on ``dev``."""
    m, _, _, cmap, div = _e2e()
    keep = np.flatnonzero(cmap >= 0)
    order = keep[np.argsort(cmap[keep])]
    plain = sp.csr_matrix(m[:, order])
    big = ops.sparse.DeviceCSR.from_scipy(m, device=dev)
    return {"dense": torch.from_numpy(plain.toarray()).to(dev),
            "device_csr": ops.sparse.DeviceCSR.from_scipy(plain, device=dev),
            "view": big.view(col_map=cmap, col_div=div, n_out=E_G)}


@functools.lru_cache(maxsize=None)
def _e2e_cpu(form):
    _, W, U, _, _ = _e2e()
    X = _forms("cpu")[form]
    it_h, it_s = torch.zeros(3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    H = refit.fit_H_online(X, W, chunk_size=E_CHUNK, beta_loss=1, random_state=2, iters=it_h)
    S = refit.fit_spectra_online(X, U, chunk_size=E_CHUNK, beta_loss=1, random_state=2,
                                 iters=it_s)
    return H, S, it_h, it_s


@gpu
@pytest.mark.parametrize("form", ["dense", "device_csr", "view"])
def test_refit_layer_on_gpu_matches_cpu_path(form):
    _, W, U, _, _ = _e2e()
    Hc, Sc, ihc, isc = _e2e_cpu(form)
    X = _forms("cuda")[form]
    ih = torch.zeros(3, dtype=torch.int32, device="cuda")
    is_ = torch.zeros(1, dtype=torch.int32, device="cuda")
    H = refit.fit_H_online(X, W, chunk_size=E_CHUNK, beta_loss=1, random_state=2, device="cuda",
                           iters=ih)
    S = refit.fit_spectra_online(X, U, chunk_size=E_CHUNK, beta_loss=1, random_state=2,
                                 device="cuda", iters=is_)
    print("steps", ih.tolist(), is_.tolist(), "usages: x tolerance",
          _ratio(torch.from_numpy(H), torch.from_numpy(Hc), **H_TOL), "spectra: x tolerance",
          _ratio(torch.from_numpy(S), torch.from_numpy(Sc), **H_TOL))
    assert ih.cpu().tolist() == ihc.tolist() and is_.cpu().tolist() == isc.tolist()
    np.testing.assert_allclose(H, Hc, **H_TOL)
    np.testing.assert_allclose(S, Sc, **H_TOL)


@gpu
def test_rank_above_128_takes_the_eager_route_and_warns_once():
    from cnmf_torch_amd.models import nmf_base

    m = _sparse(120, 60, 0.2, seed=5)
    W = (np.random.default_rng(6).random((130, 60)) + 0.05).astype(np.float32)
    Hc = refit.fit_H_online(m, W, chunk_size=50, beta_loss=1)
    for msg in [w for w in nmf_base._WARNED if "KL refit K=130" in w]:
        nmf_base._WARNED.discard(msg)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        H1 = refit.fit_H_online(m, W, chunk_size=50, beta_loss=1, device="cuda")
        H2 = refit.fit_H_online(m, W, chunk_size=50, beta_loss=1, device="cuda")
    assert len([w for w in rec if "KL refit K=130" in str(w.message)]) == 1
    np.testing.assert_allclose(H1, Hc, **H_TOL)
    np.testing.assert_allclose(H2, Hc, **H_TOL)
