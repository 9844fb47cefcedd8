"""The HIP kernels of csrc/kernels/pca_csr.hip (csr_gram, csr_project) and the sparse PCA
built on them, at the smallest shapes where they can go wrong, against the numpy float64
oracle of pca_csr_cases.py (test_pca_csr_cpu.py runs the same checks through the torch
paths).  Every check first asserts ``ops.use_native`` on its GPU input.

Edges reached (kernel constant -> case id):
  csr_gram     kGrTile = 64: gram-nh{1,63,64,65} (one tile, both tile edges), gram-nh{130,200}
               (three / four tiles, a ragged last one, tile pairs I < J); 4 waves, their 64-row
               chunks and kGrMinRows = 256 rows per slab: gram-n{1,3,4,5,63,64,65,255,256,257,
               515} (257 rows: two slabs; 515: three, the last one short); second and third
               chunks of a wave, 32 tiles: gram-wide; pairs per row 64 / 65 / 4096 (one, two
               and 64 lane steps), a row stored only in dropped columns, empty rows:
               gram-pairs; every pair of a row: gram-full; each transform factor, float32 /
               float64 data and values, a permuting col_map with dropped columns: xform-*,
               rows-n130.
  csr_project  64 components per launch: c in {1,50,64,65,130}; the ROW_LENS row lengths
               (the 64-entry trips and their tails): rows-n{1,3,4,5,130}.
"""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import csr_cases as cc
import pca_csr_cases as pc
from cnmf_torch_amd import Preprocess
from cnmf_torch_amd.models import pp
from cnmf_torch_amd.ops import sparse as sops
from cnmf_torch_amd.utils.anndata_lite import AnnData
from cnmf_torch_amd.utils.synthetic import simulate_counts

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_slab_count_is_a_function_of_the_shape():
    R = int(sops._hip.csr_gram_min_rows())
    assert R == pc.MIN_ROWS
    slabs = sops._hip.csr_gram_slabs
    assert [slabs(n, 130) for n in (1, R - 1, R, R + 1, 2 * R + 3)] == [1, 1, 1, 2, 3]
    # about 512 workgroups while the rows allow, which also bounds the slab partials
    assert slabs(10 ** 6, 130) == 86 and slabs(500000, 2000) == 1 and slabs(10 ** 6, 64) == 512
    for nh in (64, 128, 130, 512, 2000, 5000):
        assert slabs(10 ** 6, nh) * nh * nh * 8 <= (32 << 20) + nh * nh * 8


@pytest.mark.parametrize("case", pc.exact_cases(), ids=lambda c: c.name)
def test_gram_small_integers_exact(case):
    pc.check_gram(case, DEV, exact=True)


@pytest.mark.parametrize("vd", ["float32", "float64"])
@pytest.mark.parametrize("in_dtype", ["float32", "float64"])
@pytest.mark.parametrize("col_map", ["nomap", "perm"])
@pytest.mark.parametrize("factor", pc.FACTORS)
def test_gram_transform_factors(factor, col_map, in_dtype, vd):
    pc.check_gram(cc.factor_case(factor, col_map, in_dtype), DEV, vd)


@pytest.mark.parametrize("vd", ["float32", "float64"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_gram_every_factor_permuting_map(dtype, vd):
    pc.check_gram(cc.rows_case(130, dtype, "perm"), DEV, vd)


@pytest.mark.parametrize("vd", ["float32", "float64"])
@pytest.mark.parametrize("shift", [False, True], ids=["noshift", "shift"])
@pytest.mark.parametrize("c", pc.C_LIST)
def test_project(c, shift, vd):
    pc.check_project(cc.rows_case(130), DEV, c, vd, shift)


def test_project_short_rows():
    for n in (1, 3, 4, 5):
        pc.check_project(cc.rows_case(n), DEV, 7, shift=True)


def test_empty_inputs_are_exact_zeros():
    for which in ("norows", "nonnz"):
        case = cc.empty_case(which)
        A = case.csr(DEV)
        # freed, non-zero device memory of the results' sizes: unwritten output cannot read
        # as zeros by luck
        for shape in ((1, 30, 30), (case.n, 5)):
            torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
        G = sops.gram(A)
        assert tuple(G.shape) == (30, 30) and G.dtype == torch.float64 and not G.any()
        out = sops.project(A, torch.ones((30, 5), dtype=torch.float64, device=DEV))
        assert tuple(out.shape) == (case.n, 5) and not out.any()


def test_non_injective_col_map_raises():
    A = cc.rows_case(5).csr(DEV)
    cm = np.arange(600, dtype=np.int32) % 300
    with pytest.raises(ValueError):
        sops.gram(A.view(col_map=cm, n_out=300))


@pytest.mark.parametrize("vd", ["float32", "float64"])
@pytest.mark.parametrize("i", [0, 1])
def test_pca_csr_matches_cpu_oracle(i, vd):
    pc.check_pca_csr(i, vd, DEV)


def test_pipeline_csr_backend_matches_dense():
    Xc, cells, genes = simulate_counts(3000, 400, 4, seed=3, sparse=True)
    rs = np.random.default_rng(0)
    obs = pd.DataFrame({"batch": pd.Categorical(rs.choice(["x", "y", "z"], 3000))}, index=cells)
    ad = AnnData(X=sp.csr_matrix(Xc, dtype=np.float32), obs=obs, var=pd.DataFrame(index=genes))
    p = Preprocess(random_seed=0)
    kw = dict(harmony_vars=["batch"], n_top_genes=100, makeplots=False, max_iter_harmony=3,
              device="cuda")
    d_out, d_hv = p.normalize_batchcorrect(ad.copy(), pca_backend="dense", **kw)
    p.harmony_info_ = None
    c_out, c_hv = p.normalize_batchcorrect(ad.copy(), pca_backend="csr", **kw)
    assert c_hv == d_hv
    np.testing.assert_allclose(c_out.obsm["X_pca"], d_out.obsm["X_pca"], rtol=1e-4, atol=1e-4)
    assert c_out.X.shape == (3000, 100) and c_out.X.dtype == np.float32
    assert np.isfinite(c_out.X).all() and (c_out.X >= 0).all()
    assert p.harmony_info_ is not None


def test_pca_csr_peak_memory_below_one_dense_copy():
    """20,000 x 512 at about 7 % non-zero: everything pca_csr allocates, the uploaded CSR
    included, stays below one dense float64 copy of the matrix (a condition, not a tuned
    number: packed entries, pointers and slab partials are a fraction of it)."""
    n, g, nh = 20000, 640, 512
    rs = np.random.default_rng(11)
    X = sp.random(n, g, density=0.07, format="csr", dtype=np.float32, random_state=rs)
    X.data[:] = rs.integers(1, 10, X.nnz)
    cm = np.full(g, -1, np.int32)
    cm[rs.permutation(g)[:nh]] = np.arange(nh)
    lib = 1e4 / np.maximum(np.asarray(X.sum(1)).reshape(-1), 1.0)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    A = sops.DeviceCSR.from_scipy(X, device=DEV)
    V = A.view(col_map=cm, n_out=nh, row_scale=lib, round_mid=True,
               col_div=rs.random(nh) + 0.5)
    xs, vh, var, ratio = pp.pca_csr(V, 50, value_dtype=torch.float32)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"pca_csr peak {peak / 1e6:.1f} MB, one dense float64 copy {n * nh * 8 / 1e6:.1f} MB")
    assert xs.shape == (n, 50) and np.isfinite(xs).all()
    assert peak < n * nh * 8
