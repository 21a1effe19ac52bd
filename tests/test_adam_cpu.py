"""CPU tests of the fused Adam of an Adam-layout table: the numpy model (tests/adam_ref.py) against
torch.optim.SparseAdam, the model's skip rules, and the refusals of the C entries and of the Python surface that can be
reached without a device."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import adam_cases as cases  # noqa: E402
import adam_ref as ref  # noqa: E402
from cachedembedding_amd.functional import FusedAdam  # noqa: E402  (the feature: without it nothing here has a subject)

RTOL, ATOL = 1e-5, 1e-6           # the GPU tests' tolerance: the project's own from test_gpu_rowwise_adagrad.py


def _model_run(steps, dtype, W0=None, use_psw=True, lr=cases.LR):
    W = (cases.initial_weight() if W0 is None else W0).astype(dtype)
    M, V = np.zeros_like(W), np.zeros_like(W)
    for t, (ids, off, go, psw) in enumerate(steps, 1):
        rows, grads = ref.lookup_grads(ids, off, go.astype(dtype), cases.N, psw=psw if use_psw else None, dtype=dtype)
        ref.step(W, M, V, rows, grads, lr, t, cases.BETAS, cases.EPS, dtype=dtype)
    return W, M, V


@pytest.fixture(scope="module")
def steps():
    return cases.zipf_steps()


@pytest.fixture(scope="module")
def model64(steps):
    return _model_run(steps, np.float64)


def test_workload_is_what_the_issue_asks_for(steps):
    assert len(steps) == 12 and cases.N == 64 and cases.D == 8
    ids = np.concatenate([s[0] for s in steps])
    assert cases.NEVER not in ids
    assert max(np.bincount(s[0]).max() for s in steps) >= 10                  # heavy duplicates
    assert len({tuple(np.diff(s[1])) for s in steps}) == 12 and any(len(set(np.diff(s[1]))) > 3 for s in steps)   # ragged


def test_fp64_model_equals_sparse_adam(steps, model64):
    w, m, v = cases.sparse_adam_run(cases.initial_weight(), steps, torch.float64)
    for got, want in zip(model64, (w, m, v)):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    # the row nobody looks up: the initial weight, zero moments
    np.testing.assert_array_equal(model64[0][cases.NEVER], cases.initial_weight()[cases.NEVER].astype(np.float64))
    assert not model64[1][cases.NEVER].any() and not model64[2][cases.NEVER].any()


def test_torch_fp32_stays_within_the_gpu_tolerance_of_the_fp64_model(steps, model64):
    got = cases.sparse_adam_run(cases.initial_weight(), steps, torch.float32)
    for name, g, want in zip("wmv", got, model64):
        err = np.abs(g - want)
        print(f"torch fp32 vs fp64 model, {name}: max abs error {err.max():.3g}")
        np.testing.assert_allclose(g, want, rtol=RTOL, atol=ATOL)


def test_fp32_model_stays_within_the_tolerance_too(steps, model64):
    for g, want in zip(_model_run(steps, np.float32), model64):
        np.testing.assert_allclose(g.astype(np.float64), want, rtol=RTOL, atol=ATOL)


def test_model_skip_rules():
    W0 = np.arange(5 * 4, dtype=np.float64).reshape(5, 4)
    go = np.asarray([[1.0, 2, 3, 4], [0.5, 0, 0, 0], [9, 9, 9, 9]])
    # lookups: row 1 (bag 0), slot -1 (bag 0), row 2 with weight zero (bag 1), row 7 out of range (bag 1), and a tail of
    # two lookups of row 3 behind offsets[-1] that no bag covers (bag 2 is empty)
    ids = [1, -1, 2, 7, 3, 3]
    off = [0, 2, 4, 4]
    psw = [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]
    rows, grads = ref.lookup_grads(ids, off, go, 5, psw=psw)
    assert rows.tolist() == [1, 2]                                  # -1, 7 and the uncovered tail take no part
    W, M, V = W0.copy(), np.full_like(W0, 0.25), np.full_like(W0, 0.5)
    ref.step(W, M, V, rows, grads, 0.1, 1)
    for r in (0, 3, 4):                                             # not named: bit for bit
        np.testing.assert_array_equal(W[r], W0[r])
        assert (M[r] == 0.25).all() and (V[r] == 0.5).all()
    # row 2: g = 0 -- the moments decay and the weight still moves by the decayed m
    np.testing.assert_allclose(M[2], 0.25 * 0.9, rtol=1e-15)
    np.testing.assert_allclose(V[2], 0.5 * 0.999, rtol=1e-15)
    c1 = np.sqrt(1 - 0.999) / (1 - 0.9)
    np.testing.assert_allclose(W[2], W0[2] - 0.1 * c1 * (0.225 / (np.sqrt(0.4995) + 1e-8)), rtol=1e-14)
    # row 1: the hand-computed step
    m1 = 0.25 + 0.1 * (go[0] - 0.25)
    v1 = 0.5 + 0.001 * (go[0] ** 2 - 0.5)
    np.testing.assert_allclose(M[1], m1, rtol=1e-14)
    np.testing.assert_allclose(V[1], v1, rtol=1e-14)
    np.testing.assert_allclose(W[1], W0[1] - 0.1 * c1 * m1 / (np.sqrt(v1) + 1e-8), rtol=1e-14)


def test_per_lookup_application_is_a_different_wrong_answer():
    W0 = np.zeros((2, 4))
    rows, grads = ref.lookup_grads([0, 0, 0], [0, 1, 2, 3], np.ones((3, 4)), 2)
    a = [W0.copy(), np.zeros_like(W0), np.zeros_like(W0)]
    b = [W0.copy(), np.zeros_like(W0), np.zeros_like(W0)]
    ref.step(*a, rows, grads, 0.1, 1)
    ref.step_per_lookup(*b, rows, grads, 0.1, 1)
    np.testing.assert_allclose(a[1][0], 0.1 * 3)                     # one update with g = 3
    np.testing.assert_allclose(b[1][0], 0.1 + 0.09 + 0.081)          # three updates with g = 1
    assert np.abs(a[0][0] - b[0][0]).min() > 0.05 and not np.allclose(a[2], b[2])


# ---- the C entries, without a GPU: everything is refused before a HIP call

def _entries():
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    return _lib, _lib.lib


def _call(lib, src, dim=8, beta1=0.9, beta2=0.999, lr=0.1, eps=1e-8, step=0x1000, acc=0, ws=0x10000, ws_bytes=1 << 30,
          weight=0x2000, nnz=5, num_rows=10):
    """pointers are fake (aligned, never dereferenced: every call here is refused before a launch)"""
    p = ctypes.c_void_p
    tail = (beta1, beta2, lr, None, eps, p(step) if step else None, acc, p(ws), ws_bytes, None)
    if src:
        return lib.ce_bag_backward_adam_src(p(weight), num_rows, dim, nnz, p(0x3000), 0, p(0x4000), *tail)
    return lib.ce_bag_backward_adam(p(weight), num_rows, dim, p(0x5000), nnz, p(0x6000), 1, nnz, 1, None, 0, 0, p(0x3000), 0,
                                    None, *tail)


@pytest.mark.parametrize("src", [False, True])
def test_c_entries_refuse_before_anything_happens(src):
    _lib, lib = _entries()
    # null step comes first: before a bad accumulator, bad betas and a bad dim in the same call
    assert _call(lib, src, step=0, acc=7, beta1=1.5, dim=6) == _lib.CE_ERR_INVALID
    assert "step" in _lib.last_error()
    assert _call(lib, src, acc=7, beta1=1.5, dim=6) == _lib.CE_ERR_INVALID and "accumulator" in _lib.last_error()
    for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, -1e-9), (float("nan"), 0.5)):
        assert _call(lib, src, beta1=b1, beta2=b2, dim=6) == _lib.CE_ERR_INVALID and "beta" in _lib.last_error()
    assert _call(lib, src, eps=-1e-8, dim=6) == _lib.CE_ERR_INVALID and "eps" in _lib.last_error()
    assert _call(lib, src, lr=-0.1, dim=6) == _lib.CE_ERR_INVALID and "lr" in _lib.last_error()
    for dim in (0, 2, 6, 7, 1028, 2048):
        assert _call(lib, src, dim=dim, ws_bytes=0) == _lib.CE_ERR_UNSUPPORTED, dim
        assert "dim % 4 == 0" in _lib.last_error()
    assert _call(lib, src, weight=0x2004) == _lib.CE_ERR_INVALID and "aligned" in _lib.last_error()
    for acc in (_lib.CE_ACC_CACHE, _lib.CE_ACC_STEP):
        need = lib.ce_bag_backward_adam_workspace(10, 5, 8, acc)
        assert need > 0
        assert _call(lib, src, acc=acc, ws_bytes=need - 1) == _lib.CE_ERR_INVALID
        assert "workspace too small" in _lib.last_error()
    # beta = 0 and eps = 0 are legal: the call gets as far as the workspace
    assert _call(lib, src, beta1=0.0, beta2=0.0, eps=0.0, ws_bytes=0) == _lib.CE_ERR_INVALID
    assert "workspace too small" in _lib.last_error()


def test_workspace_is_the_covered_entries_workspace():
    _lib, lib = _entries()
    for R, n, d in ((70, 600, 4), (4100, 33, 128), (8, 40, 1024)):
        assert lib.ce_bag_backward_adam_workspace(R, n, d, _lib.CE_ACC_CACHE) == \
            lib.ce_bag_backward_rowwise_adagrad_workspace(R, d)
        assert lib.ce_bag_backward_adam_workspace(R, n, d, _lib.CE_ACC_STEP) == \
            lib.ce_bag_backward_update_compact_workspace(R, n, d)
    assert lib.ce_bag_backward_adam_workspace(70, 600, 4, 2) == 0


def test_forward_entries_refuse_the_dim_rule_first():
    _lib, lib = _entries()
    p = ctypes.c_void_p
    for dim in (2, 6, 1028):
        rc = lib.ce_bag_forward_adam(p(0x2000), 10, dim, p(0x5000), 5, p(0x6000), 1, 5, 1, None, 0, 0, p(0x3000), 0, None)
        assert rc == _lib.CE_ERR_UNSUPPORTED and "Adam-layout" in _lib.last_error()
        rc = lib.ce_bag_forward_src_keys_adam(p(0x2000), 10, dim, 5, p(0x4000), p(0x3000), 0, None)
        assert rc == _lib.CE_ERR_UNSUPPORTED and "Adam-layout" in _lib.last_error()
    rc = lib.ce_bag_forward_adam(p(0x2004), 10, 8, p(0x5000), 5, p(0x6000), 1, 5, 1, None, 0, 0, p(0x3000), 0, None)
    assert rc == _lib.CE_ERR_INVALID and "aligned" in _lib.last_error()
    assert lib.ce_bag_forward_adam(None, 10, 8, None, 5, None, 1, 5, 1, None, 0, 0, None, 0, None) == _lib.CE_ERR_INVALID


def test_host_fill_matches_the_plain_fill_row_by_row():
    _lib, lib = _entries()
    n, d = 37, 12
    plain = np.empty((n, d), np.float32)
    assert lib.ce_host_fill_uniform(plain.ctypes.data, n * d, -0.5, 0.25, 1024, 3) == 0
    for threads in (1, 5):
        t = np.full((n, 3 * d), np.nan, np.float32)
        assert lib.ce_host_fill_uniform_adam(t.ctypes.data, n, d, -0.5, 0.25, 1024, threads) == 0
        np.testing.assert_array_equal(t[:, :d], plain)
        assert not t[:, d:].any()
    assert lib.ce_host_fill_uniform_adam(plain.ctypes.data, 1, 6, 0.0, 1.0, 1, 1) == _lib.CE_ERR_UNSUPPORTED


# ---- the Python surface: what is refused before a device is asked for

def test_python_refusals_without_a_device():
    import cachedembedding_amd as ce
    from cachedembedding_amd.tablewise import ParallelCachedEmbeddingBagTablewise
    from cachedembedding_amd.parallel import ParallelCachedEmbeddingBag
    for dt in (torch.bfloat16, torch.float16, torch.uint8, torch.quint4x2):
        with pytest.raises(NotImplementedError, match="Adam layout is an fp32 table"):
            ce.CachedEmbeddingBag(64, 32, fused_optimizer="adam", table_dtype=dt, cuda_row_num=8)
    for kw in (dict(mode="max"), dict(max_norm=1.0), dict(sparse=True)):
        with pytest.raises(NotImplementedError, match="Adam-layout"):
            ce.CachedEmbeddingBag(64, 8, fused_optimizer="adam", cuda_row_num=8, **kw)
    with pytest.raises(NotImplementedError, match="deterministic"):
        FusedAdam(0.1, deterministic=True)
    for dim in (6, 2, 1028):
        with pytest.raises(NotImplementedError, match="embedding_dim % 4 == 0"):
            ce.CachedEmbeddingBag(64, dim, fused_optimizer="adam", cuda_row_num=8)
    with pytest.raises(ValueError, match="fused_optimizer"):
        ce.CachedEmbeddingBag(64, 8, fused_optimizer="adamw", cuda_row_num=8)
    with pytest.raises(NotImplementedError, match="Adam-layout"):
        ParallelCachedEmbeddingBag(64, 8, fused_optimizer="adam", cuda_row_num=8)
    with pytest.raises(NotImplementedError, match="Adam-layout"):
        ParallelCachedEmbeddingBagTablewise([], 8, fused_optimizer="adam")
    for bad in (dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(eps=-1.0), dict(accumulator="row")):
        with pytest.raises(ValueError):
            FusedAdam(0.1, **bad)
    with pytest.raises(TypeError):
        FusedAdam(torch.zeros(1, dtype=torch.float64))              # check_lr: a tensor rate is one fp32 element
    # the object refuses a weight that has not the layout, before any kernel
    f = FusedAdam(0.1)
    with pytest.raises(NotImplementedError, match="Adam-layout rows"):
        f.check(torch.zeros(4, 8))
    with pytest.raises(NotImplementedError, match="Adam-layout rows"):
        f.check(torch.zeros(4, 24, dtype=torch.bfloat16))


def test_example_parses_adam_and_refuses_what_it_must(monkeypatch):
    import importlib
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "examples"))
    dm = importlib.import_module("dlrm_main")
    a = dm.parse_args(["--use_cache", "--adam", "--adam_beta1", "0.8", "--adam_beta2", "0.99", "--eps", "1e-6"])
    assert a.adam and (a.adam_beta1, a.adam_beta2, a.eps) == (0.8, 0.99, 1e-6)
    d = dm.parse_args(["--use_cache"])
    assert not d.adam and (d.adam_beta1, d.adam_beta2, d.eps) == (0.9, 0.999, 1e-8)
    for other in ("--adagrad", "--fused_sgd"):
        with pytest.raises(ValueError, match="--adam takes the place"):
            dm.main(["--use_cache", "--adam", other])
    with pytest.raises(NotImplementedError, match="--adam is implemented for one process"):
        dm.main(["--use_cache", "--adam", "--use_tablewise"])
    with pytest.raises(NotImplementedError, match="--table_dtype fp32"):
        dm.main(["--use_cache", "--adam", "--table_dtype", "bf16"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="--adam is implemented for one process"):
        dm.main(["--use_cache", "--adam"])
