"""CPU tests of partial row-wise Adam (rows w | m, one second moment per table row): the numpy model
(tests/partial_rowwise_adam_ref.py) against torch.optim.SparseAdam where the two coincide, its fp32 form against its
fp64 form, the wrong forms it must tell apart, and the refusals of the C entries and of the Python surface that can be
reached without a device."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import adam_cases as cases  # noqa: E402
import adam_ref  # noqa: E402
import partial_rowwise_adam_ref as ref  # noqa: E402
from cachedembedding_amd.functional import FusedAdam  # noqa: E402

RTOL, ATOL = 1e-5, 1e-6           # the project's Adam tolerance (tests/test_adam_cpu.py, tests/test_gpu_adam.py)
LAYOUT = "partial_rowwise_adam"


def _model_run(steps, dtype, step_fn=None, **kw):
    W = cases.initial_weight().astype(dtype)
    M, V = np.zeros_like(W), np.zeros(cases.N, dtype)
    for t, (ids, off, go, psw) in enumerate(steps, 1):
        rows, grads = ref.lookup_grads(ids, off, go.astype(dtype), cases.N, psw=psw, dtype=dtype)
        (step_fn or ref.step)(W, M, V, rows, grads, cases.LR, t, cases.BETAS, cases.EPS, dtype=dtype, **kw)
    return W, M, V


def _ratio(got, want):
    """max |got - want| / (atol + rtol |want|): above 1 fails assert_allclose"""
    want = np.asarray(want, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - want) / (ATOL + RTOL * np.abs(want))).max())


@pytest.fixture(scope="module")
def steps():
    return cases.zipf_steps()


@pytest.fixture(scope="module")
def model64(steps):
    return _model_run(steps, np.float64)


# ---- the reference against torch: where every element of a folded gradient has one magnitude, the mean of the squares
# is each square, and SparseAdam's per-element v is the row scalar in every column

def test_fp64_model_equals_sparse_adam_on_gradients_of_one_magnitude(steps):
    rng = np.random.default_rng(3)
    sigma = rng.choice([-1.0, 1.0], cases.D)
    same = []
    for ids, off, go, psw in steps:
        c = rng.uniform(0.25, 2.0, (go.shape[0], 1))                       # c_bag > 0
        same.append((ids, off, (c * sigma).astype(np.float32), psw))
    W, M, V = _model_run(same, np.float64)
    w, m, v = cases.sparse_adam_run(cases.initial_weight(), same, torch.float64)
    np.testing.assert_allclose(W, w, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(M, m, rtol=1e-12, atol=1e-12)
    for d in range(cases.D):
        np.testing.assert_allclose(V, v[:, d], rtol=1e-12, atol=1e-12)
    assert V.any() and not V[cases.NEVER] and not M[cases.NEVER].any()
    np.testing.assert_array_equal(W[cases.NEVER], cases.initial_weight()[cases.NEVER].astype(np.float64))


# ---- fp32 against fp64 on zipf_steps(): the tolerance the GPU tests use is one the fp32 reference alone keeps

def test_fp32_model_stays_within_the_tolerance_of_the_fp64_model(steps, model64):
    got = _model_run(steps, np.float32)
    for name, g, want in zip("wmv", got, model64):
        print(f"fp32 vs fp64 model, {name}: max |err| / (atol + rtol |ref|) = {_ratio(g, want):.3g}")
    for g, want in zip(got, model64):
        np.testing.assert_allclose(g.astype(np.float64), want, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("wd_mode", [None, "l2", "decoupled"])
@pytest.mark.parametrize("D", [4, 192])
def test_fp32_model_keeps_the_tolerance_on_the_kernel_tests_inputs(D, wd_mode):
    """the inputs tests/test_gpu_partial_rowwise_adam.py holds the kernels to the same tolerance on"""
    import partial_rowwise_adam_cases as kc
    for src in (False, True):
        steps = kc.kernel_steps(D, src, seed=D)
        W0 = kc.initial_weight(D, D)
        kw = dict(wd=kc.WD if wd_mode else 0.0, wd_mode=wd_mode or "l2")
        want = kc.model(W0, steps, np.float64, **kw)
        got = kc.model(W0, steps, np.float32, **kw)
        assert not want[3][kc.R - 5:].any() and want[3][kc.R - 20:kc.R - 5].any() and want[3][kc.HOT]
        for name, g, w in zip("wmv", got, want):
            print(f"D={D} src={src} wd={wd_mode} {name}: max |err| / (atol + rtol |ref|) = {_ratio(g, w):.3g}")
            np.testing.assert_allclose(g.astype(np.float64), w, rtol=RTOL, atol=ATOL)


# ---- wrong forms are told apart, each by more than ten times the tolerance on zipf_steps()

def test_per_lookup_application_is_told_apart(steps, model64):
    wrong = _model_run(steps, np.float64, step_fn=ref.step_per_lookup)
    assert _ratio(wrong[0], model64[0]) > 10 and _ratio(wrong[1], model64[1]) > 10 and _ratio(wrong[2], model64[2]) > 10
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(wrong[0], model64[0], rtol=RTOL, atol=ATOL)


def test_sum_of_squares_instead_of_the_mean_is_told_apart(steps, model64):
    wrong = _model_run(steps, np.float64, v_from="sum")
    assert _ratio(wrong[0], model64[0]) > 10 and _ratio(wrong[2], model64[2]) > 10
    np.testing.assert_allclose(wrong[2], cases.D * model64[2], rtol=1e-12)   # (v is linear in what feeds it)
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(wrong[0], model64[0], rtol=RTOL, atol=ATOL)


def test_per_element_second_moment_is_told_apart(steps, model64):
    W = cases.initial_weight().astype(np.float64)
    M, V = np.zeros_like(W), np.zeros_like(W)
    for t, (ids, off, go, psw) in enumerate(steps, 1):
        rows, grads = ref.lookup_grads(ids, off, go.astype(np.float64), cases.N, psw=psw)
        adam_ref.step(W, M, V, rows, grads, cases.LR, t, cases.BETAS, cases.EPS)
    assert _ratio(W, model64[0]) > 10
    np.testing.assert_allclose(M, model64[1], rtol=1e-12, atol=1e-15)         # m does not look at v
    np.testing.assert_allclose(V.mean(axis=1), model64[2], rtol=1e-12, atol=1e-18)
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(W, model64[0], rtol=RTOL, atol=ATOL)


def test_model_skip_rules_and_decay():
    W0 = np.arange(5 * 4, dtype=np.float64).reshape(5, 4) / 8
    go = np.asarray([[1.0, 2, 3, 4], [0.5, 0, 0, 0], [9, 9, 9, 9]])
    ids, off, psw = [1, -1, 2, 7, 3, 3], [0, 2, 4, 4], [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]
    rows, grads = ref.lookup_grads(ids, off, go, 5, psw=psw)
    assert rows.tolist() == [1, 2]                                  # -1, 7 and the uncovered tail take no part
    W, M, V = W0.copy(), np.full_like(W0, 0.25), np.full(5, 0.5)
    ref.step(W, M, V, rows, grads, 0.1, 1)
    for r in (0, 3, 4):
        np.testing.assert_array_equal(W[r], W0[r])
        assert (M[r] == 0.25).all() and V[r] == 0.5
    c1 = np.sqrt(1 - 0.999) / (1 - 0.9)
    # row 2: g = 0 -- both moments decay, the weight moves by the decayed m
    np.testing.assert_allclose(M[2], 0.225, rtol=1e-15)
    np.testing.assert_allclose(V[2], 0.4995, rtol=1e-15)
    np.testing.assert_allclose(W[2], W0[2] - 0.1 * c1 * (0.225 / (np.sqrt(0.4995) + 1e-8)), rtol=1e-14)
    # row 1: the hand-computed step, mean of squares = 30 / 4
    m1, v1 = 0.25 + 0.1 * (go[0] - 0.25), 0.5 + 0.001 * (7.5 - 0.5)
    np.testing.assert_allclose(M[1], m1, rtol=1e-14)
    np.testing.assert_allclose(V[1], v1, rtol=1e-14)
    np.testing.assert_allclose(W[1], W0[1] - 0.1 * c1 * m1 / (np.sqrt(v1) + 1e-8), rtol=1e-14)
    # decay: l2 feeds h = g + wd w to both moments; decoupled scales w by 1 - lr wd and leaves the moments alone
    for mode in ("l2", "decoupled"):
        W, M, V = W0.copy(), np.zeros_like(W0), np.zeros(5)
        ref.step(W, M, V, rows, grads, 0.1, 1, wd=0.5, wd_mode=mode)
        h = go[0] + 0.5 * W0[1] if mode == "l2" else go[0]
        np.testing.assert_allclose(M[1], 0.1 * h, rtol=1e-14)
        np.testing.assert_allclose(V[1], 0.001 * (h * h).mean(), rtol=1e-14)
        base = W0[1] if mode == "l2" else W0[1] * 0.95
        np.testing.assert_allclose(W[1], base - 0.1 * c1 * M[1] / (np.sqrt(V[1]) + 1e-8), rtol=1e-14)
    # a slot whose row lies outside the second moment is left alone, decay and all
    W, M, V = W0.copy(), np.full_like(W0, 0.25), np.full(2, 0.5)
    ref.step(W, M, V, rows, grads, 0.1, 1, wd=0.5, wd_mode="decoupled", row_of=[0, -1, 2, 1, 0])
    np.testing.assert_array_equal(W, W0)
    assert (M == 0.25).all() and (V == 0.5).all()
    ref.step(W, M, V, rows, grads, 0.1, 1, row_of=[0, 1, 2, 1, 0])   # slot 1 -> row 1; slot 2 -> row 2: outside
    assert V[1] != 0.5 and V[0] == 0.5 and (M[2] == 0.25).all() and not (M[1] == 0.25).any()


# ---- the C entries, without a GPU: everything is refused before a HIP call

def _entries():
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    return _lib, _lib.lib


def _call(lib, src, dim=8, beta1=0.9, beta2=0.999, lr=0.1, eps=1e-8, step=0x1000, acc=0, ws=0x10000, ws_bytes=1 << 30,
          weight=0x2000, nnz=5, num_rows=10, v=0x7000, v_rows=10, wd=0.0, wd_mode=0):
    """pointers are fake (aligned, never dereferenced: every call here is refused before a launch)"""
    p = ctypes.c_void_p
    tail = (p(0x8000), p(v) if v else None, v_rows, beta1, beta2, lr, None, eps, wd, wd_mode, p(step) if step else None,
            acc, p(ws), ws_bytes, None)
    if src:
        return lib.ce_bag_backward_pradam_src(p(weight), num_rows, dim, nnz, p(0x3000), 0, p(0x4000), *tail)
    return lib.ce_bag_backward_pradam(p(weight), num_rows, dim, p(0x5000), nnz, p(0x6000), 1, nnz, 1, None, 0, 0,
                                      p(0x3000), 0, None, *tail)


@pytest.mark.parametrize("src", [False, True])
def test_c_entries_refuse_before_anything_happens(src):
    _lib, lib = _entries()
    assert _call(lib, src, step=0, acc=7, beta1=1.5, dim=6) == _lib.CE_ERR_INVALID and "step" in _lib.last_error()
    assert _call(lib, src, acc=7, beta1=1.5, dim=6) == _lib.CE_ERR_INVALID and "accumulator" in _lib.last_error()
    assert _call(lib, src, wd_mode=9, beta1=1.5) == _lib.CE_ERR_INVALID and "weight_decay_mode" in _lib.last_error()
    assert _call(lib, src, wd=-1.0, wd_mode=1, beta1=1.5) == _lib.CE_ERR_INVALID and "weight_decay" in _lib.last_error()
    for b1, b2 in ((1.0, 0.999), (0.9, -1e-9), (float("nan"), 0.5)):
        assert _call(lib, src, beta1=b1, beta2=b2, dim=6) == _lib.CE_ERR_INVALID and "beta" in _lib.last_error()
    assert _call(lib, src, eps=-1e-8, dim=6) == _lib.CE_ERR_INVALID and "eps" in _lib.last_error()
    assert _call(lib, src, lr=-0.1, dim=6) == _lib.CE_ERR_INVALID and "lr" in _lib.last_error()
    for dim in (0, 2, 6, 7, 1028, 2048):
        assert _call(lib, src, dim=dim, v=0, ws_bytes=0) == _lib.CE_ERR_UNSUPPORTED, dim
        assert "dim % 4 == 0" in _lib.last_error()
    # the second moment: a null v or no rows, behind the dim rule and before the alignment and the workspace
    assert _call(lib, src, v=0, weight=0x2004, ws_bytes=0) == _lib.CE_ERR_INVALID and "v_rows" in _lib.last_error()
    for v_rows in (0, -3):
        assert _call(lib, src, v_rows=v_rows, ws_bytes=0) == _lib.CE_ERR_INVALID and "v_rows" in _lib.last_error()
    assert _call(lib, src, weight=0x2004) == _lib.CE_ERR_INVALID and "aligned" in _lib.last_error()
    for acc in (_lib.CE_ACC_CACHE, _lib.CE_ACC_STEP):
        need = lib.ce_bag_backward_pradam_workspace(10, 5, 8, acc)
        assert need > 0 and need == lib.ce_bag_backward_adam_workspace(10, 5, 8, acc)
        assert _call(lib, src, acc=acc, ws_bytes=need - 1) == _lib.CE_ERR_INVALID
        assert "workspace too small" in _lib.last_error()
    assert lib.ce_bag_backward_pradam_workspace(70, 600, 4, 2) == 0
    assert lib.ce_version() == 6


def test_forward_entries_refuse_the_dim_rule_first():
    _lib, lib = _entries()
    p = ctypes.c_void_p
    for dim in (2, 6, 1028):
        rc = lib.ce_bag_forward_pradam(p(0x2000), 10, dim, p(0x5000), 5, p(0x6000), 1, 5, 1, None, 0, 0, p(0x3000), 0, None)
        assert rc == _lib.CE_ERR_UNSUPPORTED and "dim % 4 == 0" in _lib.last_error()
        rc = lib.ce_bag_forward_src_keys_pradam(p(0x2000), 10, dim, 5, p(0x4000), p(0x3000), 0, None)
        assert rc == _lib.CE_ERR_UNSUPPORTED and "dim % 4 == 0" in _lib.last_error()
    rc = lib.ce_bag_forward_pradam(p(0x2004), 10, 8, p(0x5000), 5, p(0x6000), 1, 5, 1, None, 0, 0, p(0x3000), 0, None)
    assert rc == _lib.CE_ERR_INVALID and "aligned" in _lib.last_error()
    assert lib.ce_bag_forward_pradam(None, 10, 8, None, 5, None, 1, 5, 1, None, 0, 0, None, 0, None) == _lib.CE_ERR_INVALID


def test_host_fill_matches_the_plain_fill_row_by_row():
    _lib, lib = _entries()
    n, d = 37, 12
    plain = np.empty((n, d), np.float32)
    assert lib.ce_host_fill_uniform(plain.ctypes.data, n * d, -0.5, 0.25, 1024, 3) == 0
    for threads in (1, 5):
        t = np.full((n, 2 * d), np.nan, np.float32)
        assert lib.ce_host_fill_uniform_pradam(t.ctypes.data, n, d, -0.5, 0.25, 1024, threads) == 0
        np.testing.assert_array_equal(t[:, :d], plain)
        assert not t[:, d:].any()
    assert lib.ce_host_fill_uniform_pradam(plain.ctypes.data, 1, 6, 0.0, 1.0, 1, 1) == _lib.CE_ERR_UNSUPPORTED


# ---- the Python surface: what is refused before a device is asked for

def test_python_refusals_without_a_device():
    import cachedembedding_amd as ce
    from cachedembedding_amd.modules import FusedSparseModules
    from cachedembedding_amd.parallel import ParallelCachedEmbeddingBag
    from cachedembedding_amd.tablewise import ParallelCachedEmbeddingBagTablewise
    for dt in (torch.bfloat16, torch.float16, torch.uint8, torch.quint4x2):
        with pytest.raises(NotImplementedError, match="Adam layout is an fp32 table"):
            ce.CachedEmbeddingBag(64, 32, fused_optimizer=LAYOUT, table_dtype=dt, cuda_row_num=8)
    for kw in (dict(mode="max"), dict(max_norm=1.0), dict(sparse=True)):
        with pytest.raises(NotImplementedError, match="Adam-layout"):
            ce.CachedEmbeddingBag(64, 8, fused_optimizer=LAYOUT, cuda_row_num=8, **kw)
    with pytest.raises(NotImplementedError, match="deterministic"):
        FusedAdam(0.1, deterministic=True, layout=LAYOUT)
    for dim in (6, 2, 1028):
        with pytest.raises(NotImplementedError, match="embedding_dim % 4 == 0"):
            ce.CachedEmbeddingBag(64, dim, fused_optimizer=LAYOUT, cuda_row_num=8)
    for bad in ("adamw", "rowwise_adam", "partial_rowwise_adagrad"):
        with pytest.raises(ValueError, match="fused_optimizer"):
            ce.CachedEmbeddingBag(64, 8, fused_optimizer=bad, cuda_row_num=8)
    with pytest.raises(NotImplementedError, match="Adam-layout"):
        ParallelCachedEmbeddingBag(64, 8, fused_optimizer=LAYOUT, cuda_row_num=8)
    with pytest.raises(NotImplementedError, match="Adam-layout"):
        ParallelCachedEmbeddingBagTablewise([], 8, fused_optimizer=LAYOUT)
    with pytest.raises(NotImplementedError, match="Adam-layout"):
        FusedSparseModules([64], 8, fused_optimizer=LAYOUT, use_tablewise_parallel=True)
    with pytest.raises(ValueError, match="layout"):
        FusedAdam(0.1, layout="rowwise")
    with pytest.raises(ValueError, match="layout"):
        ce.HostTable.allocate(8, 8, layout="rowwise")
    # the object derives D from the layout's span and refuses a weight that lacks the layout, before any kernel
    f = FusedAdam(0.1, layout=LAYOUT)
    assert f.span == 2 and FusedAdam(0.1).span == 3 and FusedAdam(0.1).layout == "adam"
    with pytest.raises(NotImplementedError, match="Adam-layout rows"):
        f.check(torch.zeros(4, 9))
    with pytest.raises(NotImplementedError, match="Adam-layout rows"):
        f.check(torch.zeros(4, 16, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="embedding_dim % 4 == 0"):
        f.check(torch.zeros(4, 12))                                  # D = 6


def test_example_parses_the_flag_and_refuses_it_without_adam():
    import importlib
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "examples"))
    dm = importlib.import_module("dlrm_main")
    a = dm.parse_args(["--use_cache", "--adam", "--adam_partial_rowwise"])
    assert a.adam and a.adam_partial_rowwise and dm._fused_optimizer(a) == LAYOUT
    assert dm._fused_optimizer(dm.parse_args(["--use_cache", "--adam"])) == "adam"
    d = dm.parse_args(["--use_cache"])
    assert not d.adam_partial_rowwise and dm._fused_optimizer(d) is None
    with pytest.raises(ValueError, match="--adam_partial_rowwise"):
        dm.main(["--use_cache", "--adam_partial_rowwise"])
    with pytest.raises(ValueError, match="--adam_partial_rowwise"):
        dm.main(["--use_cache", "--adagrad", "--adam_partial_rowwise"])
    for other in ("--adagrad", "--fused_sgd"):
        with pytest.raises(ValueError, match="--adam takes the place"):
            dm.main(["--use_cache", "--adam", "--adam_partial_rowwise", other])
    with pytest.raises(NotImplementedError, match="--table_dtype fp32"):
        dm.main(["--use_cache", "--adam", "--adam_partial_rowwise", "--table_dtype", "bf16"])


# ---- load_adam_state on the level of the host table: the moment parts are written, the weights are not

@pytest.mark.parametrize("layout", ["adam", LAYOUT])
def test_host_table_moments_round_trip(layout):
    import cachedembedding_amd as ce
    from cachedembedding_amd import _lib
    n, d = 9, 8
    span = _lib.LAYOUT_SPAN[layout]
    rng = np.random.default_rng(2)
    # (HostTable.allocate needs a device for its pinned memory: the same object over plain host memory)
    t = ce.HostTable(torch.zeros(n, span * d), 0, 0, registered=False, layout=layout)
    assert t.span == span
    w = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32))
    m = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32))
    v = torch.from_numpy(rng.random((n, d)).astype(np.float32))
    t.set_weight_(w)
    assert torch.equal(t.tensor[:, :d], w) and not t.tensor[:, d:].any()
    t.set_moments_(m.double(), v if span == 3 else None)             # (another dtype is cast)
    assert torch.equal(t.tensor[:, :d], w) and torch.equal(t.tensor[:, d:2 * d], m)
    if span == 3:
        assert torch.equal(t.tensor[:, 2 * d:], v)
    # read back as a module reads them, into a second table: the same bytes
    u = ce.HostTable(torch.zeros(n, span * d), 0, 0, registered=False, layout=layout)
    u.set_weight_(t.tensor[:, :d]).set_moments_(t.tensor[:, d:2 * d], t.tensor[:, 2 * d:] if span == 3 else None)
    assert torch.equal(u.tensor, t.tensor)
    with pytest.raises(AssertionError):
        t.set_moments_(m[:, :4], v if span == 3 else None)
    with pytest.raises(AssertionError):
        t.set_moments_(m, None if span == 3 else v)
    # a module without either layout refuses before it looks at anything else
    import types
    with pytest.raises(ValueError, match="load_adam_state"):
        ce.CachedEmbeddingBag.load_adam_state(types.SimpleNamespace(fused_optimizer=None), m, v, 3)
