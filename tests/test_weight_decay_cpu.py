"""Weight decay of the fused updates without a GPU: the numpy model (tests/weight_decay_ref.py) against
torch's optimizers on the CPU, the lazy rule, the evidence for the GPU test's tolerance on the GPU test's own workload,
the refusals of the five ce_*_wd entries and of the Python surface, and the example's two flags."""
import ctypes
import importlib
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import adam_ref  # noqa: E402
import rowwise_adagrad_ref as adagrad_ref  # noqa: E402
import weight_decay_ref as ref  # noqa: E402

RTOL, ATOL = 1e-5, 1e-6                       # the GPU test's (test_gpu_weight_decay.py)


# ---- weight_decay = 0 is the existing references, exactly ------------------------------------------------------------

@pytest.mark.parametrize("mode", ref.MODES)
def test_zero_decay_reproduces_the_existing_references(mode):
    rng = np.random.default_rng(0)
    R, D = 12, 5
    W0 = rng.standard_normal((R, D))
    rows = rng.integers(0, R - 2, 30)
    grads = rng.standard_normal((30, D))
    for dt in (np.float64, np.float32):
        a, am = W0.astype(dt), np.zeros(R, dt)
        b, bm = W0.astype(dt), np.zeros(R, dt)
        for _ in range(3):
            adagrad_ref.step(a, am, rows, grads.astype(dt), 0.1, 1e-8, dt)
            ref.step_adagrad(b, bm, rows, grads.astype(dt), 0.1, 1e-8, 0.0, mode, dt)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(am, bm)
        a = [W0.astype(dt), np.zeros((R, D), dt), np.zeros((R, D), dt)]
        b = [W0.astype(dt), np.zeros((R, D), dt), np.zeros((R, D), dt)]
        for t in (1, 2, 3):
            adam_ref.step(*a, rows, grads.astype(dt), 0.1, t, dtype=dt)
            ref.step_adam(*b, rows, grads.astype(dt), 0.1, t, weight_decay=0.0, mode=mode, dtype=dt)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


# ---- the fp64 model is torch's optimizers when every row is named in every step (lazy == dense) ----------------------

def _dense_case(D, steps=4, R=9, seed=1):
    rng = np.random.default_rng(seed)
    W0 = rng.standard_normal((R, D))
    grads = [rng.standard_normal((R, D)) for _ in range(steps)]
    return W0, np.arange(R), grads


def _torch_run(make, W0, grads):
    p = torch.nn.Parameter(torch.from_numpy(W0.copy()))
    opt = make([p])
    for g in grads:
        p.grad = torch.from_numpy(g.astype(W0.dtype))
        opt.step()
    return p.detach().numpy(), opt.state[p]


def test_sgd_l2_is_torch_sgd():
    W0, rows, grads = _dense_case(6)
    W = W0.copy()
    for g in grads:
        ref.step_sgd(W, rows, g, 0.1, 0.05, "l2")
    want, _ = _torch_run(lambda ps: torch.optim.SGD(ps, lr=0.1, weight_decay=0.05), W0, grads)
    np.testing.assert_allclose(W, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("mode", ref.MODES)
def test_adam_is_torch_adam_and_adamw(mode):
    W0, rows, grads = _dense_case(6)
    W, M, V = W0.copy(), np.zeros_like(W0), np.zeros_like(W0)
    for t, g in enumerate(grads, 1):
        ref.step_adam(W, M, V, rows, g, 0.1, t, (0.9, 0.999), 0.0, 0.05, mode)
    cls = torch.optim.Adam if mode == "l2" else torch.optim.AdamW
    # eps = 0: torch.optim.Adam adds eps to sqrt(v) / sqrt(1 - beta2^t), the model (SparseAdam's form, as the kernels)
    # to sqrt(v) -- with eps = 0 the two are one formula
    want, st = _torch_run(lambda ps: cls(ps, lr=0.1, betas=(0.9, 0.999), eps=0.0, weight_decay=0.05), W0, grads)
    np.testing.assert_allclose(W, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(M, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(V, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-12)


def test_adagrad_l2_is_torch_adagrad_at_dim_one():
    W0, rows, grads = _dense_case(1)                                  # row-wise and element-wise coincide at D = 1
    W, M = W0.copy(), np.zeros(len(W0))
    for g in grads:
        ref.step_adagrad(W, M, rows, g, 0.1, 1e-8, 0.05, "l2")
    want, st = _torch_run(lambda ps: torch.optim.Adagrad(ps, lr=0.1, lr_decay=0, eps=1e-8, weight_decay=0.05), W0, grads)
    np.testing.assert_allclose(W, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(M, st["sum"].numpy().reshape(-1), rtol=1e-12, atol=1e-12)


def test_decoupled_sgd_and_adagrad_by_hand():
    """torch has neither: the formulas on three rows, worked out by hand.  lr = 0.5, wd = 0.2: f = 0.9."""
    W = np.array([[1.0, -2.0], [4.0, 0.5], [3.0, 3.0]])
    ref.step_sgd(W, np.array([0, 1]), np.array([[0.2, 0.4], [-1.0, 0.0]]), 0.5, 0.2, "decoupled")
    np.testing.assert_allclose(W, [[0.9 - 0.1, -1.8 - 0.2], [3.6 + 0.5, 0.45], [3.0, 3.0]], rtol=1e-15)
    W = np.array([[1.0, -2.0], [4.0, 0.5], [3.0, 3.0]])
    M = np.array([0.0, 1.0, 7.0])
    ref.step_adagrad(W, M, np.array([0, 1]), np.array([[3.0, 4.0], [0.0, 0.0]]), 0.5, 0.0, 0.2, "decoupled")
    # row 0: m = (9 + 16) / 2 = 12.5, w = 0.9 w - 0.5 g / sqrt(12.5); row 1: g = 0, m stays 1, w = 0.9 w
    s = 0.5 / np.sqrt(12.5)
    np.testing.assert_allclose(W, [[0.9 - 3 * s, -1.8 - 4 * s], [3.6, 0.45], [3.0, 3.0]], rtol=1e-15)
    np.testing.assert_allclose(M, [12.5, 1.0, 7.0], rtol=1e-15)
    # and l2 Adagrad: h = g + 0.2 w feeds the sum of squares too
    W = np.array([[1.0, -2.0]])
    M = np.zeros(1)
    ref.step_adagrad(W, M, np.array([0]), np.array([[3.0, 4.0]]), 0.5, 0.0, 0.2, "l2")
    h = np.array([3.2, 3.6])
    np.testing.assert_allclose(M, [(h * h).sum() / 2], rtol=1e-15)
    np.testing.assert_allclose(W, [np.array([1.0, -2.0]) - 0.5 * h / np.sqrt((h * h).sum() / 2)], rtol=1e-15)


# ---- the lazy rule and the skip rules -------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adam"])
def test_lazy_rule_and_skip_rules(opt, mode):
    R, D = 8, 4
    rng = np.random.default_rng(3)
    W0 = rng.standard_normal((R, D))
    # bags cover positions [0, 5): row 0 twice, row 1 with weight zero only, slot -1; the tail names row 6 uncovered
    ids = np.array([0, 1, -1, 0, 2, 6, 6])
    off = np.array([0, 2, 5])
    psw = np.array([1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0], np.float32)
    go = rng.standard_normal((2, D))
    rows, grads = ref.lookup_grads(ids, off, go, R, psw=psw)
    assert sorted(set(rows.tolist())) == [0, 1, 2]
    W = W0.copy()
    if opt == "sgd":
        ref.step_sgd(W, rows, grads, 0.1, 0.3, mode)
    elif opt == "adagrad":
        M = np.full(R, 0.5)
        ref.step_adagrad(W, M, rows, grads, 0.1, 1e-8, 0.3, mode)
        np.testing.assert_array_equal(M[3:], 0.5)
    else:
        M, V = np.zeros_like(W), np.full_like(W, 0.01)
        ref.step_adam(W, M, V, rows, grads, 0.1, 1, weight_decay=0.3, mode=mode)
        assert not M[3:].any() and (V[3:] == 0.01).all()
    np.testing.assert_array_equal(W[3:], W0[3:])                      # not named, the uncovered tail's row 6 among them
    assert (np.abs(W[1]) < np.abs(W0[1])).all()                       # named with weight zero only: g = 0, it decays
    assert (W[0] != W0[0]).all() and (W[2] != W0[2]).all()
    # a row whose momentum index lies outside the momentum is not touched, so it does not decay either
    if opt == "adagrad":
        W = W0.copy()
        ref.step_adagrad(W, np.zeros(2), rows, grads, 0.1, 1e-8, 0.3, mode, row_of=np.array([0, 5, -1, 0, 0, 0, 0, 0]))
        np.testing.assert_array_equal(W[1:], W0[1:])
        assert (W[0] != W0[0]).all()


# ---- the evidence for the GPU tolerance: fp32 runs of the GPU test's workload stay within it ------------------------

@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("opt", ["adagrad", "adam", "sgd"])
def test_fp32_runs_keep_the_gpu_tolerance_on_the_gpu_workload(opt, mode):
    R, D = 70, 100
    rng = np.random.default_rng(100 * D + R)
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    steps = ref.steps(R, D, False, seed=D + R)
    want = ref.run_model(opt, W0, steps, mode)
    got = ref.run_model(opt, W0, steps, mode, dtype=np.float32)
    assert want[-1][ref.HOT] and not want[-1][R - 5:].any()
    for k, (a, b) in enumerate(zip(got[:-1], want[:-1])):
        err = np.abs(a.astype(np.float64) - b) - RTOL * np.abs(b)
        print(f"{opt} {mode} part {k}: model fp32 vs fp64, max (|err| - rtol |ref|) = {err.max():.3g}")
        np.testing.assert_allclose(a.astype(np.float64), b, rtol=RTOL, atol=ATOL)


def _workload_folded(R, D):
    rng = np.random.default_rng(100 * D + R)
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    folded = []
    for s in ref.steps(R, D, False, seed=D + R):
        rows, grads = ref.lookup_grads(s["ids"], s["off"], s["go"], R, mode=s["mode"], psw=s["psw"],
                                       hook_features=s["hook"])
        g = np.zeros((R, D))
        np.add.at(g, rows, grads)
        folded.append(g)
    return W0, folded


@pytest.mark.parametrize("mode", ref.MODES)
def test_torch_fp32_adam_keeps_the_gpu_tolerance_on_the_gpu_gradients(mode):
    """torch's own fp32 Adam / AdamW over the workload's folded gradients, dense (every row in every step, in torch and
    in the model alike), from the moments the GPU test starts from, against the fp64 model: the tolerance is not the
    model's alone"""
    R, D = 70, 100
    W0, folded = _workload_folded(R, D)
    v0 = ref.adam_v0(mode, ref.WD)
    W, M, V = W0.astype(np.float64), np.zeros((R, D)), np.full((R, D), v0)
    p = torch.nn.Parameter(torch.from_numpy(W0.copy()))
    cls = torch.optim.Adam if mode == "l2" else torch.optim.AdamW
    # eps = 0 on both sides: torch.optim.Adam adds eps to sqrt(v) / sqrt(1 - beta2^t), the model to sqrt(v), and the
    # workload's smallest sqrt(v) is 50 eps -- the two FORMULAS differ there by 2 %, which is no rounding error
    opt = cls([p], lr=ref.LR, betas=ref.BETAS, eps=0.0, weight_decay=ref.WD)
    opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p.data),
                    "exp_avg_sq": torch.full_like(p.data, v0)}
    with np.errstate(invalid="ignore"):
        for t, g in enumerate(folded, 1):
            ref.step_adam(W, M, V, np.arange(R), g, ref.LR, t, ref.BETAS, 0.0, ref.WD, mode)
            p.grad = torch.from_numpy(g.astype(np.float32))
            opt.step()
    sel = V > 0                                                        # (never named from v = 0: 0 / 0 on both sides)
    assert sel[ref.HOT].all() and sel.mean() > 0.9
    np.testing.assert_allclose(p.detach().numpy().astype(np.float64)[sel], W[sel], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(opt.state[p]["exp_avg"].numpy().astype(np.float64), M, rtol=RTOL, atol=ATOL)


def test_torch_fp32_sgd_keeps_the_gpu_tolerance_on_the_gpu_gradients():
    R, D = 70, 100
    W0, folded = _workload_folded(R, D)
    W = W0.astype(np.float64)
    p = torch.nn.Parameter(torch.from_numpy(W0.copy()))
    opt = torch.optim.SGD([p], lr=ref.LR, weight_decay=ref.WD)
    for g in folded:
        ref.step_sgd(W, np.arange(R), g, ref.LR, ref.WD, "l2")
        p.grad = torch.from_numpy(g.astype(np.float32))
        opt.step()
    np.testing.assert_allclose(p.detach().numpy().astype(np.float64), W, rtol=RTOL, atol=ATOL)


# ---- the C entries, without a GPU: everything is refused before a HIP call -------------------------------------------

def _entries():
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    return _lib, _lib.lib


P = ctypes.c_void_p
_SLOTS = (P(0x5000), 5, P(0x6000), 1, 5, 1, None, 0, 0, P(0x3000), 0)          # indices .. grad_out, act_dtype
_SRC = (5, P(0x3000), 0, P(0x4000))                                            # nnz, grad_out, act_dtype, keys


def _update(lib, src, wd=0.05, wd_mode=1, acc=0, wdt=0, opt=1, lr=0.1, eps=1e-8, dim=8, ws_bytes=1 << 30, weight=0x2000):
    """pointers are fake (aligned, never dereferenced: every call here is refused before a launch)"""
    tail = (None, P(0x7000), 10, lr, None, eps, wd, wd_mode, opt, 0, 0, acc, P(0x10000), ws_bytes, None)
    if src:
        return lib.ce_bag_backward_update_src_wd(P(weight), wdt, 10, dim, *_SRC, *tail)
    return lib.ce_bag_backward_update_wd(P(weight), wdt, 10, dim, *_SLOTS, None, *tail)


def _sorted(lib, wd=0.05, wd_mode=1, wdt=0, act=0, ws_bytes=1 << 30, rounding=0):
    slots = _SLOTS[:-1] + (act,)
    return lib.ce_bag_backward_update_sorted_wd(P(0x2000), wdt, 10, 8, *slots, None, P(0x7000), 10, 0.1, 1e-8, wd, wd_mode,
                                                1, rounding, 0, P(0x10000), ws_bytes, None)


def _adam(lib, src, wd=0.05, wd_mode=2, step=0x1000, acc=0, beta1=0.9, dim=8, ws_bytes=1 << 30):
    tail = (beta1, 0.999, 0.1, None, 1e-8, wd, wd_mode, P(step) if step else None, acc, P(0x10000), ws_bytes, None)
    if src:
        return lib.ce_bag_backward_adam_src_wd(P(0x2000), 10, dim, *_SRC, *tail)
    return lib.ce_bag_backward_adam_wd(P(0x2000), 10, dim, *_SLOTS, None, *tail)


BAD_DECAY = (dict(wd_mode=3), dict(wd_mode=-1), dict(wd=-0.01), dict(wd=float("nan")))


@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
def test_update_entries_refuse_before_anything_happens(src):
    _lib, lib = _entries()
    INV, UNS = _lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED
    # the accumulator code leads; the decay's mode, then its value, come before every refusal of the covered entry
    assert _update(lib, src, acc=7, wd_mode=3, wdt=9) == INV and "accumulator" in _lib.last_error()
    for acc in (_lib.CE_ACC_CACHE, _lib.CE_ACC_STEP):
        assert _update(lib, src, acc=acc, wd_mode=3, wd=-1.0, wdt=9) == INV and "weight_decay_mode" in _lib.last_error()
        for bad in BAD_DECAY:
            for later in (dict(wdt=9), dict(opt=5), dict(lr=-1.0), dict(ws_bytes=0), dict(dim=0), dict(wdt=0, opt=0)):
                assert _update(lib, src, acc=acc, **bad, **later) == INV, (bad, later)
                assert "weight_decay" in _lib.last_error()
        assert _update(lib, src, acc=acc, wd=-0.01, wdt=9) == INV and "weight_decay must" in _lib.last_error()
        # ... then the covered entry's own, with its codes: an unknown table, fp32 + SGD, a small workspace
        assert _update(lib, src, acc=acc, wdt=9) == INV and "weight_dtype" in _lib.last_error()
        assert _update(lib, src, acc=acc, wdt=0, opt=_lib.CE_OPT_SGD) == UNS and "fp32 table" in _lib.last_error()
        assert _update(lib, src, acc=acc, lr=-1.0) == INV and "lr" in _lib.last_error()
        assert _update(lib, src, acc=acc, ws_bytes=0) == INV and "workspace too small" in _lib.last_error()
        for wdt in (1, 2):
            assert _update(lib, src, acc=acc, wdt=wdt, opt=0, ws_bytes=0) == INV and "workspace" in _lib.last_error()
    # the decay checks also hold for nnz == 0, where the fp32 cache-sized entry returns before it looks at anything
    tail = (None, P(0x7000), 10, 0.1, None, 1e-8, 0.05, 5, 1, 0, 0, 0, P(0x10000), 0, None)
    if src:
        assert lib.ce_bag_backward_update_src_wd(P(0x2000), 0, 10, 8, 0, P(0x3000), 0, P(0x4000), *tail) == INV
    else:
        assert lib.ce_bag_backward_update_wd(P(0x2000), 0, 10, 8, P(0x5000), 0, P(0x6000), 1, 5, 1, None, 0, 0, P(0x3000),
                                             0, None, *tail) == INV
    assert "weight_decay_mode" in _lib.last_error()
    # CE_WD_NONE and a zero decay are legal in every mode: the call gets as far as the workspace
    for kw in (dict(wd_mode=0), dict(wd=0.0, wd_mode=1), dict(wd=0.0, wd_mode=2)):
        assert _update(lib, src, ws_bytes=0, **kw) == INV and "workspace too small" in _lib.last_error()


def test_sorted_entry_refuses_before_anything_happens():
    _lib, lib = _entries()
    INV, UNS = _lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED
    for bad in BAD_DECAY:                                              # first: before an unknown act_dtype / table
        assert _sorted(lib, act=9, wdt=9, **bad) == INV and "weight_decay" in _lib.last_error()
    assert _sorted(lib, wd_mode=3, wd=-1.0) == INV and "weight_decay_mode" in _lib.last_error()
    assert _sorted(lib, act=9) == INV and "activation" in _lib.last_error()
    assert _sorted(lib, wdt=1, rounding=1) == UNS and "STOCHASTIC" in _lib.last_error()
    assert _sorted(lib, ws_bytes=0) == INV and "workspace too small" in _lib.last_error()


@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
def test_adam_entries_refuse_before_anything_happens(src):
    _lib, lib = _entries()
    INV, UNS = _lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED
    assert _adam(lib, src, step=0, acc=7, wd_mode=3) == INV and "step" in _lib.last_error()
    assert _adam(lib, src, acc=7, wd_mode=3) == INV and "accumulator" in _lib.last_error()
    for bad in BAD_DECAY:
        for later in (dict(beta1=1.5), dict(dim=6), dict(ws_bytes=0)):
            assert _adam(lib, src, **bad, **later) == INV and "weight_decay" in _lib.last_error(), (bad, later)
    assert _adam(lib, src, wd_mode=3, wd=-1.0) == INV and "weight_decay_mode" in _lib.last_error()
    assert _adam(lib, src, beta1=1.5) == INV and "beta" in _lib.last_error()
    assert _adam(lib, src, dim=6) == UNS
    assert _adam(lib, src, ws_bytes=0) == INV and "workspace too small" in _lib.last_error()


# ---- the Python surface ---------------------------------------------------------------------------------------------

def test_python_keywords_and_refusals_without_a_device():
    from cachedembedding_amd import functional as Fn
    from cachedembedding_amd.cached_embedding import CachedEmbeddingBag
    from cachedembedding_amd.parallel import ParallelCachedEmbeddingBag, RowwiseShardedEmbeddingBag
    for cls in (Fn.FusedSGD, Fn.FusedRowwiseAdagrad, Fn.FusedAdam):
        f = cls(0.1)
        assert f.weight_decay == 0.0 and f.weight_decay_mode == "l2"
        f = cls(0.1, weight_decay=0.05, weight_decay_mode="decoupled")
        assert f.weight_decay == 0.05 and f.weight_decay_mode == "decoupled"
        with pytest.raises(TypeError):
            cls(0.1, None, None, None, None, None, None, 0.05)         # keyword-only
        with pytest.raises(ValueError, match="weight_decay_mode"):
            cls(0.1, weight_decay=0.1, weight_decay_mode="L2")
        for bad in (-0.1, float("nan")):
            with pytest.raises(ValueError, match="weight_decay"):
                cls(0.1, weight_decay=bad)
    f = Fn.FusedAdam(0.1)
    f.set((0.9, 0.99), 1e-8, "cache", weight_decay=0.2, weight_decay_mode="decoupled")
    assert (f.weight_decay, f.weight_decay_mode) == (0.2, "decoupled")
    with pytest.raises(ValueError):
        f.set((0.9, 0.99), 1e-8, "cache", weight_decay=-1.0)
    # what the paths do not take
    with pytest.raises(NotImplementedError, match=r"no per-row\s+pass.*deterministic=True"):
        Fn.check_weight_decay_path("sgd", torch.float32, 0.1)
    Fn.check_weight_decay_path("sgd", torch.float32, 0.1, deterministic=True)
    Fn.check_weight_decay_path("sgd", torch.bfloat16, 0.1)
    Fn.check_weight_decay_path("sgd", torch.float32, 0.0, mode="max")
    for opt in ("sgd", "rowwise_adagrad"):
        with pytest.raises(NotImplementedError, match="mode='max'"):
            Fn.check_weight_decay_path(opt, torch.bfloat16, 0.1, mode="max")
        with pytest.raises(NotImplementedError, match="tensor learning rate"):
            Fn.check_weight_decay_path(opt, torch.bfloat16, 0.1, True, torch.zeros(1))
    with pytest.raises(NotImplementedError):
        Fn.FusedRowwiseAdagrad(torch.zeros(1), deterministic=True, weight_decay=0.1)
    # embedding_bag asks again, before any kernel (a CPU weight never reaches one)
    w = torch.zeros(4, 8, requires_grad=True)
    ids, off = torch.arange(4), torch.arange(5)
    with pytest.raises(NotImplementedError, match="deterministic=True"):
        Fn.embedding_bag(ids, w, off, mode="sum", include_last_offset=True, fused_sgd=Fn.FusedSGD(0.1, weight_decay=0.1))
    with pytest.raises(NotImplementedError, match="mode='max'"):
        Fn.embedding_bag(ids, w, off, mode="max", include_last_offset=True,
                         fused_sgd=Fn.FusedSGD(0.1, deterministic=True, weight_decay=0.1))
    # the module's setters (on a stub: no device), the sharded and table-wise modules
    mgr = types.SimpleNamespace(momentum1=torch.zeros(4), cached_idx_map=None, num_embeddings=4, device="cpu")

    def stub(**kw):
        return types.SimpleNamespace(mode="sum", table_dtype=torch.float32, weight_rounding="stochastic",
                                     fused_sgd=Fn.FusedSGD(), fused_adagrad=Fn.FusedRowwiseAdagrad(), cache_weight_mgr=mgr,
                                     **kw)
    s = stub()
    with pytest.raises(NotImplementedError, match="deterministic=True"):
        CachedEmbeddingBag.set_fused_sgd(s, 0.1, weight_decay=0.1)
    assert s.fused_sgd.lr is None and s.fused_sgd.weight_decay == 0.0
    CachedEmbeddingBag.set_fused_sgd(s, 0.1, deterministic=True, weight_decay=0.1, weight_decay_mode="decoupled")
    assert (s.fused_sgd.weight_decay, s.fused_sgd.weight_decay_mode) == (0.1, "decoupled")
    s = stub()
    CachedEmbeddingBag.set_fused_rowwise_adagrad(s, 0.1, weight_decay=0.3)
    assert (s.fused_adagrad.weight_decay, s.fused_adagrad.weight_decay_mode) == (0.3, "l2")
    with pytest.raises(ValueError):
        CachedEmbeddingBag.set_fused_rowwise_adagrad(s, 0.1, weight_decay=0.3, weight_decay_mode="cowclip")
    for name in ("ParallelCachedEmbeddingBag", "ParallelCachedEmbeddingBagTablewise"):
        s = stub(_no_weight_decay=name)
        for call in (lambda: CachedEmbeddingBag.set_fused_sgd(s, 0.1, weight_decay=0.1),
                     lambda: CachedEmbeddingBag.set_fused_rowwise_adagrad(s, 0.1, weight_decay=0.1)):
            with pytest.raises(NotImplementedError, match="ce_rows_axpy"):
                call()
        CachedEmbeddingBag.set_fused_rowwise_adagrad(s, 0.1)
    assert ParallelCachedEmbeddingBag._no_weight_decay and CachedEmbeddingBag._no_weight_decay is None
    shard = types.SimpleNamespace(_lr=[None])
    with pytest.raises(NotImplementedError, match="ce_rows_axpy"):
        RowwiseShardedEmbeddingBag.set_fused_sgd(shard, 0.1, weight_decay=0.1)
    assert shard._lr == [None]
    RowwiseShardedEmbeddingBag.set_fused_sgd(shard, 0.1)


def test_example_parses_the_flags_and_refuses_what_it_must():
    sys.path.insert(0, str(HERE.parent / "examples"))
    dm = importlib.import_module("dlrm_main")
    a = dm.parse_args(["--use_cache", "--adagrad"])
    assert a.embed_weight_decay == 0.0 and a.embed_weight_decay_mode == "l2"
    a = dm.parse_args(["--use_cache", "--adam", "--embed_weight_decay", "0.01", "--embed_weight_decay_mode", "decoupled"])
    assert dm._decay(a) == {"weight_decay": 0.01, "weight_decay_mode": "decoupled"}
    with pytest.raises(SystemExit):
        dm.parse_args(["--embed_weight_decay_mode", "cowclip"])
    with pytest.raises(ValueError, match="--adagrad, --adam or"):
        dm.main(["--use_cache", "--embed_weight_decay", "0.01"])
    with pytest.raises(ValueError, match="weight_decay"):
        dm.main(["--use_cache", "--adagrad", "--embed_weight_decay", "-1"])
    with pytest.raises(NotImplementedError, match="no per-row"):
        dm.main(["--use_cache", "--fused_sgd", "--embed_weight_decay", "0.01"])
    for argv in (["--adagrad"], ["--adam"], ["--adagrad", "--adagrad_deterministic"], ["--fused_sgd", "--table_dtype", "bf16"]):
        dm.check_embed_weight_decay(dm.parse_args(["--use_cache", "--embed_weight_decay", "0.01"] + argv))
