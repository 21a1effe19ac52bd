"""Gradient clipping of the fused updates without a GPU: the numpy model (tests/grad_clip_ref.py)
against the existing references and against torch's clip_grad_value_ / clip_grad_norm_ + optimizers on the CPU, the
condition that the GPU test's workloads have gradients on both sides of the threshold, the evidence for the GPU test's
tolerance on its own workload, the refusals of the seven ce_*_clip entries and of the Python surface, and the example's
two flags."""
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
import grad_clip_ref as ref  # noqa: E402
import partial_rowwise_adam_ref as pradam_ref  # noqa: E402
import weight_decay_ref as wref  # noqa: E402

RTOL, ATOL = 1e-5, 1e-6                       # the GPU test's (test_gpu_grad_clip.py): the project's own


# ---- the clip itself -------------------------------------------------------------------------------------------------

def test_clip_by_hand():
    g = np.array([[3.0, -4.0, 0.5], [0.3, 0.4, 0.0], [np.nan, 9.0, -9.0], [0.0, 0.0, 0.0]])
    v = ref.clip(g, 1.0, "value")
    np.testing.assert_array_equal(v[:2], [[1.0, -1.0, 0.5], [0.3, 0.4, 0.0]])
    assert np.isnan(v[2, 0]) and v[2, 1] == 1.0 and v[2, 2] == -1.0           # a NaN stays a NaN, as torch.clamp
    np.testing.assert_array_equal(v[3], 0.0)
    n = ref.clip(g[:2], 1.0, "row_norm")
    k = 1.0 / (np.sqrt(25.25) + 1e-6)
    np.testing.assert_allclose(n[0], g[0] * k, rtol=1e-15)
    np.testing.assert_array_equal(n[1], g[1])                               # |row| = 0.5 < 1: untouched, bit for bit
    for mode in ref.MODES:                                                   # +inf changes nothing; zeros stay zeros
        np.testing.assert_array_equal(ref.clip(g[[0, 1, 3]], np.inf, mode), g[[0, 1, 3]])
        np.testing.assert_array_equal(ref.clip(g[3:], 1e-9, mode), g[3:])
    t = torch.tensor(g[:2])
    np.testing.assert_array_equal(ref.clip(g[:2], 1.0, "value"), torch.clamp(t, -1.0, 1.0).numpy())


@pytest.mark.parametrize("mode", wref.MODES)
def test_no_clip_reproduces_the_existing_references(mode):
    rng = np.random.default_rng(0)
    R, D = 12, 5
    W0 = rng.standard_normal((R, D))
    rows = rng.integers(0, R - 2, 30)
    grads = rng.standard_normal((30, D))
    for dt in (np.float64, np.float32):
        for wd in (0.0, 0.05):
            g = grads.astype(dt)
            a, b = W0.astype(dt), W0.astype(dt)
            for _ in range(3):
                wref.step_sgd(a, rows, g, 0.1, wd, mode, dt)
                ref.step_sgd(b, rows, g, 0.1, wd, mode, dt)
            np.testing.assert_array_equal(a, b)
            a, am, b, bm = W0.astype(dt), np.zeros(R, dt), W0.astype(dt), np.zeros(R, dt)
            for _ in range(3):
                wref.step_adagrad(a, am, rows, g, 0.1, 1e-8, wd, mode, dt)
                ref.step_adagrad(b, bm, rows, g, 0.1, 1e-8, wd, mode, dt)
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(am, bm)
            a = [W0.astype(dt), np.zeros((R, D), dt), np.full((R, D), 0.01, dt)]
            b = [x.copy() for x in a]
            for t in (1, 2, 3):
                wref.step_adam(*a, rows, g, 0.1, t, weight_decay=wd, mode=mode, dtype=dt)
                ref.step_adam(*b, rows, g, 0.1, t, weight_decay=wd, wd_mode=mode, dtype=dt)
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)
            a = [W0.astype(dt), np.zeros((R, D), dt), np.zeros(R, dt)]
            b = [x.copy() for x in a]
            for t in (1, 2, 3):
                pradam_ref.step(*a, rows, g, 0.1, t, dtype=dt, wd=wd, wd_mode=mode)
                ref.step_pradam(*b, rows, g, 0.1, t, weight_decay=wd, wd_mode=mode, dtype=dt)
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)


# ---- the fp64 model is torch's clip + torch's optimizers when every row is named in every step -----------------------

def _dense_case(D, steps=4, R=9, seed=1):
    rng = np.random.default_rng(seed)
    W0 = rng.standard_normal((R, D))
    grads = [rng.standard_normal((R, D)) * rng.uniform(0.1, 3.0, (R, 1)) for _ in range(steps)]
    return W0, np.arange(R), grads


def _torch_run(make, W0, grads, c, mode):
    """torch's clip in front of torch's optimizer; "row_norm": every row its own parameter"""
    if mode == "value":
        ps = [torch.nn.Parameter(torch.from_numpy(W0.copy()))]
    else:
        ps = [torch.nn.Parameter(torch.from_numpy(W0[r:r + 1].copy())) for r in range(len(W0))]
    opt = make(ps)
    for g in grads:
        if mode == "value":
            ps[0].grad = torch.from_numpy(g.copy())
            torch.nn.utils.clip_grad_value_(ps, c)
        else:
            for r, p in enumerate(ps):
                p.grad = torch.from_numpy(g[r:r + 1].copy())
                torch.nn.utils.clip_grad_norm_([p], c)
        opt.step()
    w = np.concatenate([p.detach().numpy() for p in ps])
    state = {k: np.concatenate([opt.state[p][k].numpy() for p in ps]) for k in ("exp_avg", "exp_avg_sq")
             if k in opt.state[ps[0]]}
    return w, state


def _both_sides(grads, c, mode):
    m = np.concatenate([ref.clipped_mask(g, c, mode).reshape(-1) for g in grads])
    return m.any() and not m.all()


@pytest.mark.parametrize("mode", ref.MODES)
def test_clipped_sgd_is_torch_clip_then_sgd(mode):
    W0, rows, grads = _dense_case(6)
    c = 1.0 if mode == "value" else 2.0
    assert _both_sides(grads, c, mode)
    W = W0.copy()
    for g in grads:
        ref.step_sgd(W, rows, g, 0.1, 0.05, "l2", grad_clip=c, clip_mode=mode)
    want, _ = _torch_run(lambda ps: torch.optim.SGD(ps, lr=0.1, weight_decay=0.05), W0, grads, c, mode)
    np.testing.assert_allclose(W, want, rtol=1e-12, atol=1e-12)
    plain = W0.copy()
    for g in grads:
        wref.step_sgd(plain, rows, g, 0.1, 0.05, "l2")
    assert np.abs(plain - W).max() > 1e-3                                     # the clip is in it


@pytest.mark.parametrize("wd_mode", wref.MODES)
@pytest.mark.parametrize("mode", ref.MODES)
def test_clipped_adam_is_torch_clip_then_adam_and_adamw(mode, wd_mode):
    W0, rows, grads = _dense_case(6)
    c = 1.0 if mode == "value" else 2.0
    W, M, V = W0.copy(), np.zeros_like(W0), np.zeros_like(W0)
    for t, g in enumerate(grads, 1):
        ref.step_adam(W, M, V, rows, g, 0.1, t, (0.9, 0.999), 0.0, 0.05, wd_mode, grad_clip=c, clip_mode=mode)
    cls = torch.optim.Adam if wd_mode == "l2" else torch.optim.AdamW
    # eps = 0: torch.optim.Adam adds eps to sqrt(v) / sqrt(1 - beta2^t), the model (SparseAdam's form) to sqrt(v)
    want, st = _torch_run(lambda ps: cls(ps, lr=0.1, betas=(0.9, 0.999), eps=0.0, weight_decay=0.05), W0, grads, c, mode)
    np.testing.assert_allclose(W, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(M, st["exp_avg"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(V, st["exp_avg_sq"], rtol=1e-12, atol=1e-12)


def test_clipped_adagrad_and_pradam_see_the_clipped_gradient_everywhere():
    """torch has neither optimizer: by hand on one row.  c = 1 (value): g = (3, -4) -> (1, -1); row_norm c = 1:
    g -> g / (5 + 1e-6).  The L2 term, the sum of squares, the moments and the step all use the clipped g."""
    for mode, gc in (("value", np.array([1.0, -1.0])), ("row_norm", np.array([3.0, -4.0]) / (5.0 + 1e-6))):
        W, M = np.array([[1.0, -2.0]]), np.zeros(1)
        ref.step_adagrad(W, M, np.array([0]), np.array([[3.0, -4.0]]), 0.5, 0.0, 0.2, "l2", grad_clip=1.0, clip_mode=mode)
        h = gc + 0.2 * np.array([1.0, -2.0])
        np.testing.assert_allclose(M, [(h * h).sum() / 2], rtol=1e-15)
        np.testing.assert_allclose(W, [np.array([1.0, -2.0]) - 0.5 * h / np.sqrt((h * h).sum() / 2)], rtol=1e-15)
        W, M, V = np.array([[1.0, -2.0]]), np.zeros((1, 2)), np.zeros(1)
        ref.step_pradam(W, M, V, np.array([0]), np.array([[3.0, -4.0]]), 0.5, 1, (0.9, 0.99), 0.0, grad_clip=1.0,
                        clip_mode=mode)
        v = 0.01 * (gc * gc).sum() / 2
        m = 0.1 * gc
        np.testing.assert_allclose(V, [v], rtol=1e-13)
        np.testing.assert_allclose(M, [m], rtol=1e-13)
        size = 0.5 * adam_ref.bias_correction(1, (0.9, 0.99))
        np.testing.assert_allclose(W, [np.array([1.0, -2.0]) - size * m / np.sqrt(v)], rtol=1e-13)


@pytest.mark.parametrize("mode", ref.MODES)
def test_clipping_does_not_change_which_rows_a_step_names(mode):
    R, D = 8, 4
    rng = np.random.default_rng(3)
    W0 = rng.standard_normal((R, D))
    ids = np.array([0, 1, -1, 0, 2, 6, 6])          # bags cover [0, 5): row 1 with weight zero only; the tail is uncovered
    off = np.array([0, 2, 5])
    psw = np.array([1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0], np.float32)
    rows, grads = ref.lookup_grads(ids, off, rng.standard_normal((2, D)), R, psw=psw)
    W, M = W0.copy(), np.full(R, 0.5)
    ref.step_adagrad(W, M, rows, grads, 0.1, grad_clip=0.01, clip_mode=mode)
    np.testing.assert_array_equal(W[3:], W0[3:])
    np.testing.assert_array_equal(W[1], W0[1])       # g = 0 without decay: a no-op for Adagrad (and SGD)
    assert M[1] == 0.5 and (M[3:] == 0.5).all()
    assert (W[0] != W0[0]).all() and (W[2] != W0[2]).all()
    W = W0.copy()                                    # a momentum index outside the momentum: the slot is not touched
    ref.step_adagrad(W, np.zeros(2), rows, grads, 0.1, grad_clip=0.01, clip_mode=mode,
                     row_of=np.array([0, 5, -1, 0, 0, 0, 0, 0]))
    np.testing.assert_array_equal(W[1:], W0[1:])


# ---- the GPU test's workloads: gradients on both sides of the threshold (a condition, not a tolerance) --------------

def _case(R, D, src):
    rng = np.random.default_rng(100 * D + R)
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    return W0, wref.steps(R, D, src, seed=D + R)


GPU_SHAPES = sorted({(R, D) for R in (70, 4100) for D in (4, 100, 128, 260, 1024)} |
                    {(R, D) for R in (70, 4100) for D in (8, 128, 264)})


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
@pytest.mark.parametrize("R,D", GPU_SHAPES)
def test_every_gpu_workload_has_gradients_on_both_sides_of_the_threshold(R, D, src, mode):
    W0, steps = _case(R, D, src)
    stats = {}
    ref.run_model("sgd", W0, steps, mode, stats=stats)
    share = stats["clipped"] / (stats["clipped"] + stats["kept"])
    print(f"R={R} D={D} {'src' if src else 'slots'} {mode}: {stats['clipped']} clipped, {stats['kept']} kept ({share:.1%})")
    assert stats["clipped"] > 0 and stats["kept"] > 0


# ---- the evidence for the GPU tolerance: fp32 runs of the GPU test's workload stay within it ------------------------

@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("opt,wd,wd_mode", [("adagrad", 0.0, "l2"), ("adam", 0.0, "l2"), ("pradam", 0.0, "l2"),
                                            ("sgd", 0.0, "l2"), ("adagrad", wref.WD, "l2"), ("adam", wref.WD, "l2"),
                                            ("pradam", wref.WD, "decoupled"), ("sgd", wref.WD, "decoupled")])
def test_fp32_runs_keep_the_gpu_tolerance_on_the_gpu_workload(opt, wd, wd_mode, mode):
    R, D = 70, 100
    W0, steps = _case(R, D, False)
    want = ref.run_model(opt, W0, steps, mode, wd=wd, wd_mode=wd_mode)
    got = ref.run_model(opt, W0, steps, mode, wd=wd, wd_mode=wd_mode, dtype=np.float32)
    assert want[-1][wref.HOT] and not want[-1][R - 5:].any()
    for k, (a, b) in enumerate(zip(got[:-1], want[:-1])):
        err = np.abs(a.astype(np.float64) - b) - RTOL * np.abs(b)
        print(f"{opt} {mode} wd={wd} {wd_mode} part {k}: model fp32 vs fp64, max (|err| - rtol |ref|) = {err.max():.3g}")
        np.testing.assert_allclose(a.astype(np.float64), b, rtol=RTOL, atol=ATOL)
    unclipped = ref.run_model(opt, W0, steps, mode, grad_clip=None, wd=wd, wd_mode=wd_mode)
    assert np.abs(unclipped[0] - want[0]).max() > 100 * ATOL                 # the clip is in it


def _workload_folded(R, D):
    W0, steps = _case(R, D, False)
    folded = []
    for s in steps:
        rows, grads = ref.lookup_grads(s["ids"], s["off"], s["go"], R, mode=s["mode"], psw=s["psw"],
                                       hook_features=s["hook"])
        g = np.zeros((R, D))
        np.add.at(g, rows, grads)
        folded.append(g)
    return W0, folded


@pytest.mark.parametrize("mode", ref.MODES)
def test_torch_fp32_clip_and_sgd_keep_the_gpu_tolerance_on_the_gpu_gradients(mode):
    """torch's own fp32 clip + SGD over the workload's folded gradients, dense (every row in every step, in torch and in
    the model alike), against the fp64 model: the tolerance is not the model's alone"""
    R, D = 70, 100
    W0, folded = _workload_folded(R, D)
    c = ref.threshold(mode, D)
    W = W0.astype(np.float64)
    for g in folded:
        ref.step_sgd(W, np.arange(R), g, wref.LR, wref.WD, "l2", grad_clip=c, clip_mode=mode)
    want, _ = _torch_run(lambda ps: torch.optim.SGD(ps, lr=wref.LR, weight_decay=wref.WD), W0.astype(np.float32),
                         [g.astype(np.float32) for g in folded], c, mode)
    assert want.dtype == np.float32
    np.testing.assert_allclose(want.astype(np.float64), W, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("mode", ref.MODES)
def test_torch_fp32_clip_and_adam_keep_the_gpu_tolerance_on_the_gpu_gradients(mode):
    """the same with torch.optim.Adam (no decay; eps = 0 on both sides, as in test_weight_decay_cpu.py), from v = 0.01 so
    that rows a step does not name divide by something"""
    R, D = 70, 100
    W0, folded = _workload_folded(R, D)
    c = ref.threshold(mode, D)
    W, M, V = W0.astype(np.float64), np.zeros((R, D)), np.full((R, D), 0.01)
    if mode == "value":
        ps = [torch.nn.Parameter(torch.from_numpy(W0.copy()))]
    else:
        ps = [torch.nn.Parameter(torch.from_numpy(W0[r:r + 1].copy())) for r in range(R)]
    opt = torch.optim.Adam(ps, lr=wref.LR, betas=wref.BETAS, eps=0.0)
    for p in ps:
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p.data),
                        "exp_avg_sq": torch.full_like(p.data, 0.01)}
    for t, g in enumerate(folded, 1):
        ref.step_adam(W, M, V, np.arange(R), g, wref.LR, t, wref.BETAS, 0.0, grad_clip=c, clip_mode=mode)
        g32 = g.astype(np.float32)
        if mode == "value":
            ps[0].grad = torch.from_numpy(g32.copy())
            torch.nn.utils.clip_grad_value_(ps, c)
        else:
            for r, p in enumerate(ps):
                p.grad = torch.from_numpy(g32[r:r + 1].copy())
                torch.nn.utils.clip_grad_norm_([p], c)
        opt.step()
    got = np.concatenate([p.detach().numpy() for p in ps]).astype(np.float64)
    np.testing.assert_allclose(got, W, rtol=RTOL, atol=ATOL)


# ---- the C entries, without a GPU: everything is refused before a HIP call -------------------------------------------

def _entries():
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    return _lib, _lib.lib


P = ctypes.c_void_p
_SLOTS = (P(0x5000), 5, P(0x6000), 1, 5, 1, None, 0, 0, P(0x3000), 0)          # indices .. grad_out, act_dtype
_SRC = (5, P(0x3000), 0, P(0x4000))                                            # nnz, grad_out, act_dtype, keys


def _update(lib, src, clip=0.05, clip_mode=1, wd=0.05, wd_mode=1, acc=0, wdt=0, opt=1, lr=0.1, dim=8, ws_bytes=1 << 30):
    """pointers are fake (aligned, never dereferenced: every call here is refused before a launch)"""
    tail = (None, P(0x7000), 10, lr, None, 1e-8, wd, wd_mode, clip, clip_mode, opt, 0, 0, acc, P(0x10000), ws_bytes, None)
    if src:
        return lib.ce_bag_backward_update_src_clip(P(0x2000), wdt, 10, dim, *_SRC, *tail)
    return lib.ce_bag_backward_update_clip(P(0x2000), wdt, 10, dim, *_SLOTS, None, *tail)


def _sorted(lib, clip=0.05, clip_mode=1, wd=0.05, wd_mode=1, wdt=0, act=0, ws_bytes=1 << 30, rounding=0, opt=1):
    slots = _SLOTS[:-1] + (act,)
    return lib.ce_bag_backward_update_sorted_clip(P(0x2000), wdt, 10, 8, *slots, None, P(0x7000), 10, 0.1, 1e-8, wd,
                                                  wd_mode, clip, clip_mode, opt, rounding, 0, P(0x10000), ws_bytes, None)


def _adam(lib, src, partial, clip=0.05, clip_mode=2, wd=0.05, wd_mode=2, step=0x1000, acc=0, beta1=0.9, dim=8,
          ws_bytes=1 << 30, v=0x7000):
    tail = (beta1, 0.999, 0.1, None, 1e-8, wd, wd_mode, clip, clip_mode, P(step) if step else None, acc, P(0x10000),
            ws_bytes, None)
    if partial:
        tail = (None, P(v) if v else None, 10) + tail
        if src:
            return lib.ce_bag_backward_pradam_src_clip(P(0x2000), 10, dim, *_SRC, *tail)
        return lib.ce_bag_backward_pradam_clip(P(0x2000), 10, dim, *_SLOTS, None, *tail)
    if src:
        return lib.ce_bag_backward_adam_src_clip(P(0x2000), 10, dim, *_SRC, *tail)
    return lib.ce_bag_backward_adam_clip(P(0x2000), 10, dim, *_SLOTS, None, *tail)


BAD_CLIP = (dict(clip_mode=3), dict(clip_mode=-1), dict(clip=0.0), dict(clip=-0.01), dict(clip=float("nan")))


@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
def test_update_entries_refuse_before_anything_happens(src):
    _lib, lib = _entries()
    INV, UNS = _lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED
    assert (_lib.CE_CLIP_NONE, _lib.CE_CLIP_VALUE, _lib.CE_CLIP_ROW_NORM) == (0, 1, 2) and lib.ce_version() == 6
    # the accumulator code, then the decay's two, then the clip's two, then the covered entry's own
    assert _update(lib, src, acc=7, wd_mode=3, clip_mode=3) == INV and "accumulator" in _lib.last_error()
    for acc in (_lib.CE_ACC_CACHE, _lib.CE_ACC_STEP):
        assert _update(lib, src, acc=acc, wd_mode=3, clip_mode=3) == INV and "weight_decay_mode" in _lib.last_error()
        assert _update(lib, src, acc=acc, wd=-1.0, clip_mode=3) == INV and "weight_decay must" in _lib.last_error()
        assert _update(lib, src, acc=acc, clip_mode=3, clip=-1.0, wdt=9) == INV and "grad_clip_mode" in _lib.last_error()
        for bad in BAD_CLIP:
            for later in (dict(wdt=9), dict(opt=5), dict(lr=-1.0), dict(ws_bytes=0), dict(dim=0), dict(wdt=0, opt=0)):
                assert _update(lib, src, acc=acc, **bad, **later) == INV, (bad, later)
                assert "grad_clip" in _lib.last_error()
        assert _update(lib, src, acc=acc, clip=0.0, wdt=9) == INV and "grad_clip must" in _lib.last_error()
        assert _update(lib, src, acc=acc, wdt=9) == INV and "weight_dtype" in _lib.last_error()
        # fp32 + SGD stays unsupported in the atomic entries, with either clip
        for mode in (1, 2):
            assert _update(lib, src, acc=acc, wdt=0, opt=_lib.CE_OPT_SGD, clip_mode=mode) == UNS
            assert "fp32 table" in _lib.last_error()
        assert _update(lib, src, acc=acc, ws_bytes=0) == INV and "workspace too small" in _lib.last_error()
        # +inf is a threshold; CE_CLIP_NONE looks at no threshold: both get as far as the workspace
        for kw in (dict(clip=float("inf")), dict(clip_mode=0, clip=-1.0), dict(clip_mode=0, clip=float("nan"))):
            assert _update(lib, src, acc=acc, ws_bytes=0, **kw) == INV and "workspace too small" in _lib.last_error()
    # the clip checks also hold for nnz == 0, where the fp32 cache-sized entry returns before it looks at anything
    tail = (None, P(0x7000), 10, 0.1, None, 1e-8, 0.05, 1, 0.0, 1, 1, 0, 0, 0, P(0x10000), 0, None)
    if src:
        assert lib.ce_bag_backward_update_src_clip(P(0x2000), 0, 10, 8, 0, P(0x3000), 0, P(0x4000), *tail) == INV
    else:
        assert lib.ce_bag_backward_update_clip(P(0x2000), 0, 10, 8, P(0x5000), 0, P(0x6000), 1, 5, 1, None, 0, 0,
                                               P(0x3000), 0, None, *tail) == INV
    assert "grad_clip must" in _lib.last_error()


def test_sorted_entry_refuses_before_anything_happens():
    _lib, lib = _entries()
    INV, UNS = _lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED
    assert _sorted(lib, wd_mode=3, clip_mode=3, act=9) == INV and "weight_decay_mode" in _lib.last_error()
    for bad in BAD_CLIP:                                               # behind the decay's, before an unknown act_dtype
        assert _sorted(lib, act=9, wdt=9, **bad) == INV and "grad_clip" in _lib.last_error()
    assert _sorted(lib, act=9) == INV and "activation" in _lib.last_error()
    assert _sorted(lib, wdt=1, rounding=1) == UNS and "STOCHASTIC" in _lib.last_error()
    assert _sorted(lib, ws_bytes=0) == INV and "workspace too small" in _lib.last_error()
    assert _sorted(lib, ws_bytes=0, opt=_lib.CE_OPT_SGD, clip=float("inf")) == INV       # fp32 SGD is taken here
    assert "workspace too small" in _lib.last_error()


@pytest.mark.parametrize("partial", [False, True], ids=["adam", "pradam"])
@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
def test_adam_entries_refuse_before_anything_happens(src, partial):
    _lib, lib = _entries()
    INV, UNS = _lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED
    assert _adam(lib, src, partial, step=0, acc=7, clip_mode=3) == INV and "step" in _lib.last_error()
    assert _adam(lib, src, partial, acc=7, clip_mode=3) == INV and "accumulator" in _lib.last_error()
    assert _adam(lib, src, partial, wd_mode=3, clip_mode=3) == INV and "weight_decay_mode" in _lib.last_error()
    for bad in BAD_CLIP:
        for later in (dict(beta1=1.5), dict(dim=6), dict(ws_bytes=0)):
            assert _adam(lib, src, partial, **bad, **later) == INV and "grad_clip" in _lib.last_error(), (bad, later)
    assert _adam(lib, src, partial, clip_mode=3, clip=-1.0) == INV and "grad_clip_mode" in _lib.last_error()
    assert _adam(lib, src, partial, beta1=1.5) == INV and "beta" in _lib.last_error()
    assert _adam(lib, src, partial, dim=6) == UNS
    if partial:
        assert _adam(lib, src, partial, v=0) == INV and "second moment" in _lib.last_error()
    assert _adam(lib, src, partial, ws_bytes=0, clip=float("inf")) == INV and "workspace too small" in _lib.last_error()


# ---- the Python surface ---------------------------------------------------------------------------------------------

def test_python_keywords_and_refusals_without_a_device():
    from cachedembedding_amd import functional as Fn
    from cachedembedding_amd.cached_embedding import CachedEmbeddingBag
    from cachedembedding_amd.parallel import RowwiseShardedEmbeddingBag
    assert Fn.GRAD_CLIP_MODES == ("value", "row_norm")
    assert Fn.check_grad_clip(None, "value") is None and Fn.check_grad_clip(0.5, "row_norm") == 0.5
    assert Fn.check_grad_clip(float("inf"), "value") == float("inf")
    for bad in (0.0, -0.1, float("nan"), torch.ones(1)):
        with pytest.raises(ValueError, match="grad_clip"):
            Fn.check_grad_clip(bad, "value")
    with pytest.raises(ValueError, match="grad_clip_mode"):
        Fn.check_grad_clip(None, "norm")
    for cls in (Fn.FusedSGD, Fn.FusedRowwiseAdagrad, Fn.FusedAdam):
        f = cls(0.1)
        assert f.grad_clip is None and f.grad_clip_mode == "value"
        f = cls(0.1, deterministic=cls is Fn.FusedSGD, grad_clip=0.05, grad_clip_mode="row_norm")
        assert f.grad_clip == 0.05 and f.grad_clip_mode == "row_norm"
        assert f.clip_args() == (0.05, 2)
        with pytest.raises(ValueError, match="grad_clip_mode"):
            cls(0.1, grad_clip=0.1, grad_clip_mode="global")
        for bad in (0.0, -0.1, float("nan"), torch.ones(1)):
            with pytest.raises(ValueError, match="grad_clip"):
                cls(0.1, grad_clip=bad)
    f = Fn.FusedAdam(0.1, layout="partial_rowwise_adam", grad_clip=2.0)
    assert f.grad_clip == 2.0
    f.set((0.9, 0.99), 1e-8, "cache", grad_clip=0.2, grad_clip_mode="row_norm")
    assert (f.grad_clip, f.grad_clip_mode) == (0.2, "row_norm")
    f.set((0.9, 0.99), 1e-8, "cache")
    assert f.grad_clip is None
    with pytest.raises(ValueError):
        f.set((0.9, 0.99), 1e-8, "cache", grad_clip=-1.0)
    # what the paths do not take
    with pytest.raises(NotImplementedError, match=r"no per-row pass[\s\S]*deterministic=True"):
        Fn.check_grad_clip_path("sgd", torch.float32, 0.1)
    Fn.check_grad_clip_path("sgd", torch.float32, 0.1, deterministic=True)
    Fn.check_grad_clip_path("sgd", torch.bfloat16, 0.1)
    Fn.check_grad_clip_path("sgd", torch.float32, None, mode="max")
    for opt in ("sgd", "rowwise_adagrad"):
        with pytest.raises(NotImplementedError, match="mode='max'"):
            Fn.check_grad_clip_path(opt, torch.bfloat16, 0.1, mode="max")
        with pytest.raises(NotImplementedError, match="tensor learning rate"):
            Fn.check_grad_clip_path(opt, torch.bfloat16, 0.1, True, torch.zeros(1))
    # embedding_bag asks again, before any kernel (a CPU weight never reaches one)
    w = torch.zeros(4, 8, requires_grad=True)
    ids, off = torch.arange(4), torch.arange(5)
    f = Fn.FusedSGD(0.1, deterministic=True, grad_clip=0.1)
    f.deterministic = False                                            # (set after the switch was built)
    with pytest.raises(NotImplementedError, match="deterministic=True"):
        Fn.embedding_bag(ids, w, off, mode="sum", include_last_offset=True, fused_sgd=f)
    with pytest.raises(NotImplementedError, match="mode='max'"):
        Fn.embedding_bag(ids, w, off, mode="max", include_last_offset=True,
                         fused_sgd=Fn.FusedSGD(0.1, deterministic=True, grad_clip=0.1))
    Fn.FusedSGD(0.1, grad_clip=0.1)                                    # (no table yet: a 16-bit one would take it)
    # the module's setters (on a stub: no device), the sharded and table-wise modules
    mgr = types.SimpleNamespace(momentum1=torch.zeros(4), cached_idx_map=None, num_embeddings=4, device="cpu")

    def stub(fused_optimizer=None, mode="sum", **kw):
        return types.SimpleNamespace(mode=mode, table_dtype=torch.float32, weight_rounding="stochastic",
                                     fused_sgd=Fn.FusedSGD(), fused_adagrad=Fn.FusedRowwiseAdagrad(),
                                     fused_adam=Fn.FusedAdam(), fused_optimizer=fused_optimizer, cache_weight_mgr=mgr,
                                     **kw)
    s = stub()
    with pytest.raises(NotImplementedError, match="deterministic=True"):
        CachedEmbeddingBag.set_fused_sgd(s, 0.1, grad_clip=0.1)
    assert s.fused_sgd.lr is None and s.fused_sgd.grad_clip is None
    CachedEmbeddingBag.set_fused_sgd(s, 0.1, deterministic=True, grad_clip=0.1, grad_clip_mode="row_norm")
    assert (s.fused_sgd.grad_clip, s.fused_sgd.grad_clip_mode) == (0.1, "row_norm")
    CachedEmbeddingBag.set_fused_sgd(s, None)
    assert s.fused_sgd.grad_clip is None
    CachedEmbeddingBag.set_fused_rowwise_adagrad(s, 0.1, grad_clip=0.3)
    assert (s.fused_adagrad.grad_clip, s.fused_adagrad.grad_clip_mode) == (0.3, "value")
    with pytest.raises(ValueError):
        CachedEmbeddingBag.set_fused_rowwise_adagrad(s, 0.1, grad_clip=0.3, grad_clip_mode="cowclip")
    with pytest.raises(ValueError):
        CachedEmbeddingBag.set_fused_rowwise_adagrad(s, 0.1, grad_clip=0.0)
    assert s.fused_adagrad.grad_clip == 0.3                            # a refused call changes nothing
    mx = stub(mode="max")
    with pytest.raises(NotImplementedError, match="mode='max'"):
        CachedEmbeddingBag.set_fused_rowwise_adagrad(mx, 0.1, grad_clip=0.3)
    a = stub(fused_optimizer="adam")
    CachedEmbeddingBag.set_fused_adam(a, 0.1, grad_clip=0.5, grad_clip_mode="row_norm")
    assert (a.fused_adam.grad_clip, a.fused_adam.grad_clip_mode) == (0.5, "row_norm")
    with pytest.raises(ValueError, match="grad_clip"):
        CachedEmbeddingBag.set_fused_adam(a, 0.1, grad_clip=torch.ones(1))
    with pytest.raises(TypeError):
        CachedEmbeddingBag.set_fused_adam(a, 0.1, (0.9, 0.999), 1e-8, "step", False, 0.0, "l2", 0.5)   # keyword-only
    for name in ("ParallelCachedEmbeddingBag", "ParallelCachedEmbeddingBagTablewise"):
        s = stub(_no_weight_decay=name)
        for call in (lambda: CachedEmbeddingBag.set_fused_sgd(s, 0.1, deterministic=True, grad_clip=0.1),
                     lambda: CachedEmbeddingBag.set_fused_rowwise_adagrad(s, 0.1, grad_clip=0.1)):
            with pytest.raises(NotImplementedError, match="ce_rows_axpy"):
                call()
        CachedEmbeddingBag.set_fused_rowwise_adagrad(s, 0.1)
    shard = types.SimpleNamespace(_lr=[None])
    with pytest.raises(NotImplementedError, match="ce_rows_axpy"):
        RowwiseShardedEmbeddingBag.set_fused_sgd(shard, 0.1, grad_clip=0.1)
    with pytest.raises(NotImplementedError, match="ce_rows_axpy"):
        RowwiseShardedEmbeddingBag.set_fused_rowwise_adagrad(shard, None, grad_clip=0.1)
    assert shard._lr == [None]
    RowwiseShardedEmbeddingBag.set_fused_sgd(shard, 0.1)


def test_example_parses_the_flags_and_refuses_what_it_must():
    sys.path.insert(0, str(HERE.parent / "examples"))
    dm = importlib.import_module("dlrm_main")
    a = dm.parse_args(["--use_cache", "--adagrad"])
    assert a.embed_grad_clip is None and a.embed_grad_clip_mode == "value"
    assert dm._clip(a) == {"grad_clip": None, "grad_clip_mode": "value"}
    a = dm.parse_args(["--use_cache", "--adam", "--embed_grad_clip", "0.5", "--embed_grad_clip_mode", "row_norm"])
    assert dm._clip(a) == {"grad_clip": 0.5, "grad_clip_mode": "row_norm"}
    with pytest.raises(SystemExit):
        dm.parse_args(["--embed_grad_clip_mode", "global"])
    with pytest.raises(ValueError, match="--adagrad, --adam or"):
        dm.main(["--use_cache", "--embed_grad_clip", "0.5"])
    for bad in ("-1", "0", "nan"):
        with pytest.raises(ValueError, match="grad_clip"):
            dm.main(["--use_cache", "--adagrad", "--embed_grad_clip", bad])
    with pytest.raises(NotImplementedError, match="no per-row"):
        dm.main(["--use_cache", "--fused_sgd", "--embed_grad_clip", "0.5"])
    for argv in (["--adagrad"], ["--adam"], ["--adagrad", "--adagrad_deterministic"], ["--fused_sgd", "--table_dtype", "bf16"]):
        dm.check_embed_grad_clip(dm.parse_args(["--use_cache", "--embed_grad_clip", "0.5"] + argv))
