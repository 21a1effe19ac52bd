"""GPU tests of gradient clipping in the fused updates: the seven ce_*_clip entries against the fp64
model (tests/grad_clip_ref.py) on the workload of tests/weight_decay_ref.py, 16-bit tables, the rows that must keep their
bits, CE_CLIP_NONE and grad_clip = +inf against the covered entries, the three folds against each other, stochastic
rounding, the module over a cache that evicts at every step, a prefetch window with source-row keys, a captured step
replayed at two rates, and the refusals that need a device.

Largest |err| - rtol |ref| seen on an MI355X against the fp64 model, over every case of this file: see DESIGN.md 3.14
(every run prints its own figures)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import adam_cases as cases  # noqa: E402
import grad_clip_ref as ref  # noqa: E402
import stochastic_update_ref as sref  # noqa: E402
import table_dtype_ref as tref  # noqa: E402
import weight_decay_ref as wref  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6           # the project's own; test_grad_clip_cpu.py shows that fp32 runs keep it on this workload
LR, WD, EPS, BETAS = wref.LR, wref.WD, wref.EPS, wref.BETAS
NNZ, HOT = wref.NNZ, wref.HOT
DIMS = [4, 100, 128, 260, 1024]   # one lane | a masked last chunk | the bench shape | two chunks per lane, masked | 4 x 64
DIMS3 = [4, 128, 260]
DIMS16 = [8, 128, 264]
ROWS = [70, 4100]                 # across a 64-position wave | across a CE_COMPACT_BLOCK
CLIPS = list(ref.MODES)


def _L():
    from cachedembedding_amd import _lib as L
    return L


def _wd_code(mode):
    L = _L()
    return {"l2": L.CE_WD_L2, "decoupled": L.CE_WD_DECOUPLED, None: L.CE_WD_NONE}[mode]


def _clip_code(mode):
    L = _L()
    return {"value": L.CE_CLIP_VALUE, "row_norm": L.CE_CLIP_ROW_NORM, None: L.CE_CLIP_NONE}[mode]


def _device_step(s, R, src):
    """the lookups of one step on the device: (slot arguments behind dim, or the source-row key arguments), what to keep"""
    from cachedembedding_amd.functional import presort_window
    L = _L()
    ptr = L.ptr
    idx = torch.from_numpy(s["ids"]).cuda()
    off = torch.from_numpy(s["off"]).cuda()
    if s["off32"]:
        off = off.to(torch.int32)
    go = torch.from_numpy(s["go"]).cuda()
    if s["bf16"]:
        go = go.to(torch.bfloat16)
    act = L.ACT_DTYPES[go.dtype]
    psw = None if s["psw"] is None else torch.from_numpy(s["psw"]).cuda()
    keep = [idx, off, go, psw]
    if src:
        keys = presort_window(idx.view(1, -1), R, offsets=off, include_last_offset=True, hook_features=s["hook"])[0]
        keep.append(keys)
        return (NNZ, ptr(go), act, ptr(keys.keys)), keep
    return (ptr(idx), NNZ, ptr(off), int(off.dtype == torch.int64), off.numel() - 1, 1, ptr(psw),
            L.CE_MODE_MEAN if s["mode"] == "mean" else L.CE_MODE_SUM, s["hook"], ptr(go), act), keep


def _run_update(W0, steps, src, path, opt, clip, clip_mode, wd=0.0, wd_mode=None, entry="clip", rounding="nearest",
                seed=0, each=None):
    """`steps` through one update entry on the table W0 (a CPU tensor of the table's dtype).  path: "cache" / "step" /
    "sorted"; opt: "adagrad" / "sgd"; entry: "clip" (the new entries) or "wd" (the entries they cover).
    each(k, w, mom): called after every step with host copies.  Returns (w, mom) on the host."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    R, D = W0.shape
    w = W0.clone().cuda()
    wdt = L.ACT_DTYPES[w.dtype]
    w16 = wdt != L.CE_ACT_F32
    ada = opt == "adagrad"
    mom = torch.zeros(R, device="cuda") if ada else None
    code = L.CE_OPT_ROWWISE_ADAGRAD if ada else L.CE_OPT_SGD
    rnd = L.CE_ROUND_STOCHASTIC if rounding == "stochastic" else L.CE_ROUND_NEAREST
    if path == "sorted":
        ws = torch.empty(lib.ce_bag_backward_update_sorted_workspace(R, NNZ, D), dtype=torch.uint8, device="cuda")
    elif path == "step":
        ws = torch.zeros(lib.ce_bag_backward_update_compact_workspace(R, NNZ, D), dtype=torch.uint8, device="cuda")
    else:
        need = lib.ce_bag_backward_w16_workspace(R, D) if w16 else lib.ce_bag_backward_rowwise_adagrad_workspace(R, D)
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    acc = L.CE_ACC_STEP if path == "step" else L.CE_ACC_CACHE
    state = (None, ptr(mom), R if ada else 0)
    end = (ptr(ws), ws.numel(), L.stream_ptr())
    decay = (float(wd), _wd_code(wd_mode))
    if entry == "clip":
        decay += (float(clip), _clip_code(clip_mode))
    for k, s in enumerate(steps):
        look, keep = _device_step(s, R, src)
        table = (ptr(w), wdt, R, D)
        if path == "sorted":
            assert not src
            fn = lib.ce_bag_backward_update_sorted_clip if entry == "clip" else lib.ce_bag_backward_update_sorted_wd
            L.check(fn(*table, *look, *state, LR, EPS, *decay, code, rnd, seed, *end))
        else:
            if entry == "clip":
                fn = lib.ce_bag_backward_update_src_clip if src else lib.ce_bag_backward_update_clip
            else:
                fn = lib.ce_bag_backward_update_src_wd if src else lib.ce_bag_backward_update_wd
            L.check(fn(*table, *look, *(() if src else (None,)), *state, LR, None, EPS, *decay, code, rnd, seed, acc, *end))
        if each is not None:
            torch.cuda.synchronize()
            each(k, w.cpu(), None if mom is None else mom.cpu())
        del keep
    torch.cuda.synchronize()
    if path == "cache" and not w16:
        assert not ws.any()                                          # the workspace is left zero-filled
    return w.cpu(), (None if mom is None else mom.cpu())


def _run_adam(W0, steps, src, path, clip, clip_mode, wd=0.0, wd_mode=None, entry="clip", v0=0.0, partial=False):
    """Adam (rows w | m | v) or partial row-wise Adam (rows w | m, v [R]) through the _clip entries or the entries they
    cover.  Returns (w, m, v) as numpy."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    R, D = W0.shape
    span = 2 if partial else 3
    t = torch.zeros(R, span * D, dtype=torch.float32)
    t[:, :D] = torch.from_numpy(W0)
    if not partial:
        t[:, 2 * D:] = v0
    w = t.cuda()
    v = torch.zeros(R, device="cuda") if partial else None
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    code = L.CE_ACC_STEP if path == "step" else L.CE_ACC_CACHE
    ws = torch.zeros(lib.ce_bag_backward_adam_workspace(R, NNZ, D, code), dtype=torch.uint8, device="cuda")
    name = "ce_bag_backward_" + ("pradam" if partial else "adam") + ("_src" if src else "")
    if entry == "clip":
        name += "_clip"
    elif not partial:
        name += "_wd"
    fn = getattr(lib, name)
    for s in steps:
        look, keep = _device_step(s, R, src)
        tail = (BETAS[0], BETAS[1], LR, None, EPS, float(wd), _wd_code(wd_mode))
        if entry == "clip":
            tail += (float(clip), _clip_code(clip_mode))
        tail += (ptr(step), code, ptr(ws), ws.numel(), L.stream_ptr())
        if partial:
            tail = (None, ptr(v), R) + tail
        L.check(fn(ptr(w), R, D, *look, *(() if src else (None,)), *tail))
        del keep
    torch.cuda.synchronize()
    assert int(step.item()) == len(steps)
    out = w.cpu().numpy()
    return out[:, :D], out[:, D:2 * D], (v.cpu().numpy() if partial else out[:, 2 * D:])


def _case(R, D, src):
    rng = np.random.default_rng(100 * D + R)
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    return W0, wref.steps(R, D, src, seed=D + R)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _close(what, got, want):
    err = np.abs(got - want) - RTOL * np.abs(want)
    print(f"{what}: max (|err| - rtol |ref|) = {err.max():.3g}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)


def _check_update(what, W0, got, model, opt):
    """a (w, momentum) result against the model's (W, M, named), and the rows that keep their bits"""
    W, M, named = model
    R = len(W0)
    assert not named[R - 5:].any() and named[R - 20:R - 5].any() and named[HOT]
    w = got[0].numpy()
    _close(what + " w", w, W)
    # rows no covered lookup names -- row R - 1 of step 0's uncovered tail among them -- keep their bits
    np.testing.assert_array_equal(_bits(w[~named]), _bits(W0[~named]), err_msg=what)
    assert not np.array_equal(w[named], W0[named])
    if opt == "adagrad":
        m = got[1].numpy()
        _close(what + " momentum", m, M)
        assert not m[~named].any(), what


def _check_adam(what, W0, got, model, v0=0.0):
    W, M, V, named = model
    w, m, v = got
    for name, g, want in (("w", w, W), ("m", m, M), ("v", v, V)):
        _close(f"{what} {name}", g, want)
    np.testing.assert_array_equal(_bits(w[~named]), _bits(W0[~named]), err_msg=what)
    assert not m[~named].any() and (v[~named] == np.float32(v0)).all(), what


# ---- 1, 2: every entry against the fp64 model; the rows that keep their bits -----------------------------------------

@pytest.mark.parametrize("clip_mode", CLIPS)
@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("D", DIMS)
def test_adagrad_cache_sized_against_the_fp64_model(D, R, src, clip_mode):
    W0, steps = _case(R, D, src)
    c = ref.threshold(clip_mode, D)
    stats = {}
    model = ref.run_model("adagrad", W0, steps, clip_mode, stats=stats)
    assert stats["clipped"] > 0 and stats["kept"] > 0
    got = _run_update(torch.from_numpy(W0), steps, src, "cache", "adagrad", c, clip_mode)
    _check_update(f"adagrad {clip_mode} D={D} R={R} {'src' if src else 'slots'} cache", W0, got, model, "adagrad")
    if D == 128 and R == 70:                          # the clip is in it: the unclipped model ends elsewhere
        plain = ref.run_model("adagrad", W0, steps, clip_mode, grad_clip=None)
        assert np.abs(got[0].numpy() - plain[0]).max() > 100 * ATOL


@pytest.mark.parametrize("clip_mode", CLIPS)
@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
@pytest.mark.parametrize("D", DIMS3)
def test_step_sized_and_sorted_adagrad_against_the_fp64_model(D, src, clip_mode):
    R = 70
    W0, steps = _case(R, D, src)
    c = ref.threshold(clip_mode, D)
    model = ref.run_model("adagrad", W0, steps, clip_mode)
    for path in ("step",) + (() if src else ("sorted",)):
        got = _run_update(torch.from_numpy(W0), steps, src, path, "adagrad", c, clip_mode)
        _check_update(f"adagrad {clip_mode} D={D} {'src' if src else 'slots'} {path}", W0, got, model, "adagrad")


@pytest.mark.parametrize("partial", [False, True], ids=["adam", "pradam"])
@pytest.mark.parametrize("clip_mode", CLIPS)
@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
@pytest.mark.parametrize("D", DIMS3)
def test_adam_entries_against_the_fp64_model(D, src, clip_mode, partial):
    R = 70
    W0, steps = _case(R, D, src)
    c = ref.threshold(clip_mode, D)
    opt = "pradam" if partial else "adam"
    model = ref.run_model(opt, W0, steps, clip_mode)
    once = np.arange(R - 20, R - 5)
    got = {}
    for path in ("cache", "step"):
        got[path] = _run_adam(W0, steps, src, path, c, clip_mode, partial=partial)
        _check_adam(f"{opt} {clip_mode} D={D} {'src' if src else 'slots'} {path}", W0, got[path], model)
    for a, b in zip(got["cache"], got["step"]):       # rows looked up at most once per step: both accumulators, same bits
        np.testing.assert_array_equal(_bits(a[once]), _bits(b[once]))


@pytest.mark.parametrize("clip_mode", CLIPS)
@pytest.mark.parametrize("D", DIMS3)
def test_sorted_sgd_on_an_fp32_table_against_the_fp64_model(D, clip_mode):
    R = 70
    W0, steps = _case(R, D, False)
    model = ref.run_model("sgd", W0, steps, clip_mode)
    got = _run_update(torch.from_numpy(W0), steps, False, "sorted", "sgd", ref.threshold(clip_mode, D), clip_mode)
    _check_update(f"sorted sgd {clip_mode} D={D}", W0, got, model, "sgd")


@pytest.mark.parametrize("opt", ["adagrad", "sgd", "adam", "pradam"])
@pytest.mark.parametrize("clip_mode,wd_mode", [("row_norm", "l2"), ("value", "decoupled")])
def test_clip_in_front_of_the_decay_against_the_fp64_model(clip_mode, wd_mode, opt):
    """the clipped g feeds the L2 term; the decoupled factor scales the row the clipped step starts from"""
    R, D = 70, 128
    W0, steps = _case(R, D, False)
    c = ref.threshold(clip_mode, D)
    model = ref.run_model(opt, W0, steps, clip_mode, wd=WD, wd_mode=wd_mode)
    what = f"{opt} {clip_mode} + {wd_mode}"
    if opt in ("adam", "pradam"):
        v0 = wref.adam_v0(wd_mode, WD) if opt == "adam" else 0.0       # "l2": g + wd w can cancel to the size of eps (3.11)
        for path in ("cache", "step"):
            got = _run_adam(W0, steps, False, path, c, clip_mode, WD, wd_mode, v0=v0, partial=opt == "pradam")
            _check_adam(f"{what} {path}", W0, got, model, v0)
        return
    for path in ("sorted",) if opt == "sgd" else ("cache", "step", "sorted"):
        got = _run_update(torch.from_numpy(W0), steps, False, path, opt, c, clip_mode, WD, wd_mode)
        _check_update(f"{what} {path}", W0, got, model, opt)
    other = ref.run_model(opt, W0, steps, clip_mode, wd=0.0)
    assert np.abs(other[0] - model[0]).max() > 100 * ATOL              # the decay is in it


# ---- 1: 16-bit tables ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clip_mode", CLIPS)
@pytest.mark.parametrize("opt", ["adagrad", "sgd"])
@pytest.mark.parametrize("wt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", DIMS16)
def test_16bit_tables_round_once_per_row_and_step(D, wt, opt, clip_mode):
    """the rule of test_gpu_table_dtype.py::test_update_nearest: after every step, against the fp64 update of the 16-bit
    row the step started from, |float(W16) - x64| <= u |x64| + (1 + u) E, E the project's fp32 tolerance of x"""
    R = 70
    W0, steps = _case(R, D, False)
    c = ref.threshold(clip_mode, D)
    T0 = torch.from_numpy(W0).to(wt)
    folds = [ref.lookup_grads(s["ids"], s["off"], s["go"], R, mode=s["mode"], psw=s["psw"], hook_features=s["hook"])
             for s in steps]
    once = np.arange(R - 20, R - 5)
    final = {}
    for path in ("cache", "step", "sorted"):
        cur = {"w": T0.clone(), "m": np.zeros(R)}

        def each(k, w, m):
            rows, grads = folds[k]
            x = cur["w"].float().numpy().astype(np.float64)
            M = cur["m"].copy()
            if opt == "adagrad":
                ref.step_adagrad(x, M, rows, grads, LR, EPS, grad_clip=c, clip_mode=clip_mode)
                np.testing.assert_allclose(m.numpy(), M, rtol=RTOL, atol=ATOL, err_msg=f"{path} step {k}")
                cur["m"] = m.numpy().astype(np.float64)
            else:
                ref.step_sgd(x, rows, grads, LR, grad_clip=c, clip_mode=clip_mode)
            lim = tref.update_bound(x, RTOL * np.abs(x) + ATOL, wt)
            err = np.abs(w.double().numpy() - x)
            bad = np.nonzero(err > lim)
            assert bad[0].size == 0, (path, k, bad[0][:5], err[bad][:5], lim[bad][:5])
            untouched = np.setdiff1d(np.arange(R), rows)
            assert torch.equal(w[untouched].view(torch.int16), cur["w"][untouched].view(torch.int16)), (path, k)
            cur["w"] = w.clone()
        final[path] = _run_update(T0, steps, False, path, opt, c, clip_mode, each=each)[0]
    for path in ("step", "sorted"):
        assert torch.equal(final[path][once].view(torch.int16), final["cache"][once].view(torch.int16)), path
    assert not torch.equal(final["cache"][once], T0[once])


# ---- 3: CE_CLIP_NONE is the covered entry ----------------------------------------------------------------------------

@pytest.mark.parametrize("wd,wd_mode", [(0.0, None), (WD, "l2"), (WD, "decoupled")])
@pytest.mark.parametrize("wt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_clip_none_writes_the_bits_of_the_covered_entries(wt, wd, wd_mode):
    """the host picks the covered entry's kernels whenever the mode is CE_CLIP_NONE, whatever the threshold (also one a
    real mode would refuse).  Sorted: whole tables.  Atomic: the rows looked up at most once per step and the rows never
    named bit for bit -- the others depend on the order of atomics -- and the rest within the tolerance."""
    R, D = 4100, 128
    quiet = np.arange(R - 20, R)
    for src in (False, True):
        W0, steps = _case(R, D, src)
        T0 = torch.from_numpy(W0).to(wt)
        for opt in ("adagrad",) + (("sgd",) if wt != torch.float32 else ()):
            for path in ("cache", "step") + (() if src else ("sorted",)):
                new = _run_update(T0, steps, src, path, opt, -1.0 if src else float("nan"), None, wd, wd_mode)
                old = _run_update(T0, steps, src, path, opt, 0.0, None, wd, wd_mode, entry="wd")
                rows = slice(None) if path == "sorted" else quiet
                assert torch.equal(new[0][rows].view(torch.int16), old[0][rows].view(torch.int16)), (src, opt, path)
                if opt == "adagrad":
                    assert torch.equal(new[1][rows].view(torch.int32), old[1][rows].view(torch.int32)), (src, opt, path)
                assert not torch.equal(new[0][quiet], T0[quiet])
                if wt == torch.float32:
                    np.testing.assert_allclose(new[0].numpy(), old[0].numpy(), rtol=RTOL, atol=ATOL)
        if wt == torch.float32:
            for partial in (False, True):
                if partial and wd_mode is None:
                    wdm = "l2"                         # (the pradam entry takes CE_WD_NONE too; both ways are one call)
                else:
                    wdm = wd_mode
                for path in ("cache", "step"):
                    new = _run_adam(W0, steps, src, path, -1.0, None, wd, wdm, v0=0.01, partial=partial)
                    old = _run_adam(W0, steps, src, path, 0.0, None, wd, wdm, entry="wd", v0=0.01, partial=partial)
                    for a, b in zip(new, old):
                        np.testing.assert_array_equal(_bits(a[quiet]), _bits(b[quiet]))
                        np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)
    if wt == torch.float32:                            # fp32 SGD: the sorted entries, whole tables
        W0, steps = _case(70, 100, False)
        new = _run_update(torch.from_numpy(W0), steps, False, "sorted", "sgd", 0.0, None, wd, wd_mode)
        old = _run_update(torch.from_numpy(W0), steps, False, "sorted", "sgd", 0.0, None, wd, wd_mode, entry="wd")
        assert torch.equal(new[0].view(torch.int32), old[0].view(torch.int32))


# ---- 4: grad_clip = +inf changes nothing, through the clipped kernels -----------------------------------------------

@pytest.mark.parametrize("wd,wd_mode", [(0.0, None), (WD, "l2")])
@pytest.mark.parametrize("clip_mode", CLIPS)
def test_an_infinite_threshold_changes_nothing(clip_mode, wd, wd_mode):
    R, D = 4100, 128
    inf = float("inf")
    W0, steps = _case(R, D, False)
    quiet = np.arange(R - 20, R)
    T0 = torch.from_numpy(W0)
    for wt in (torch.float32, torch.bfloat16):         # the sorted entry: bit-equal on the whole table
        new = _run_update(T0.to(wt), steps, False, "sorted", "adagrad", inf, clip_mode, wd, wd_mode)
        old = _run_update(T0.to(wt), steps, False, "sorted", "adagrad", 0.0, None, wd, wd_mode, entry="wd")
        assert torch.equal(new[0].view(torch.int16), old[0].view(torch.int16)), wt
        assert torch.equal(new[1].view(torch.int32), old[1].view(torch.int32)), wt
    new = _run_update(T0, steps, False, "sorted", "sgd", inf, clip_mode, wd, wd_mode)
    old = _run_update(T0, steps, False, "sorted", "sgd", 0.0, None, wd, wd_mode, entry="wd")
    assert torch.equal(new[0].view(torch.int32), old[0].view(torch.int32))
    for path in ("cache", "step"):                     # Adagrad and Adam: on the rows looked up at most once
        new = _run_update(T0, steps, False, path, "adagrad", inf, clip_mode, wd, wd_mode)
        old = _run_update(T0, steps, False, path, "adagrad", 0.0, None, wd, wd_mode, entry="wd")
        assert torch.equal(new[0][quiet].view(torch.int32), old[0][quiet].view(torch.int32)), path
        assert torch.equal(new[1][quiet].view(torch.int32), old[1][quiet].view(torch.int32)), path
        np.testing.assert_allclose(new[0].numpy(), old[0].numpy(), rtol=RTOL, atol=ATOL)
        for partial in (False, True):
            wdm = "l2" if wd_mode is None else wd_mode
            new = _run_adam(W0, steps, False, path, inf, clip_mode, wd, wdm, v0=0.01, partial=partial)
            old = _run_adam(W0, steps, False, path, 0.0, None, wd, wdm, entry="wd", v0=0.01, partial=partial)
            for a, b in zip(new, old):
                np.testing.assert_array_equal(_bits(a[quiet]), _bits(b[quiet]))
                np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)


# ---- 5: the three folds agree on a row looked up once, with a clip that bites ---------------------------------------

@pytest.mark.parametrize("scale", [1.0, 0.4], ids=["workload", "tight"])
@pytest.mark.parametrize("clip_mode", CLIPS)
@pytest.mark.parametrize("wt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [128, 264])          # (264: two chunks per lane, the last one masked, and a bf16 row's 8)
def test_the_three_folds_agree_on_rows_looked_up_once(D, wt, clip_mode, scale):
    """one atomic add onto zero is exact, so a row looked up at most once per step has the same folded gradient in all
    three forms, and the clip is spelled once: same bits.  The workload's thresholds leave such rows (|g| < 0.03 per
    element) alone; the tight ones (0.4 of them) clip them, which the model confirms."""
    R = 70
    W0, steps = _case(R, D, False)
    c = scale * ref.threshold(clip_mode, D)
    once = np.arange(R - 20, R - 5)
    hit = 0
    for s in steps:
        rows, grads = ref.lookup_grads(s["ids"], s["off"], s["go"], R, mode=s["mode"], psw=s["psw"], hook_features=s["hook"])
        uniq, g = ref.adam_ref.fold(rows, grads, D)
        hit += int(ref.clipped_mask(g[np.isin(uniq, once)], c, clip_mode).sum())
    assert (hit > 0) == (scale < 1.0)
    T0 = torch.from_numpy(W0).to(wt)
    got = {path: _run_update(T0, steps, False, path, "adagrad", c, clip_mode) for path in ("cache", "step", "sorted")}
    for path in ("step", "sorted"):
        assert torch.equal(got[path][0][once].view(torch.int16), got["cache"][0][once].view(torch.int16)), path
        assert torch.equal(got[path][1][once].view(torch.int32), got["cache"][1][once].view(torch.int32)), path
    assert not torch.equal(got["cache"][0][once], T0[once])


# ---- 6: stochastic rounding ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [ref.C_VALUE, 0.02], ids=["workload", "tight"])
def test_stochastic_rounding_of_the_clipped_update(c):
    """bf16 table, row-wise Adagrad, a value clip, one step: on the rows looked up once every element that
    stochastic_update_ref.predict can decide from the CLIPPED gradient (a clamp of one fp32 gradient row is exact) is that
    value bit for bit, and the momentum is the nearest twin's.  c = 0.02 clips about half of such a row's elements
    (|g| in [0.01, 0.03)); the workload's 0.05 none."""
    wt = torch.bfloat16
    R, D, seed = 4100, 128, 11
    W0, steps = _case(R, D, False)
    T0 = torch.from_numpy(W0).to(wt)
    near, mn = _run_update(T0, steps[:1], False, "cache", "adagrad", c, "value", rounding="nearest")
    sto, ms = _run_update(T0, steps[:1], False, "cache", "adagrad", c, "value", rounding="stochastic", seed=seed)
    rows, grads = ref.lookup_grads(steps[0]["ids"], steps[0]["off"], steps[0]["go"], R, dtype=np.float32)
    cnt = np.bincount(rows, minlength=R)
    one_np = np.nonzero(cnt == 1)[0]
    one = torch.from_numpy(one_np)
    assert len(one) > 300
    g = np.zeros((R, D), np.float32)
    g[rows[cnt[rows] == 1]] = grads[cnt[rows] == 1]
    gc = ref.clip(g[one_np], c, "value", np.float32)
    assert (gc != g[one_np]).any() == (c < 0.03)
    never = torch.from_numpy(np.nonzero(cnt == 0)[0])
    assert torch.equal(sto[never].view(torch.int16), T0[never].view(torch.int16)) and not ms[never].any()
    assert torch.equal(mn.view(torch.int32)[one], ms.view(torch.int32)[one])
    ss = (gc.astype(np.float64) ** 2).sum(1) / D                     # the momentum saw the clipped gradient
    np.testing.assert_allclose(mn.numpy()[one_np], ss, rtol=RTOL, atol=0)
    bits = sref.random_bits(seed, 1, one_np, D)
    want, decided = sref.predict(T0[one], gc, mn.numpy()[one_np], LR, EPS, bits, wt)
    a = sref.bits16(sto[one])
    wrong = decided & (a != sref.bits16(want))
    assert not wrong.any(), (int(wrong.sum()), "of", int(decided.sum()), np.argwhere(wrong)[:4])
    undecided = 1.0 - float(decided.mean())
    print(f"stochastic value clip c={c}: undecided share {undecided:.5f}")
    assert undecided <= sref.CAP
    assert not torch.equal(sto[one], near[one])


# ---- 7: through the module, with a cache that evicts at every step ---------------------------------------------------

def _module_model(opt, W0, steps, clip, clip_mode, wd=0.0, wd_mode="l2", use_psw=True, stats=None):
    """the fp64 model over the HOST table"""
    W = W0.astype(np.float64)
    if opt == "adam":
        M, V = np.zeros_like(W), np.zeros_like(W)
    else:
        M = np.zeros(len(W))
    hit = kept = 0
    for t, (ids, off, go, psw) in enumerate(steps, 1):
        rows, grads = ref.lookup_grads(ids, off, go, cases.N, psw=psw if use_psw else None)
        mask = ref.clipped_mask(ref.adam_ref.fold(rows, grads, cases.D)[1], clip, clip_mode)
        hit, kept = hit + int(mask.sum()), kept + int(mask.size - mask.sum())
        if opt == "adam":
            ref.step_adam(W, M, V, rows, grads, cases.LR, t, cases.BETAS, cases.EPS, wd, wd_mode, grad_clip=clip,
                          clip_mode=clip_mode)
        else:
            ref.step_adagrad(W, M, rows, grads, cases.LR, cases.EPS, wd, wd_mode, grad_clip=clip, clip_mode=clip_mode)
    assert hit > 0 and kept > 0
    return (W, M, V) if opt == "adam" else (W, M)


def _module(W0, **kw):
    import cachedembedding_amd as ce
    return ce.CachedEmbeddingBag.from_pretrained(torch.from_numpy(W0.copy()), freeze=False, mode="sum",
                                                 include_last_offset=True, cuda_row_num=8, **kw)


def _train(emb, steps):
    for ids, off, go, psw in steps:
        out = emb(torch.from_numpy(ids).cuda(), torch.from_numpy(off).cuda(), per_sample_weights=torch.from_numpy(psw).cuda())
        out.backward(torch.from_numpy(go).cuda())
    assert sum(n > 0 for n in emb.num_write_back_history) >= len(steps) - 1, emb.num_write_back_history
    emb.flush()
    torch.cuda.synchronize()


@pytest.mark.parametrize("clip,clip_mode", [(0.5, "value"), (6.0, "row_norm")])
def test_adam_with_a_clip_through_a_cache_that_evicts_at_every_step(clip, clip_mode):
    import cachedembedding_amd as ce
    steps = cases.zipf_steps(seed=32, max_unique=6)[:6]
    W0 = cases.initial_weight()
    emb = _module(W0, evict_strategy=ce.EvictionStrategy.LFU, fused_optimizer="adam")
    emb.set_fused_adam(cases.LR, cases.BETAS, cases.EPS, grad_clip=clip, grad_clip_mode=clip_mode)
    _train(emb, steps)
    W, M, V = _module_model("adam", W0, steps, clip, clip_mode)
    for name, got, want in (("weight", emb.weight, W), ("exp_avg", emb.exp_avg, M), ("exp_avg_sq", emb.exp_avg_sq, V)):
        _close(f"module adam {clip_mode} {name}", got.numpy().astype(np.float64), want)
    # the clip is in it: torch.optim.SparseAdam over the same steps, unclipped, ends elsewhere
    assert np.abs(emb.exp_avg_sq.numpy() - cases.sparse_adam_run(W0, steps, torch.float64)[2]).max() > 100 * ATOL


@pytest.mark.parametrize("clip,clip_mode,wd_mode", [(0.5, "value", "l2"), (6.0, "row_norm", "decoupled")])
def test_adagrad_with_a_clip_and_decay_through_a_cache_that_evicts_at_every_step(clip, clip_mode, wd_mode):
    import cachedembedding_amd as ce
    steps = cases.zipf_steps(seed=31, max_unique=6)[:6]
    W0 = cases.initial_weight()
    emb = _module(W0, evict_strategy=ce.EvictionStrategy.LFU)
    emb.set_fused_rowwise_adagrad(cases.LR, eps=cases.EPS, grad_clip=clip, grad_clip_mode=clip_mode, weight_decay=WD,
                                  weight_decay_mode=wd_mode)
    _train(emb, steps)
    assert emb.cache_weight_mgr.cuda_cached_weight.grad is None
    W, M = _module_model("adagrad", W0, steps, clip, clip_mode, WD, wd_mode)
    _close(f"module adagrad {clip_mode} {wd_mode} weight", emb.weight.numpy().astype(np.float64), W)
    _close(f"module adagrad {clip_mode} {wd_mode} momentum", emb.cache_weight_mgr.momentum1.cpu().numpy().astype(np.float64), M)
    Mp = np.zeros(cases.N)                              # the clip is in it: the unclipped run's momentum is elsewhere
    Wp = W0.astype(np.float64)
    for ids, off, go, psw in steps:
        wref.step_adagrad(Wp, Mp, *ref.lookup_grads(ids, off, go, cases.N, psw=psw), cases.LR, cases.EPS, WD, wd_mode)
    assert np.abs(emb.cache_weight_mgr.momentum1.cpu().numpy() - Mp).max() > 100 * ATOL


# ---- 8: a prefetch window with source-row keys -----------------------------------------------------------------------

def test_a_prefetch_window_with_source_row_keys_gives_the_eager_result():
    import cachedembedding_amd as ce
    from cachedembedding_amd.pipeline import PrefetchWindow
    clip, clip_mode = 6.0, "row_norm"
    steps = cases.zipf_steps(seed=33, max_unique=4)[:6]
    off_np = steps[0][1]
    steps = [(ids, off_np, go[:len(off_np) - 1], psw) for ids, _, go, psw in steps]
    W0 = cases.initial_weight()
    off = torch.from_numpy(off_np).to(torch.int32).cuda()

    def module():
        emb = _module(W0, evict_strategy=ce.EvictionStrategy.LFU)
        emb.set_fused_rowwise_adagrad(cases.LR, eps=cases.EPS, accumulator="step", grad_clip=clip, grad_clip_mode=clip_mode)
        return emb

    eager = module()
    for ids, _, go, _ in steps:
        out = eager(torch.from_numpy(ids).cuda(), off)
        out.backward(torch.from_numpy(go).cuda())
    eager.flush()
    emb = module()
    emb.set_cache_op(False)
    win = PrefetchWindow(emb, 2, presort=True, bag_layout=(off, True, 0))
    for k in range(0, len(steps), 2):
        slots = win.prepare([torch.from_numpy(s[0]).cuda() for s in steps[k:k + 2]])
        for i in range(2):
            assert type(win.keys[i]).__name__ == "SrcKeys"
            out = emb(slots[i], off, presorted=win.keys[i])
            out.backward(torch.from_numpy(steps[k + i][2]).cuda())
    assert sum(emb.num_write_back_history) > 0
    emb.flush()
    torch.cuda.synchronize()
    W, M = _module_model("adagrad", W0, steps, clip, clip_mode, use_psw=False)
    _close("window weight", emb.weight.numpy().astype(np.float64), W)
    _close("window momentum", emb.cache_weight_mgr.momentum1.cpu().numpy().astype(np.float64), M)
    np.testing.assert_allclose(emb.weight.numpy(), eager.weight.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(emb.cache_weight_mgr.momentum1.cpu().numpy(), eager.cache_weight_mgr.momentum1.cpu().numpy(),
                               rtol=RTOL, atol=ATOL)


# ---- 9: a captured step with a clip and a device learning rate, replayed at two rates --------------------------------

@pytest.mark.parametrize("opt,clip_mode", [("adagrad", "value"), ("adam", "row_norm")])
def test_captured_step_with_a_clip_follows_the_rate_of_the_replay(opt, clip_mode):
    from cachedembedding_amd.functional import FusedAdam, FusedRowwiseAdagrad, embedding_bag
    rng = np.random.default_rng(9)
    R, D, n = 70, 128, 96
    lrs = [0.05, 0.2]
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    ids = np.concatenate([rng.permutation(R - 5)[:n // 2]] * 2)       # every row at most twice: the atomics cannot reorder
    idx = torch.from_numpy(ids[rng.permutation(n)].astype(np.int64)).cuda()
    off = torch.arange(0, n + 1, 2, dtype=torch.int64, device="cuda")
    go_np = rng.standard_normal((n // 2, D)).astype(np.float32)
    go = torch.from_numpy(go_np).cuda()
    c = 1.0 if clip_mode == "value" else 1.0 * np.sqrt(D)             # standard-normal gradients: both sides of it
    kw = dict(grad_clip=c, grad_clip_mode=clip_mode, weight_decay=0.5, weight_decay_mode="decoupled")

    def table():
        if opt == "adam":
            t = torch.zeros(R, 3 * D)
            t[:, :D] = torch.from_numpy(W0)
            return t.cuda()
        return torch.from_numpy(W0).cuda()

    def fused(lr):
        if opt == "adam":
            return FusedAdam(lr, step=torch.zeros(1, dtype=torch.int64, device="cuda"), **kw)
        return FusedRowwiseAdagrad(lr, momentum=torch.zeros(R, device="cuda"), **kw)

    def one_step(w, f):
        w.requires_grad_(True)
        out = embedding_bag(idx, w, off, mode="sum", include_last_offset=True, fused_sgd=f)
        out.backward(go)
        assert w.grad is None

    we, fe = table(), fused(lrs[0])
    eager = []
    for lr in lrs:
        fe.lr = lr
        one_step(we, fe)
        eager.append(we.detach().clone())
    lr_t = torch.full((1,), lrs[0], dtype=torch.float32, device="cuda")
    wg, fg = table(), fused(lr_t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_step(wg, fg)                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():                                            # back to the start
        wg.copy_(table())
        if opt == "adam":
            fg.step.zero_()
        else:
            fg.momentum.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        one_step(wg, fg)
    for k, lr in enumerate(lrs):
        lr_t.fill_(lr)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(wg.detach().view(torch.int32), eager[k].view(torch.int32)), k
    # the clip is in it: the same two eager steps without it end elsewhere
    kw.pop("grad_clip"), kw.pop("grad_clip_mode")
    wp, fp = table(), fused(lrs[0])
    for lr in lrs:
        fp.lr = lr
        one_step(wp, fp)
    assert not torch.equal(wp.detach(), eager[1])


# ---- 10: the refusals that need a device -----------------------------------------------------------------------------

def test_refusals_on_the_device_leave_the_table_alone():
    import cachedembedding_amd as ce
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD, embedding_bag
    L = _L()
    w = torch.randn(16, 8, device="cuda", requires_grad=True)
    w0 = w.detach().clone()
    ids = torch.arange(8, device="cuda")
    off = torch.arange(0, 9, 2, device="cuda")
    with pytest.raises(NotImplementedError, match="deterministic=True"):
        embedding_bag(ids, w, off, mode="sum", include_last_offset=True, fused_sgd=FusedSGD(0.1, grad_clip=0.1))
    with pytest.raises(NotImplementedError, match="mode='max'"):
        embedding_bag(ids, w, off, mode="max", include_last_offset=True,
                      fused_sgd=FusedSGD(0.1, deterministic=True, grad_clip=0.1))
    f = FusedRowwiseAdagrad(torch.full((1,), 0.1, device="cuda"), momentum=torch.zeros(16, device="cuda"), grad_clip=0.1)
    f.deterministic = True                                            # (set after the switch was built)
    with pytest.raises(NotImplementedError):
        embedding_bag(ids, w, off, mode="sum", include_last_offset=True, fused_sgd=f)
    # the C entries on real buffers: refused before a launch, in the header's order, also at nnz == 0
    mom = torch.zeros(16, device="cuda")
    ws = torch.zeros(L.lib.ce_bag_backward_rowwise_adagrad_workspace(16, 8), dtype=torch.uint8, device="cuda")
    go = torch.ones(4, 8, device="cuda")

    def update(nnz, clip, clip_mode, opt=L.CE_OPT_ROWWISE_ADAGRAD, wd_mode=L.CE_WD_NONE):
        return L.lib.ce_bag_backward_update_clip(L.ptr(w), L.CE_ACT_F32, 16, 8, L.ptr(ids), nnz, L.ptr(off), 1, 4, 1, None,
                                                 L.CE_MODE_SUM, 0, L.ptr(go), L.CE_ACT_F32, None, None, L.ptr(mom), 16, 0.1,
                                                 None, 1e-8, 0.0, wd_mode, clip, clip_mode, opt, L.CE_ROUND_NEAREST, 0,
                                                 L.CE_ACC_CACHE, L.ptr(ws), ws.numel(), L.stream_ptr())
    for nnz in (8, 0):
        assert update(nnz, 0.1, 3) == L.CE_ERR_INVALID and "grad_clip_mode" in L.last_error()
        assert update(nnz, 0.1, 3, wd_mode=7) == L.CE_ERR_INVALID and "weight_decay_mode" in L.last_error()
        for bad in (0.0, -1.0, float("nan")):
            assert update(nnz, bad, L.CE_CLIP_VALUE) == L.CE_ERR_INVALID and "grad_clip must" in L.last_error()
    assert update(8, 0.1, L.CE_CLIP_ROW_NORM, opt=L.CE_OPT_SGD) == L.CE_ERR_UNSUPPORTED and "fp32 table" in L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(w.detach(), w0) and not mom.any() and not ws.any()
    # the module's setters, before the first step
    emb = ce.CachedEmbeddingBag(64, 8, mode="sum", cuda_row_num=8)
    with pytest.raises(NotImplementedError, match="deterministic=True"):
        emb.set_fused_sgd(0.1, grad_clip=0.1)
    assert emb.fused_sgd.lr is None
    with pytest.raises(ValueError, match="grad_clip"):
        emb.set_fused_rowwise_adagrad(0.1, grad_clip=0.0)
    with pytest.raises(ValueError, match="grad_clip_mode"):
        emb.set_fused_rowwise_adagrad(0.1, grad_clip=0.1, grad_clip_mode="global")
    assert emb.fused_adagrad.lr is None
    # deterministic fp32 SGD with a clip runs through the sorted entry: every looked-up element moves by lr * c at most
    emb.set_fused_sgd(0.5, deterministic=True, grad_clip=0.25)
    before = emb.weight.clone()
    out = emb(torch.arange(6, device="cuda"), torch.arange(0, 7, 2, device="cuda"))
    out.backward(torch.full_like(out, 3.0))
    emb.flush()
    torch.cuda.synchronize()
    torch.testing.assert_close(emb.weight[:6], before[:6] - 0.125, rtol=1e-6, atol=1e-7)
    assert torch.equal(emb.weight[6:], before[6:])
    mx = ce.CachedEmbeddingBag(64, 8, mode="max", cuda_row_num=8)
    with pytest.raises(NotImplementedError, match="mode='max'"):
        mx.set_fused_sgd(0.1, deterministic=True, grad_clip=0.1)
    adam = ce.CachedEmbeddingBag(64, 8, mode="sum", cuda_row_num=8, fused_optimizer="adam")
    with pytest.raises(ValueError, match="grad_clip"):
        adam.set_fused_adam(0.1, grad_clip=-1.0)
    adam.set_fused_adam(0.1, grad_clip=float("inf"), grad_clip_mode="row_norm")
