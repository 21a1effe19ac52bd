"""GPU tests of weight decay in the fused updates: the five ce_*_wd entries against the fp64 model
(tests/weight_decay_ref.py) on the workload of tests/test_gpu_adam.py, 16-bit tables, the rows that must keep their
bits, weight_decay = 0 against the existing entries, the three folds against each other, the module over a cache that
evicts at every step, a prefetch window with source-row keys, a captured step whose decay follows the rate, and the
refusals that need a device."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import adam_cases as cases  # noqa: E402
import stochastic_update_ref as sref  # noqa: E402
import table_dtype_ref as tref  # noqa: E402
import weight_decay_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6           # the project's own (test_gpu_rowwise_adagrad.py, test_gpu_adam.py); test_weight_decay_cpu.py
LR, WD, EPS, BETAS = ref.LR, ref.WD, ref.EPS, ref.BETAS      # shows that fp32 runs keep it on this workload
NNZ, HOT = ref.NNZ, ref.HOT
DIMS = [4, 100, 128, 260, 1024]   # one lane | a masked last chunk | the bench shape | two chunks per lane, masked | 4 x 64
DIMS16 = [8, 128, 264]
ROWS = [70, 4100]                 # across a 64-position wave | across a CE_COMPACT_BLOCK
MODES = ["l2", "decoupled"]


def _L():
    from cachedembedding_amd import _lib as L
    return L


def _mode_code(mode):
    L = _L()
    return {"l2": L.CE_WD_L2, "decoupled": L.CE_WD_DECOUPLED, None: L.CE_WD_NONE}[mode]


def _device_step(s, R, src):
    """the lookups of one step on the device: (slot arguments behind dim, or the source-row key arguments), act"""
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


def _run_update(W0, steps, src, path, opt, wd, mode, entry="wd", rounding="nearest", seed=0, each=None):
    """`steps` through one update entry on the table W0 (a CPU tensor of the table's dtype).  path: "cache" / "step" /
    "sorted"; opt: "adagrad" / "sgd"; entry: "wd" (the new entries) or "old" (the entries from before the decay).
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
    decay = (float(wd), _mode_code(mode))
    for k, s in enumerate(steps):
        look, keep = _device_step(s, R, src)
        table = (ptr(w), wdt, R, D)
        if path == "sorted":
            assert not src
            if entry == "wd":
                fn, tail = lib.ce_bag_backward_update_sorted_wd, state + (LR, EPS) + decay + (code, rnd, seed) + end
            else:
                fn, tail = lib.ce_bag_backward_update_sorted, state + (LR, EPS, code, rnd, seed) + end
            L.check(fn(*table, *look, *tail))
        elif entry == "wd":
            fn = lib.ce_bag_backward_update_src_wd if src else lib.ce_bag_backward_update_wd
            tail = state + (LR, None, EPS) + decay + (code, rnd, seed, acc) + end
            L.check(fn(*table, *look, *(() if src else (None,)), *tail))
        elif path == "cache" and not w16:
            fn = lib.ce_bag_backward_rowwise_adagrad_src_act if src else lib.ce_bag_backward_rowwise_adagrad_act
            L.check(fn(ptr(w), R, D, *look, *(() if src else (None,)), *state, LR, EPS, *end))
        else:
            fn = {("cache", False): lib.ce_bag_backward_update_w16, ("cache", True): lib.ce_bag_backward_update_src_w16,
                  ("step", False): lib.ce_bag_backward_update_compact,
                  ("step", True): lib.ce_bag_backward_update_compact_src}[(path, src)]
            L.check(fn(*table, *look, *(() if src else (None,)), *state, LR, EPS, code, rnd, seed, *end))
        if each is not None:
            torch.cuda.synchronize()
            each(k, w.cpu(), None if mom is None else mom.cpu())
        del keep
    torch.cuda.synchronize()
    if path == "cache" and not w16:
        assert not ws.any()                                          # the workspace is left zero-filled
    return w.cpu(), (None if mom is None else mom.cpu())


def _adam_table(W0, v0):
    R, D = W0.shape
    t = torch.zeros(R, 3 * D, dtype=torch.float32)
    t[:, :D] = torch.from_numpy(W0)
    t[:, 2 * D:] = v0
    return t


def _run_adam(W0, steps, src, path, wd, mode, entry="wd", v0=0.0):
    L = _L()
    lib, ptr = L.lib, L.ptr
    R, D = W0.shape
    w = _adam_table(W0, v0).cuda()
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    code = L.CE_ACC_STEP if path == "step" else L.CE_ACC_CACHE
    ws = torch.zeros(lib.ce_bag_backward_adam_workspace(R, NNZ, D, code), dtype=torch.uint8, device="cuda")
    for s in steps:
        look, keep = _device_step(s, R, src)
        head = (BETAS[0], BETAS[1], LR, None, EPS)
        end = (ptr(step), code, ptr(ws), ws.numel(), L.stream_ptr())
        if entry == "wd":
            fn = lib.ce_bag_backward_adam_src_wd if src else lib.ce_bag_backward_adam_wd
            tail = head + (float(wd), _mode_code(mode)) + end
        else:
            fn = lib.ce_bag_backward_adam_src if src else lib.ce_bag_backward_adam
            tail = head + end
        L.check(fn(ptr(w), R, D, *look, *(() if src else (None,)), *tail))
        del keep
    torch.cuda.synchronize()
    assert int(step.item()) == len(steps)
    return w.cpu().numpy()


def _case(R, D, src):
    rng = np.random.default_rng(100 * D + R)
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    return W0, ref.steps(R, D, src, seed=D + R)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _report(what, got, want):
    err = np.abs(got - want) - RTOL * np.abs(want)
    print(f"{what}: max (|err| - rtol |ref|) = {err.max():.3g}")


# ---- 1, 3, 5: every entry against the fp64 model; the rows that keep their bits; the folds against each other --------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("D", DIMS)
def test_adagrad_entries_against_the_fp64_model(D, R, src, mode):
    W0, steps = _case(R, D, src)
    W, M, named = ref.run_model("adagrad", W0, steps, mode)
    assert not named[R - 5:].any() and named[R - 20:R - 5].any() and named[HOT]
    once = np.arange(R - 20, R - 5)
    got = {}
    for path in ("cache", "step") + (() if src else ("sorted",)):
        w, m = _run_update(torch.from_numpy(W0), steps, src, path, "adagrad", WD, mode)
        w, m = w.numpy(), m.numpy()
        got[path] = (w, m)
        _report(f"adagrad {mode} D={D} R={R} {'src' if src else 'slots'} {path} w", w, W)
        _report(f"adagrad {mode} D={D} R={R} {'src' if src else 'slots'} {path} momentum", m, M)
        np.testing.assert_allclose(w, W, rtol=RTOL, atol=ATOL, err_msg=path)
        np.testing.assert_allclose(m, M, rtol=RTOL, atol=ATOL, err_msg=path)
        # rows no covered lookup names -- row R - 1 of step 0's uncovered tail among them -- keep their bits
        np.testing.assert_array_equal(_bits(w[~named]), _bits(W0[~named]), err_msg=path)
        assert not m[~named].any(), path
        assert not np.array_equal(w[named], W0[named])
    # rows looked up at most once per step: one atomic add onto zero is exact, so all folds agree bit for bit
    for path in got:
        np.testing.assert_array_equal(_bits(got[path][0][once]), _bits(got["cache"][0][once]), err_msg=path)
        np.testing.assert_array_equal(_bits(got[path][1][once]), _bits(got["cache"][1][once]), err_msg=path)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("D", DIMS)
def test_adam_entries_against_the_fp64_model(D, R, src, mode):
    W0, steps = _case(R, D, src)
    v0 = ref.adam_v0(mode, WD)                     # "l2": g + wd w can cancel to the size of eps; v = 0.01 keeps sqrt(v') >= 0.09
    W, M, V, named = ref.run_model("adam", W0, steps, mode)
    once = np.arange(R - 20, R - 5)
    got = {}
    for path in ("cache", "step"):
        t = _run_adam(W0, steps, src, path, WD, mode, v0=v0)
        got[path] = t
        w, m, v = t[:, :D], t[:, D:2 * D], t[:, 2 * D:]
        for name, g, want in (("w", w, W), ("m", m, M), ("v", v, V)):
            _report(f"adam {mode} D={D} R={R} {'src' if src else 'slots'} {path} {name}", g, want)
            np.testing.assert_allclose(g, want, rtol=RTOL, atol=ATOL, err_msg=f"{path} {name}")
        np.testing.assert_array_equal(_bits(w[~named]), _bits(W0[~named]))
        assert not m[~named].any() and (v[~named] == np.float32(v0)).all()
    np.testing.assert_array_equal(_bits(got["cache"][once]), _bits(got["step"][once]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [4, 100, 128])
def test_sorted_sgd_on_an_fp32_table_against_the_fp64_model(D, mode):
    R = 70
    W0, steps = _case(R, D, False)
    W, _, named = ref.run_model("sgd", W0, steps, mode)
    w, _ = _run_update(torch.from_numpy(W0), steps, False, "sorted", "sgd", WD, mode)
    np.testing.assert_allclose(w.numpy(), W, rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(_bits(w.numpy()[~named]), _bits(W0[~named]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_deterministic_sgd_with_decay_reads_a_16bit_gradient(act, mode):
    """functional.embedding_bag on an fp32 table with output_dtype = bf16 / fp16 and FusedSGD(deterministic=True,
    weight_decay=): the backward hands the sorted entry the 16-bit gradient autograd delivers, with its own dtype code.
    Against the model over the gradients as the 16-bit tensor holds them."""
    from cachedembedding_amd.functional import FusedSGD, embedding_bag
    R, D = 70, 128
    W0, steps = _case(R, D, False)
    steps = [dict(s, go=torch.from_numpy(s["go"]).to(act).float().numpy()) for s in steps]
    W, _, named = ref.run_model("sgd", W0, steps, mode)
    w = torch.from_numpy(W0).cuda().requires_grad_(True)
    fused = FusedSGD(LR, deterministic=True, weight_decay=WD, weight_decay_mode=mode)
    for s in steps:
        off = torch.from_numpy(s["off"]).cuda()
        out = embedding_bag(torch.from_numpy(s["ids"]).cuda(), w, off.to(torch.int32) if s["off32"] else off, mode=s["mode"],
                            per_sample_weights=None if s["psw"] is None else torch.from_numpy(s["psw"]).cuda(),
                            include_last_offset=True, hook_features=s["hook"], fused_sgd=fused, output_dtype=act)
        assert out.dtype == act
        out.backward(torch.from_numpy(s["go"]).to(act).cuda())
        assert w.grad is None
    got = w.detach().cpu().numpy()
    _report(f"sorted sgd {mode} grad {act}", got, W)
    np.testing.assert_allclose(got, W, rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(_bits(got[~named]), _bits(W0[~named]))
    assert np.abs(got[named] - W0[named]).max() > 100 * ATOL


# ---- 2: 16-bit tables ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("opt", ["adagrad", "sgd"])
@pytest.mark.parametrize("wt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("D", DIMS16)
def test_16bit_tables_round_once_per_row_and_step(D, R, wt, opt, mode):
    """the rule of test_gpu_table_dtype.py::test_update_nearest: after every step, against the fp64 update of the 16-bit
    row the step started from, |float(W16) - x64| <= u |x64| + (1 + u) E, E the project's fp32 tolerance of x"""
    W0, steps = _case(R, D, False)
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
                ref.step_adagrad(x, M, rows, grads, LR, EPS, WD, mode)
                np.testing.assert_allclose(m.numpy(), M, rtol=RTOL, atol=ATOL, err_msg=f"{path} step {k}")
                cur["m"] = m.numpy().astype(np.float64)
            else:
                ref.step_sgd(x, rows, grads, LR, WD, mode)
            lim = tref.update_bound(x, RTOL * np.abs(x) + ATOL, wt)
            err = np.abs(w.double().numpy() - x)
            bad = np.nonzero(err > lim)
            assert bad[0].size == 0, (path, k, bad[0][:5], err[bad][:5], lim[bad][:5])
            untouched = np.setdiff1d(np.arange(R), rows)
            assert torch.equal(w[untouched].view(torch.int16), cur["w"][untouched].view(torch.int16)), (path, k)
            cur["w"] = w.clone()
        final[path] = _run_update(T0, steps, False, path, opt, WD, mode, each=each)[0]
    for path in ("step", "sorted"):
        assert torch.equal(final[path][once].view(torch.int16), final["cache"][once].view(torch.int16)), path
    assert not torch.equal(final["cache"][once], T0[once])


def _decayed_x(w16, g32, m32, opt, mode):
    """(x, E) in fp64 of the decayed update of rows looked up ONCE (g32 is then the gradient row itself): x as the
    kernel's fp32 operands give it, E a bound of the fp32 evaluation's error (sref.exact_x's, with the decay's terms)"""
    w = w16.double().numpy()
    g = np.asarray(g32, np.float32).astype(np.float64)
    lr, wd, eps = (float(np.float32(v)) for v in (LR, WD, EPS))
    mult = lr
    if opt == "adagrad":
        mult = lr / (np.sqrt(np.asarray(m32, np.float32).astype(np.float64).reshape(-1, 1)) + eps)
    if mode == "l2":
        h, wdec = g + wd * w, w
    else:
        h, wdec = g, w * float(np.float32(1.0 - lr * wd))
    x = wdec - h * mult
    E = sref.U24 * np.abs(x) + 6 * sref.U24 * (np.abs(g) + wd * np.abs(w)) * mult + 2 * sref.U24 * np.abs(w)
    return x, E


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("opt,path", [("sgd", "cache"), ("sgd", "step"), ("adagrad", "cache")])
@pytest.mark.parametrize("wt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_16bit_stochastic_rounding_of_the_decayed_update(wt, opt, path, mode):
    """the rule of test_gpu_stochastic_adagrad.py (stochastic_update_ref.check_step), applied to the decayed update, one
    step from the same start with "stochastic" and with "nearest" rounding, on the rows looked up once (their fp32 x
    does not depend on the order of atomics): the momentum is the nearest twin's bit for bit; every element is the
    twin's value or its neighbour; wherever x - E, x and x + E round alike with the element's 16 hash bits (seed, update
    call 1, row, element) the element IS that value; the neighbour farther from zero is taken as often as the position
    of x between its neighbours says; rows not named keep their bits; another seed draws other bits."""
    R, D, seed = 4100, 128, 11
    W0, steps = _case(R, D, False)
    T0 = torch.from_numpy(W0).to(wt)
    near, mn = _run_update(T0, steps[:1], False, path, opt, WD, mode, rounding="nearest")
    sto, ms = _run_update(T0, steps[:1], False, path, opt, WD, mode, rounding="stochastic", seed=seed)
    rows, grads = ref.lookup_grads(steps[0]["ids"], steps[0]["off"], steps[0]["go"], R, dtype=np.float32)
    cnt = np.bincount(rows, minlength=R)
    one_np = np.nonzero(cnt == 1)[0]
    one = torch.from_numpy(one_np)
    assert len(one) > 300
    g = np.zeros((R, D), np.float32)
    g[rows[cnt[rows] == 1]] = grads[cnt[rows] == 1]
    never = torch.from_numpy(np.nonzero(cnt == 0)[0])
    assert torch.equal(sto[never].view(torch.int16), T0[never].view(torch.int16))
    if opt == "adagrad":
        assert torch.equal(mn.view(torch.int32)[one], ms.view(torch.int32)[one])
        assert not ms[never].any()
    a, b = sref.bits16(sto[one]), sref.bits16(near[one])
    adjacent = ((a & 0x8000) == (b & 0x8000)) & (np.abs((a & 0x7fff) - (b & 0x7fff)) <= 1)
    assert adjacent.all(), np.argwhere(~adjacent)[:4]
    x, E = _decayed_x(T0[one], g[one_np], None if mn is None else mn.numpy()[one_np], opt, mode)
    bits = sref.random_bits(seed, 1, one_np, D)
    lo, mid, hi = (sref.apply((x + sg * E).astype(np.float32), bits, wt) for sg in (-1.0, 0.0, 1.0))
    decided = (sref.bits16(lo) == sref.bits16(mid)) & (sref.bits16(mid) == sref.bits16(hi))
    wrong = decided & (a != sref.bits16(mid))
    assert not wrong.any(), (int(wrong.sum()), "of", int(decided.sum()), np.argwhere(wrong)[:4])
    undecided = 1.0 - float(decided.mean())
    print(f"{wt} {opt} {path} {mode}: undecided share {undecided:.5f}")
    assert undecided <= sref.CAP
    frac, valid = sref.frac_up(x, wt)
    _, hi_n = tref.neighbours(x.astype(np.float32), wt)
    up = (a & 0x7fff) == (sref.bits16(torch.from_numpy(hi_n).to(wt)) & 0x7fff)
    z, n = float((up[valid] - frac[valid]).sum()), float((frac[valid] * (1 - frac[valid])).sum())
    assert n > 5e3 and abs(z) / np.sqrt(n) <= 6, (z, n)
    other, _ = _run_update(T0, steps[:1], False, path, opt, WD, mode, rounding="stochastic", seed=seed + 1)
    assert not torch.equal(other[one], sto[one])


# ---- 4: weight_decay = 0 through the new entries writes the bits of the existing entries ----------------------------

@pytest.mark.parametrize("mode", MODES + [None])
@pytest.mark.parametrize("wt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_zero_decay_writes_the_bits_of_the_existing_entries(wt, mode):
    """the host picks the existing kernels whenever the decay is zero (or CE_WD_NONE with any decay).  Compared on the
    rows looked up at most once per step and the rows never named -- the others depend on the order of atomics -- and,
    for the sorted fold, over the whole table."""
    R, D = 4100, 128
    wd = 0.0 if mode is not None else 0.3
    quiet = np.arange(R - 20, R)
    for src in (False, True):
        W0, steps = _case(R, D, src)
        T0 = torch.from_numpy(W0).to(wt)
        for opt in ("adagrad",) + (("sgd",) if wt != torch.float32 else ()):
            for path in ("cache", "step") + (() if src else ("sorted",)):
                new = _run_update(T0, steps, src, path, opt, wd, mode)
                old = _run_update(T0, steps, src, path, opt, 0.0, None, entry="old")
                rows = slice(None) if path == "sorted" else quiet
                assert torch.equal(new[0][rows].view(torch.int16), old[0][rows].view(torch.int16)), (src, opt, path)
                if opt == "adagrad":
                    assert torch.equal(new[1][rows].view(torch.int32), old[1][rows].view(torch.int32)), (src, opt, path)
                assert not torch.equal(new[0][quiet], T0[quiet])
        if wt == torch.float32:
            for path in ("cache", "step"):
                new = _run_adam(W0, steps, src, path, wd, mode)
                old = _run_adam(W0, steps, src, path, 0.0, None, entry="old")
                np.testing.assert_array_equal(_bits(new[quiet]), _bits(old[quiet]))
    # fp32 SGD: the sorted entry with no decay against the existing sorted entry
    W0, steps = _case(70, 100, False)
    new = _run_update(torch.from_numpy(W0), steps, False, "sorted", "sgd", wd, mode)
    old = _run_update(torch.from_numpy(W0), steps, False, "sorted", "sgd", 0.0, None, entry="old")
    assert torch.equal(new[0].view(torch.int32), old[0].view(torch.int32))


# ---- 6: through the module, with a cache that evicts at every step ---------------------------------------------------

def _module_model(opt, W0, steps, mode, use_psw=True):
    """the fp64 model over the HOST table: a row decays exactly at its lookups, wherever it sat in between"""
    W = W0.astype(np.float64)
    if opt == "adam":
        M, V = np.zeros_like(W), np.zeros_like(W)
    else:
        M = np.zeros(len(W))
    for t, (ids, off, go, psw) in enumerate(steps, 1):
        rows, grads = ref.lookup_grads(ids, off, go, cases.N, psw=psw if use_psw else None)
        if opt == "adam":
            ref.step_adam(W, M, V, rows, grads, cases.LR, t, cases.BETAS, cases.EPS, WD, mode)
        else:
            ref.step_adagrad(W, M, rows, grads, cases.LR, cases.EPS, WD, mode)
    return (W, M, V) if opt == "adam" else (W, M)


def _lazy_adamw_on_the_cpu(W0, steps, dtype=torch.float64):
    """torch's answer to lazy decoupled Adam: torch.optim.SparseAdam over nn.EmbeddingBag(sparse=True), and before each
    of its steps the line torch.optim.AdamW decays with -- param.mul_(1 - lr * weight_decay) -- on exactly the rows of
    the step's sparse gradient.  (w, m, v) as numpy fp64."""
    bag = torch.nn.EmbeddingBag(W0.shape[0], W0.shape[1], mode="sum", sparse=True, include_last_offset=True,
                                _weight=torch.tensor(W0, dtype=dtype))
    opt = torch.optim.SparseAdam(bag.parameters(), lr=cases.LR, betas=cases.BETAS, eps=cases.EPS)
    for ids, off, go, psw in steps:
        opt.zero_grad()
        out = bag(torch.from_numpy(ids), torch.from_numpy(off), per_sample_weights=torch.tensor(psw, dtype=dtype))
        (out * torch.tensor(go, dtype=dtype)).sum().backward()
        named = bag.weight.grad.coalesce().indices()[0]
        with torch.no_grad():
            bag.weight[named] = bag.weight[named] * (1 - cases.LR * WD)
        opt.step()
    st = opt.state[bag.weight]
    return tuple(t.detach().numpy().astype(np.float64) for t in (bag.weight, st["exp_avg"], st["exp_avg_sq"]))


def _resident_rows(emb):
    """the host-table rows that sit in the cache now"""
    rows = emb.cache_weight_mgr.cached_idx_map.cpu().numpy()
    return set(int(r) for r in rows if r >= 0)


def _a_row_that_left_between_two_of_its_lookups(steps, resident_after):
    """(row, a, b, c): looked up in step a and next in step c, and NOT in the cache after step b, a <= b < c"""
    last = {}
    for c, (ids, *_) in enumerate(steps):
        for r in np.unique(ids):
            r = int(r)
            if r in last:
                a = last[r]
                for b in range(a, c):
                    if r not in resident_after[b]:
                        return r, a, b, c
            last[r] = c
    return None


def _module(W0, **kw):
    """a module over the table W0 (standard normal: the decay moves it by far more than the tolerance) with a cache
    of 8 rows"""
    import cachedembedding_amd as ce
    return ce.CachedEmbeddingBag.from_pretrained(torch.from_numpy(W0.copy()), freeze=False, mode="sum",
                                                 include_last_offset=True, cuda_row_num=8, **kw)


@pytest.mark.parametrize("strategy", ["LFU", "LRU"])
def test_adagrad_l2_through_a_cache_that_evicts_at_every_step(strategy):
    import cachedembedding_amd as ce
    steps = cases.zipf_steps(seed=31, max_unique=6)
    W0 = cases.initial_weight()
    emb = _module(W0, evict_strategy=getattr(ce.EvictionStrategy, strategy))
    emb.set_fused_rowwise_adagrad(cases.LR, eps=cases.EPS, weight_decay=WD, weight_decay_mode="l2")
    resident = []
    for ids, off, go, psw in steps:
        out = emb(torch.from_numpy(ids).cuda(), torch.from_numpy(off).cuda(), per_sample_weights=torch.from_numpy(psw).cuda())
        out.backward(torch.from_numpy(go).cuda())
        resident.append(_resident_rows(emb))
    assert emb.cache_weight_mgr.cuda_cached_weight.grad is None
    assert sum(n > 0 for n in emb.num_write_back_history) >= len(steps) - 1, emb.num_write_back_history
    emb.flush()
    torch.cuda.synchronize()
    W, M = _module_model("adagrad", W0, steps, "l2")
    np.testing.assert_allclose(emb.weight.numpy().astype(np.float64), W, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(emb.cache_weight_mgr.momentum1.cpu().numpy().astype(np.float64), M, rtol=RTOL, atol=ATOL)
    # a row evicted and readmitted between two of its lookups decayed exactly at its lookups (the model above is lazy
    # over the HOST table): such a row exists, and it is within the tolerance like the rest; the same run without decay
    # ends far outside the tolerance, so the decay is in it
    left = _a_row_that_left_between_two_of_its_lookups(steps, resident)
    assert left is not None, "no row left the cache between two of its lookups"
    np.testing.assert_allclose(emb.weight.numpy()[left[0]].astype(np.float64), W[left[0]], rtol=RTOL, atol=ATOL)
    assert np.abs(W[left[0]] - W0[left[0]]).max() > 100 * ATOL
    looked = np.zeros(cases.N, int)
    for ids, *_ in steps:
        looked[np.unique(ids)] += 1
    plain = W0.astype(np.float64)
    pm = np.zeros(cases.N)
    for ids, off, go, psw in steps:
        ref.step_adagrad(plain, pm, *ref.lookup_grads(ids, off, go, cases.N, psw=psw), cases.LR, cases.EPS)
    assert np.abs(emb.weight.numpy() - plain).max() > 100 * ATOL
    never = looked == 0
    np.testing.assert_array_equal(_bits(emb.weight.numpy()[never]), _bits(W0[never]))


def test_adam_decoupled_through_a_cache_that_evicts_at_every_step():
    import cachedembedding_amd as ce
    steps = cases.zipf_steps(seed=32, max_unique=6)
    W0 = cases.initial_weight()
    emb = _module(W0, evict_strategy=ce.EvictionStrategy.LFU, fused_optimizer="adam")
    emb.set_fused_adam(cases.LR, cases.BETAS, cases.EPS, weight_decay=WD, weight_decay_mode="decoupled")
    resident = []
    for ids, off, go, psw in steps:
        out = emb(torch.from_numpy(ids).cuda(), torch.from_numpy(off).cuda(), per_sample_weights=torch.from_numpy(psw).cuda())
        out.backward(torch.from_numpy(go).cuda())
        resident.append(_resident_rows(emb))
    assert sum(n > 0 for n in emb.num_write_back_history) >= len(steps) - 1, emb.num_write_back_history
    emb.flush()
    torch.cuda.synchronize()
    W, M, V = _module_model("adam", W0, steps, "decoupled")
    for name, got, want in (("weight", emb.weight, W), ("exp_avg", emb.exp_avg, M), ("exp_avg_sq", emb.exp_avg_sq, V)):
        np.testing.assert_allclose(got.numpy().astype(np.float64), want, rtol=RTOL, atol=ATOL, err_msg=name)
    # torch on the CPU: SparseAdam's moments and step, AdamW's decay line on exactly the rows a step names
    wt, mt, vt = _lazy_adamw_on_the_cpu(W0, steps)
    for name, got, want in (("weight", emb.weight, wt), ("exp_avg", emb.exp_avg, mt), ("exp_avg_sq", emb.exp_avg_sq, vt)):
        np.testing.assert_allclose(got.numpy().astype(np.float64), want, rtol=RTOL, atol=ATOL, err_msg="torch " + name)
    left = _a_row_that_left_between_two_of_its_lookups(steps, resident)
    assert left is not None, "no row left the cache between two of its lookups"
    np.testing.assert_allclose(emb.weight.numpy()[left[0]].astype(np.float64), wt[left[0]], rtol=RTOL, atol=ATOL)
    looked = np.zeros(cases.N, int)
    for ids, *_ in steps:
        looked[np.unique(ids[(ids >= 0) & (ids < cases.N)])] += 1
    never = looked == 0
    np.testing.assert_array_equal(_bits(emb.weight.numpy()[never]), _bits(W0[never]))
    plain, _, _ = cases.sparse_adam_run(W0, steps, torch.float64, use_psw=True)
    assert np.abs(emb.weight.numpy()[looked > 0] - plain[looked > 0]).max() > 100 * ATOL   # without decay it is elsewhere


# ---- 7: a prefetch window with source-row keys -----------------------------------------------------------------------

def test_adagrad_decay_through_a_prefetch_window_with_source_row_keys():
    import cachedembedding_amd as ce
    from cachedembedding_amd.pipeline import PrefetchWindow
    steps = cases.zipf_steps(seed=33, max_unique=4)
    off_np = steps[0][1]
    steps = [(ids, off_np, go[:len(off_np) - 1], psw) for ids, _, go, psw in steps]
    W0 = cases.initial_weight()
    emb = _module(W0, evict_strategy=ce.EvictionStrategy.LFU)
    emb.set_fused_rowwise_adagrad(cases.LR, eps=cases.EPS, accumulator="step", weight_decay=WD, weight_decay_mode="decoupled")
    emb.set_cache_op(False)
    off = torch.from_numpy(off_np).to(torch.int32).cuda()
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
    W, M = _module_model("adagrad", W0, steps, "decoupled", use_psw=False)
    np.testing.assert_allclose(emb.weight.numpy().astype(np.float64), W, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(emb.cache_weight_mgr.momentum1.cpu().numpy().astype(np.float64), M, rtol=RTOL, atol=ATOL)


# ---- 8: a captured step, replayed at two rates: the decoupled factor follows the tensor ------------------------------

@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_captured_step_decays_by_the_rate_of_the_replay(opt):
    from cachedembedding_amd.functional import FusedAdam, FusedRowwiseAdagrad, embedding_bag
    rng = np.random.default_rng(9)
    R, D, n = 70, 128, 96
    lrs = [0.05, 0.2]
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    ids = np.concatenate([rng.permutation(R - 5)[:n // 2]] * 2)       # every row at most twice: the atomics cannot reorder
    idx = torch.from_numpy(ids[rng.permutation(n)].astype(np.int64)).cuda()
    off = torch.arange(0, n + 1, 2, dtype=torch.int64, device="cuda")
    go = torch.from_numpy(rng.standard_normal((n // 2, D)).astype(np.float32)).cuda()
    kw = dict(weight_decay=0.5, weight_decay_mode="decoupled")

    def table():
        return _adam_table(W0, 0.0).cuda() if opt == "adam" else torch.from_numpy(W0).cuda()

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
    # and a replay at the first rate again would NOT have given the second table: the factor is read, not captured
    frozen = fused(lrs[0])
    wf = table()
    one_step(wf, frozen)
    one_step(wf, frozen)
    assert not torch.equal(wf.detach(), eager[1])


# ---- 9: the Python refusals that need a device ----------------------------------------------------------------------

def test_refusals_on_the_device_leave_the_table_alone():
    import cachedembedding_amd as ce
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD, embedding_bag
    w = torch.randn(16, 8, device="cuda", requires_grad=True)
    w0 = w.detach().clone()
    ids = torch.arange(8, device="cuda")
    off = torch.arange(0, 9, 2, device="cuda")
    with pytest.raises(NotImplementedError, match="deterministic=True"):
        embedding_bag(ids, w, off, mode="sum", include_last_offset=True, fused_sgd=FusedSGD(0.1, weight_decay=0.1))
    with pytest.raises(NotImplementedError, match="mode='max'"):
        embedding_bag(ids, w, off, mode="max", include_last_offset=True,
                      fused_sgd=FusedSGD(0.1, deterministic=True, weight_decay=0.1))
    f = FusedRowwiseAdagrad(torch.full((1,), 0.1, device="cuda"), momentum=torch.zeros(16, device="cuda"), weight_decay=0.1)
    f.deterministic = True                                            # (set after the switch was built)
    with pytest.raises(NotImplementedError):
        embedding_bag(ids, w, off, mode="sum", include_last_offset=True, fused_sgd=f)
    assert torch.equal(w.detach(), w0)
    emb = ce.CachedEmbeddingBag(64, 8, mode="sum", cuda_row_num=8)
    with pytest.raises(NotImplementedError, match="deterministic=True"):
        emb.set_fused_sgd(0.1, weight_decay=0.1)
    assert emb.fused_sgd.lr is None
    emb.set_fused_sgd(0.1, deterministic=True, weight_decay=0.1)
    # deterministic fp32 SGD with decay runs through the sorted entry: every looked-up row shrinks towards zero
    emb.set_fused_sgd(0.5, deterministic=True, weight_decay=1.0, weight_decay_mode="decoupled")
    before = emb.weight.clone()
    out = emb(torch.arange(6, device="cuda"), torch.arange(0, 7, 2, device="cuda"))
    out.backward(torch.zeros_like(out))
    emb.flush()
    torch.cuda.synchronize()
    torch.testing.assert_close(emb.weight[:6], before[:6] * 0.5, rtol=1e-6, atol=0)
    assert torch.equal(emb.weight[6:], before[6:])
    mx = ce.CachedEmbeddingBag(64, 8, mode="max", cuda_row_num=8)
    with pytest.raises(NotImplementedError, match="mode='max'"):
        mx.set_fused_sgd(0.1, deterministic=True, weight_decay=0.1)
