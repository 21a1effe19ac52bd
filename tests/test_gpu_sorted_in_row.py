"""GPU tests of the sorted (deterministic) fold for the in-row fused optimizers -- Adam, partial row-wise Adam, element-wise
Adagrad (ce_bag_backward_adam_sorted / _pradam_sorted / _adagrad_sorted): bit for bit against the atomic
entries where every row is looked up once, bits PREDICTED on hot runs (sorted_fold_ref.fold_sorted's gradient handed to
one CE_ACC_STEP call that names every row once), run-to-run equality from workspaces full of garbage, the ignore rules,
the step count and a captured backward, the fp64 models, the module through an evicting cache, and the C refusals."""
import gc
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import adagrad_layout_cases as ac  # noqa: E402
import adam_cases as cases  # noqa: E402
import sorted_in_row_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = sc.RTOL, sc.ATOL       # fold_sorted + the fp32 steps alone keep half of it (test_sorted_in_row_cpu.py)
WD_CODES = {None: 0, "l2": 1, "decoupled": 2}
CLIP_CODES = {None: 0, "value": 1, "row_norm": 2}
FILL = 0.25                         # what the state parts hold before the bit tests' one step


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    """the modules, graphs and streams of a test are collected and the device is idle before the next test starts: what
    a test of this file leaves in flight must surface in this file, not in whichever test comes next"""
    yield
    gc.collect()
    torch.cuda.synchronize()


def _lib():
    from cachedembedding_amd import _lib as L
    return L


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _table(layout, W0, fill=0.0):
    """[R, span D] device table with the w parts W0 and every state element `fill`"""
    n, D = W0.shape
    t = torch.full((n, sc.SPAN[layout] * D), fill, dtype=torch.float32)
    t[:, :D] = torch.from_numpy(W0)
    return t.cuda()


def _call(layout, w, D, s, ws, step, acc=None, lr_dev=None, v=None, ros=None, wd=0.0, wd_mode=None, grad_clip=None,
          clip_mode="value", lr_decay=0.0, eps=None, lr=None, **_):
    """one call for the step dict s: the sorted entry (acc None) or the atomic slots + offsets entry with accumulator
    code `acc`; returns the status"""
    L = _lib()
    lib, ptr = L.lib, L.ptr
    idx = torch.from_numpy(s["ids"]).cuda()
    off = torch.from_numpy(s["off"]).cuda()
    if s.get("off32"):
        off = off.to(torch.int32)
    go = torch.from_numpy(s["go"]).cuda().to(s.get("act", torch.float32))
    psw = None if s.get("psw") is None else torch.from_numpy(s["psw"]).cuda()
    head = (ptr(w), w.shape[0], D, ptr(idx), idx.numel(), ptr(off), int(off.dtype == torch.int64), off.numel() - 1, 1,
            ptr(psw), L.CE_MODE_MEAN if s.get("mode") == "mean" else L.CE_MODE_SUM, s.get("hook", 0), ptr(go),
            L.ACT_DTYPES[go.dtype])
    clip = grad_clip is not None
    rate = (0.0 if lr_dev is not None else float(s["lr"] if lr is None else lr), ptr(lr_dev),
            sc.eps_of(layout) if eps is None else eps, float(wd), WD_CODES[wd_mode if wd else None],
            float(grad_clip) if clip else 0.0, CLIP_CODES[clip_mode if clip else None], ptr(step))
    tail = rate + ((acc,) if acc is not None else ()) + (ptr(ws), ws.numel(), L.stream_ptr())
    keys = () if acc is None else (None,)
    if layout == "adagrad":
        fn = lib.ce_bag_backward_adagrad_sorted if acc is None else lib.ce_bag_backward_adagrad
        return fn(*head, *keys, float(lr_decay), *tail)
    if layout == "partial_rowwise_adam":
        fn = lib.ce_bag_backward_pradam_sorted if acc is None else lib.ce_bag_backward_pradam_clip
        return fn(*head, *keys, ptr(ros), ptr(v), v.numel(), *sc.BETAS, *tail)
    fn = lib.ce_bag_backward_adam_sorted if acc is None else lib.ce_bag_backward_adam_clip
    return fn(*head, *keys, *sc.BETAS, *tail)


def _sorted_ws(nnz, D, garbage=0xA5):
    """a workspace of the stated size full of garbage: nothing in it needs initialising"""
    L = _lib()
    need = L.lib.ce_bag_backward_in_row_sorted_workspace(1, nnz, D)
    assert need % 256 == 0 and need == L.lib.ce_bag_backward_in_row_sorted_workspace(1 << 20, nnz, D)
    return torch.full((need,), garbage, dtype=torch.uint8, device="cuda")


def _run(layout, W0, steps, atomic=False, lr_dev=False, fill=0.0, v_fill=0.0, v_rows=None, ros=None, garbage=0xA5, **kw):
    """(table [R, span D] numpy, v numpy or None, step count) after the steps through the sorted entries, or through
    the atomic ones with the step-sized accumulator"""
    L = _lib()
    n, D = W0.shape
    if kw.get("clip_mode") == "row_norm" and kw.get("grad_clip") is None:
        kw = dict(kw, grad_clip=ac.row_norm_threshold(D))
    w = _table(layout, W0, fill=kw.pop("init_acc", fill))
    v = None
    if layout == "partial_rowwise_adam":
        v = torch.full((n if v_rows is None else v_rows,), v_fill, dtype=torch.float32, device="cuda")
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    lr_t = torch.zeros(1, dtype=torch.float32, device="cuda") if lr_dev else None
    ros_t = None if ros is None else torch.from_numpy(ros).cuda()
    nnz = max(len(s["ids"]) for s in steps)
    if atomic:
        assert len({len(s["ids"]) for s in steps}) == 1              # (a step-sized workspace serves one nnz)
        ws = torch.zeros(L.lib.ce_bag_backward_adam_workspace(n, nnz, D, L.CE_ACC_STEP), dtype=torch.uint8, device="cuda")
    else:
        ws = _sorted_ws(nnz, D, garbage)
    for s in steps:
        if lr_dev:
            lr_t.fill_(s["lr"])
        L.check(_call(layout, w, D, s, ws, step, acc=L.CE_ACC_STEP if atomic else None, lr_dev=lr_t, v=v, ros=ros_t, **kw))
    torch.cuda.synchronize()
    return w.cpu().numpy(), None if v is None else v.cpu().numpy(), int(step.item())


def _assert_same_bits(got, want, tag):
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=f"table {tag}")
    if got[1] is not None:
        np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]), err_msg=f"v {tag}")
    assert got[2] == want[2], tag


def _once_step(rows, grads, lr):
    """every row of `rows` looked up once with its gradient row: identity bags, mode sum"""
    n = len(rows)
    return dict(ids=np.asarray(rows, np.int64), off=np.arange(n + 1, dtype=np.int64), off32=False, mode="sum", psw=None,
                hook=0, go=np.ascontiguousarray(grads, np.float32), act=torch.float32, lr=lr)


# ---- 1. rows looked up once equal the atomic path ---------------------------------------------------------------------

def _once_settings(layout, D):
    out = {"plain": dict(), "l2": dict(wd=sc.WD, wd_mode="l2"), "decoupled": dict(wd=sc.WD, wd_mode="decoupled"),
           "value_clip": dict(grad_clip=0.5, clip_mode="value"),
           # standard-normal rows have a norm near sqrt(D): about half of them are scaled
           "row_norm+l2": dict(grad_clip=float(np.sqrt(D)), clip_mode="row_norm", wd=sc.WD, wd_mode="l2")}
    if layout == "adagrad":
        out["lr_decay"] = dict(lr_decay=ac.LR_DECAY)
        out["init_acc"] = dict(init_acc=ac.INIT_ACC)
    return out


@pytest.mark.parametrize("layout", sc.LAYOUTS)
@pytest.mark.parametrize("D", ac.DIMS)
def test_rows_looked_up_once_equal_the_atomic_path_bit_for_bit(D, layout):
    steps = ac.once_steps(D, seed=D)
    W0 = ac.initial_weight(D, D + 1)
    plain = None
    for name, kw in _once_settings(layout, D).items():
        for lr_dev in (False, True):
            got = _run(layout, W0, steps, lr_dev=lr_dev, **kw)
            want = _run(layout, W0, steps, atomic=True, lr_dev=lr_dev, **kw)
            _assert_same_bits(got, want, f"D={D} {layout} {name} lr_dev={lr_dev}")
        assert got[2] == len(steps)
        t = got[0]
        # rows [ONCE_NAMED, R) are untouched, bit for bit; the named rows moved
        np.testing.assert_array_equal(_bits(t[ac.ONCE_NAMED:, :D]), _bits(W0[ac.ONCE_NAMED:]), err_msg=name)
        assert (t[ac.ONCE_NAMED:, D:] == np.float32(kw.get("init_acc", 0.0))).all(), name
        assert (t[:ac.ONCE_NAMED, :D] != W0[:ac.ONCE_NAMED]).any(axis=1).all()
        if layout == "partial_rowwise_adam":
            assert (got[1][:ac.ONCE_NAMED] > 0).all() and not got[1][ac.ONCE_NAMED:].any()
        if name == "plain":
            plain = t
        else:
            assert (t != plain).any(), name                          # the setting does something


# ---- 2. hot runs: bits predicted without a reference implementation ---------------------------------------------------

HOT_SETTINGS = {"plain": dict(), "decoupled": dict(wd=sc.WD, wd_mode="decoupled"),
                "value_clip": dict(grad_clip=0.5, clip_mode="value")}
HOT_SHAPES = [(D, torch.float32) for D in sc.DIMS] + [(128, torch.bfloat16)]


def _predicted(layout, W0, s, **kw):
    """ONE CE_ACC_STEP call in which every distinct row is looked up once with fold_sorted's gradient of it"""
    rows, grads = sc.folded(s, W0.shape[0])
    return _run(layout, W0, [_once_step(rows, grads, s["lr"])], atomic=True, **kw), rows, grads


@pytest.mark.parametrize("form", sc.HOT_FORMS)
@pytest.mark.parametrize("D,act", HOT_SHAPES, ids=[f"{D}-{'bf16' if a == torch.bfloat16 else 'fp32'}" for D, a in HOT_SHAPES])
@pytest.mark.parametrize("layout", sc.LAYOUTS)
def test_hot_runs_have_the_predicted_bits(layout, D, act, form):
    s = sc.hot_step(D, form, act=act)
    W0 = np.random.default_rng(D).standard_normal((sc.R, D)).astype(np.float32)
    for name, kw in HOT_SETTINGS.items():
        kw = dict(kw, fill=FILL, v_fill=FILL)
        got = _run(layout, W0, [s], **kw)
        want, rows, grads = _predicted(layout, W0, s, **kw)
        _assert_same_bits(got, want, f"{layout} D={D} {form} {name}")
        assert got[2] == 1 and len(rows) == len(sc.RUNS)
        others = np.setdiff1d(np.arange(sc.R), rows)
        np.testing.assert_array_equal(_bits(got[0][others, :D]), _bits(W0[others]))
        # (a run of one lookup of weight zero has g = 0: element-wise Adagrad without decay leaves such a row's bits)
        moved = rows[grads.any(axis=1)]
        assert (got[0][others, D:] == np.float32(FILL)).all() and (got[0][moved, :D] != W0[moved]).any(axis=1).all()
        assert len(moved) >= len(rows) - 1


# ---- 3. run to run -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", sc.LAYOUTS)
def test_two_runs_from_workspaces_full_of_different_garbage_agree_bit_for_bit(layout):
    D = 768
    s = sc.hot_step(D, "psw")
    W0 = np.random.default_rng(3).standard_normal((sc.R, D)).astype(np.float32)
    kw = dict(fill=FILL, v_fill=FILL, wd=sc.WD, wd_mode="l2")
    a = _run(layout, W0, [s, s], garbage=0x5A, **kw)
    b = _run(layout, W0, [s, s], garbage=0xFF, **kw)
    _assert_same_bits(a, b, layout)
    assert a[2] == 2 and not np.isnan(a[0]).any()


# ---- 4. the ignore rules -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", sc.LAYOUTS)
@pytest.mark.parametrize("D", [8, 128])
def test_ignored_and_uncovered_lookups_head_nothing(D, layout):
    R = sc.IG_R
    s = sc.ignore_step(D)
    W0 = np.random.default_rng(D + 1).standard_normal((R, D)).astype(np.float32)
    kw = dict(wd=0.1, wd_mode="decoupled")
    partial = layout == "partial_rowwise_adam"
    ros, v_rows = None, None
    if partial:
        v_rows = R + 8
        ros = (np.arange(R) + 3).astype(np.int32)                   # no identity
        ros[sc.IG_V_NEG], ros[sc.IG_V_PAST] = -1, v_rows + 2
    got = _run(layout, W0, [s], fill=FILL, v_fill=FILL, v_rows=v_rows, ros=ros, **kw)
    rows, grads = sc.folded(s, R)
    left = [sc.IG_V_NEG, sc.IG_V_PAST] if partial else []
    named = np.setdiff1d(rows, left)
    assert R - 1 in named and sc.IG_ZERO_ONLY in named and not grads[list(rows).index(sc.IG_ZERO_ONLY)].any()
    assert sc.IG_HEAD_ONLY not in rows and sc.IG_TAIL_ONLY not in rows and (s["ids"] >= R).any() and (s["ids"] < 0).any()
    # rows named only by ignored or uncovered lookups -- and the partial layout's slots without a v -- keep every part
    others = np.setdiff1d(np.arange(R), named)
    np.testing.assert_array_equal(_bits(got[0][others, :D]), _bits(W0[others]))
    assert (got[0][others, D:] == np.float32(FILL)).all() and got[2] == 1
    # the named rows: one update each, the fp32 model's (row R - 1: three covered lookups, one in front of the first bag
    # and one behind the last)
    st = sc.new_state(layout, W0, np.float32, init_acc=FILL, v_rows=v_rows)
    for k in ("M", "V"):
        if k in st:
            st[k][...] = np.float32(FILL)
    sc.model_step(layout, st, rows, grads, s["lr"], 1, np.float32, row_of=ros, **kw)
    want = np.concatenate([p for _, p in sc.parts(layout, st) if p.ndim == 2], axis=1)
    if partial:
        # (the model's sum of squares is numpy's: another order than the lane groups')
        np.testing.assert_allclose(got[0], want, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got[1], st["V"], rtol=RTOL, atol=ATOL)
        touched = np.zeros(v_rows, bool)
        touched[ros[named]] = True
        assert (got[1][~touched] == np.float32(FILL)).all() and (got[1][touched] != np.float32(FILL)).all()
    else:
        np.testing.assert_array_equal(_bits(got[0]), _bits(want))
    # a row named only by zero-weight covered lookups decays, and its moments move as the model says
    z = sc.IG_ZERO_ONLY
    assert (got[0][z, :D] != W0[z]).all()
    if layout != "adagrad":
        np.testing.assert_array_equal(got[0][z, D:2 * D], np.float32(FILL) + (np.float32(0) - np.float32(FILL)) *
                                      np.float32(1.0 - sc.BETAS[0]))
    # and the bits are the atomic entry's, given the folded gradient
    once = _once_step(rows, grads, s["lr"])
    want_atomic = _run(layout, W0, [once], atomic=True, fill=FILL, v_fill=FILL, v_rows=v_rows, ros=ros, **kw)
    _assert_same_bits(got, want_atomic, f"{layout} D={D}")


# ---- 5. the step count and a captured backward -----------------------------------------------------------------------------

@pytest.mark.parametrize("layout", sc.LAYOUTS)
def test_step_count_grows_by_one_per_call_and_an_empty_call_counts_nothing(layout):
    L = _lib()
    D = 128
    W0 = ac.initial_weight(D, 2)
    s = ac.once_steps(D, seed=2)[0]
    w = _table(layout, W0, fill=FILL)
    v = torch.full((ac.R,), FILL, device="cuda") if layout == "partial_rowwise_adam" else None
    step = torch.full((1,), 41, dtype=torch.int64, device="cuda")
    ws = _sorted_ws(len(s["ids"]), D)
    empty = dict(s, ids=np.zeros(0, np.int64), off=np.zeros(1, np.int64), go=np.zeros((1, D), np.float32))
    before = w.clone()
    L.check(_call(layout, w, D, empty, ws, step, v=v))
    no_bags = dict(s, off=np.zeros(1, np.int64), go=np.zeros((1, D), np.float32))      # lookups, and no bag
    L.check(_call(layout, w, D, no_bags, ws, step, v=v))
    torch.cuda.synchronize()
    assert int(step.item()) == 41 and torch.equal(w.view(torch.int32), before.view(torch.int32))
    for k in range(3):
        L.check(_call(layout, w, D, s, ws, step, v=v))
        torch.cuda.synchronize()
        assert int(step.item()) == 42 + k
    assert not torch.equal(w, before)


@pytest.mark.parametrize("wd_mode", [None, "decoupled"])
@pytest.mark.parametrize("layout", sc.LAYOUTS)
def test_captured_backward_replayed_equals_eager_calls(layout, wd_mode):
    """three replays equal three eager steps bit for bit, hot rows included: the step count (the bias correction;
    Adagrad's lr_decay) and a device rate rewritten between replays reach the step size and the decoupled factor"""
    from cachedembedding_amd.functional import FusedAdagrad, FusedAdam, embedding_bag
    rng = np.random.default_rng(9)
    n_rows, D, n, K = 70, 128, 384, 3
    lrs = [0.05, 0.0125, 0.2]
    W0 = rng.standard_normal((n_rows, D)).astype(np.float32)
    ids = np.minimum(rng.zipf(1.3, n) - 1, n_rows - 6)              # hot rows: runs of more than one chunk
    assert np.bincount(ids).max() > 64
    idx = torch.from_numpy(ids.astype(np.int64)).cuda()
    off = torch.arange(0, n + 1, 2, dtype=torch.int64, device="cuda")
    go = torch.from_numpy(rng.standard_normal((n // 2, D)).astype(np.float32)).cuda()
    kw = dict(weight_decay=0.1 if wd_mode else 0.0, weight_decay_mode=wd_mode or "l2", accumulator="sorted")
    vs = []

    def fused(lr):
        st = torch.zeros(1, dtype=torch.int64, device="cuda")
        if layout == "adagrad":
            return FusedAdagrad(lr, lr_decay=0.5, step=st, **kw)
        if layout == "partial_rowwise_adam":
            vs.append(torch.zeros(n_rows, device="cuda"))
            return FusedAdam(lr, step=st, layout=layout, exp_avg_sq=vs[-1], **kw)
        return FusedAdam(lr, step=st, **kw)

    def one_step(w, f):
        w.requires_grad_(True)
        out = embedding_bag(idx, w, off, mode="sum", include_last_offset=True, fused_sgd=f)
        out.backward(go)
        assert w.grad is None

    we, fe = _table(layout, W0), fused(lrs[0])
    eager, eager_v = [], []
    for lr in lrs:
        fe.lr = lr
        one_step(we, fe)
        eager.append(we.detach().clone())
        eager_v.append(vs[0].clone() if vs else None)
    # the schedule and the step count both matter to the eager run: this is what the replay has to follow
    same_rate, no_count = _table(layout, W0), _table(layout, W0)
    f1, f2 = fused(lrs[0]), fused(lrs[0])
    for lr in lrs:
        one_step(same_rate, f1)
        f2.lr = lr
        f2.step.zero_()
        one_step(no_count, f2)
    assert not torch.equal(same_rate.detach(), eager[-1]) and not torch.equal(no_count.detach(), eager[-1])

    lr_t = torch.full((1,), lrs[0], dtype=torch.float32, device="cuda")
    wg, fg = _table(layout, W0), fused(lr_t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_step(wg, fg)                                             # warm-up outside the capture: the workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():                                            # back to the start: table, v and step count
        wg.copy_(_table(layout, W0))
        fg.step.zero_()
        if vs:
            vs[-1].zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        one_step(wg, fg)
    assert int(fg.step.item()) == 0                                  # capturing runs nothing
    for k, lr in enumerate(lrs):
        lr_t.fill_(lr)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(wg.detach().view(torch.int32), eager[k].view(torch.int32)), k
        if vs:
            assert torch.equal(vs[-1].view(torch.int32), eager_v[k].view(torch.int32)), k
    assert int(fg.step.item()) == K and int(fe.step.item()) == K


# ---- 6. against the fp64 references --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,which,case", sc.SEVEN)
@pytest.mark.parametrize("D", [128, 768])
def test_seven_steps_against_the_fp64_model(D, layout, which, case):
    W0, steps, kw = sc.seven(layout, which, case, D)
    want, named = sc.model(layout, W0, steps, np.float64, **kw)
    got = _run(layout, W0, steps, lr_dev=which == "zipf", **kw)
    assert got[2] == sc.STEPS
    worst = 0.0
    for k, (name, w) in enumerate(sc.parts(layout, want)):
        g = got[1] if w.ndim == 1 else got[0][:, k * D:(k + 1) * D]
        err = float((np.abs(g - w) / (ATOL + RTOL * np.abs(w))).max())
        worst = max(worst, err)
        print(f"D={D} {layout} {which} {case} {name}: max |err| / (atol + rtol |ref|) = {err:.3g}")
        np.testing.assert_allclose(g, w, rtol=RTOL, atol=ATOL, err_msg=name)
    # rows no covered lookup names keep their bits, decay or not
    init = np.float32(kw.get("init_acc", 0.0))
    np.testing.assert_array_equal(_bits(got[0][~named, :D]), _bits(W0[~named]))
    assert (got[0][~named, D:] == init).all() and named.any() and not named.all()


# ---- 7. through the module -----------------------------------------------------------------------------------------------------

MODULE_KW = dict(weight_decay=0.01, weight_decay_mode="decoupled", accumulator="sorted")


def _module(layout, cuda_row_num, seed=77, freq=None, strategy="LFU", w=None):
    import cachedembedding_amd as ce
    return ce.CachedEmbeddingBag(cases.N, cases.D, mode="sum", include_last_offset=True, cuda_row_num=cuda_row_num,
                                 evict_strategy=getattr(ce.EvictionStrategy, strategy), fused_optimizer=layout,
                                 init_seed=seed, ids_freq_mapping=freq, _weight=w)


def _set(emb, layout, lr=cases.LR, **kw):
    kw = dict(MODULE_KW, **kw)
    if layout == "adagrad":
        emb.set_fused_adagrad(lr, lr_decay=0.1, **kw)
    else:
        emb.set_fused_adam(lr, **kw)


def _train(emb, steps, use_psw=True):
    for ids, off, go, psw in steps:
        out = emb(torch.from_numpy(ids).cuda(), torch.from_numpy(off).cuda(),
                  per_sample_weights=torch.from_numpy(psw).cuda() if use_psw else None)
        out.backward(torch.from_numpy(go).cuda())


def _state(emb, layout):
    """every part in ROW space after a flush, and the step count"""
    emb.flush()
    torch.cuda.synchronize()
    if layout == "adagrad":
        return [emb.weight.clone(), emb.state_sum.clone(), emb.adagrad_step.cpu()]
    return [emb.weight.clone(), emb.exp_avg.clone(), emb.exp_avg_sq.detach().cpu().clone(), emb.adam_step.cpu()]


def _assert_states_equal(a, b, tag):
    for k, (x, y) in enumerate(zip(a, b)):
        if x.dtype == torch.float32:
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{tag}: part {k}"
        else:
            assert torch.equal(x, y), f"{tag}: part {k}"


@pytest.mark.parametrize("strategy", ["LFU", "DATASET"])
@pytest.mark.parametrize("layout", sc.LAYOUTS)
def test_module_with_an_evicting_cache_equals_a_cache_that_holds_the_table(layout, strategy):
    """hot rows included, EVERY row bit for bit: a row's run is folded the same way whatever slot the row sits in"""
    u = 6
    steps = cases.zipf_steps(seed=21, max_unique=u)
    assert max(np.bincount(ids).max() for ids, _, _, _ in steps) > 2
    freq = torch.from_numpy(np.random.default_rng(1).permutation(cases.N).astype(np.int64))
    small, whole = (_module(layout, c, freq=freq, strategy=strategy) for c in (u + 2, cases.N))
    assert torch.equal(small.weight, whole.weight)
    row_of_id = small.cache_weight_mgr.idx_map.cpu().numpy().astype(np.int64)
    assert (row_of_id != np.arange(cases.N)).any() == (strategy == "DATASET")
    W0 = small.weight.clone()
    for e in (small, whole):
        _set(e, layout)
        _train(e, steps)
    assert sum(n > 0 for n in small.num_write_back_history) >= len(steps) // 2, small.num_write_back_history
    got, want = _state(small, layout), _state(whole, layout)
    _assert_states_equal(got, want, f"{layout} {strategy}")
    assert int(got[-1].item()) == len(steps) and not torch.equal(got[0], W0) and got[1].abs().sum() > 0


def test_prefetch_window_steps_equal_eager_steps_bit_for_bit():
    from cachedembedding_amd.pipeline import PrefetchWindow
    layout = "adam"
    steps = cases.zipf_steps(seed=22, max_unique=4)
    off_np = steps[0][1]
    steps = [(ids, off_np, go[:len(off_np) - 1], psw) for ids, _, go, psw in steps]      # one bag layout for the window
    eager, emb = _module(layout, 8, seed=78), _module(layout, 8, seed=78)
    for e in (eager, emb):
        _set(e, layout)
    _train(eager, steps, use_psw=False)
    emb.set_cache_op(False)
    off = torch.from_numpy(off_np).to(torch.int32).cuda()
    win = PrefetchWindow(emb, 2, presort=True, bag_layout=(off, True, 0))
    for k in range(0, len(steps), 2):
        slots = win.prepare([torch.from_numpy(s[0]).cuda() for s in steps[k:k + 2]])
        for i in range(2):
            out = emb(slots[i], off, presorted=win.keys[i])          # the keys are not needed and ignored
            out.backward(torch.from_numpy(steps[k + i][2]).cuda())
    assert int(emb.adam_step.item()) == len(steps) and sum(emb.num_write_back_history) > 0
    _assert_states_equal(_state(emb, layout), _state(eager, layout), "window")


@pytest.mark.parametrize("layout", ["adam", "adagrad"])
def test_resume_from_loaded_state_continues_bit_identically(layout):
    import cachedembedding_amd as ce
    k = 3
    steps = cases.zipf_steps(seed=23, steps=2 * k, max_unique=6)
    whole = _module(layout, 8, seed=5)
    _set(whole, layout)
    _train(whole, steps)
    first = _module(layout, 8, seed=5)
    _set(first, layout)
    _train(first, steps[:k])
    saved = _state(first, layout)
    second = ce.CachedEmbeddingBag.from_pretrained(saved[0], freeze=False, mode="sum", include_last_offset=True,
                                                   cuda_row_num=8, evict_strategy=ce.EvictionStrategy.LFU,
                                                   fused_optimizer=layout)
    if layout == "adagrad":
        second.load_adagrad_state(saved[1], int(saved[2].item()))
    else:
        second.load_adam_state(saved[1], saved[2], int(saved[3].item()))
    _set(second, layout)
    _train(second, steps[k:])
    _assert_states_equal(_state(second, layout), _state(whole, layout), layout)


@pytest.mark.parametrize("extra", [["--adam"], ["--adam", "--adam_partial_rowwise"], ["--adagrad_elementwise"],
                                   # (the example refuses --adam with --graph_step --change_lr: torch.optim.Adam of the
                                   # dense part reads its rate by value)
                                   ["--adagrad_elementwise", "--graph_step", "--graph_after", "6", "--change_lr",
                                    "--lr_change_point", "0.5", "--lr_after_change_point", "0.0025"]],
                         ids=["adam", "partial", "adagrad", "adagrad+graph_step+change_lr"])
def test_example_trains_the_toy_configuration_with_the_sorted_update(extra, capsys):
    import importlib
    import cachedembedding_amd as ce
    sys.path.insert(0, str(HERE.parent / "examples"))
    dm = importlib.import_module("dlrm_main")
    name = "set_fused_adagrad" if "--adagrad_elementwise" in extra else "set_fused_adam"
    seen = []
    orig = getattr(ce.CachedEmbeddingBag, name)

    def spy(self, *a, **kw):
        seen.append((self, a, kw))
        return orig(self, *a, **kw)
    setattr(ce.CachedEmbeddingBag, name, spy)
    try:
        dm.main(["--dataset", "avazu", "--table_scale", "0.01", "--batch_size", "256", "--embedding_dim", "32",
                 "--dense_arch_layer_sizes", "64,32", "--over_arch_layer_sizes", "64,1", "--use_cache", "--cache_ratio",
                 "0.03", "--use_freq", "--prefetch_num", "4", "--use_overlap", "--overlap_cache_op", "--fold_hook",
                 "--limit_train_batches", "16", "--learning_rate", "0.01", "--embed_sorted_update"] + extra)
    finally:
        setattr(ce.CachedEmbeddingBag, name, orig)
    out = capsys.readouterr().out
    emb = seen[0][0]
    assert seen[0][2]["accumulator"] == "sorted" and "16 iterations" in out
    step = emb.adagrad_step if name == "set_fused_adagrad" else emb.adam_step
    assert int(step.item()) == 16
    emb.flush()
    assert torch.isfinite(emb.weight).all()
    state = emb.state_sum if name == "set_fused_adagrad" else emb.exp_avg
    assert state.abs().sum() > 0 and torch.isfinite(state).all()
    if "--change_lr" in extra:
        assert "Changing learning rate to: 0.0025" in out and isinstance(seen[0][1][0], torch.Tensor)
        assert float(seen[0][1][0].item()) == np.float32(0.0025)     # the captured step read the rewritten tensor
    # the trainer keeps its last model, loaders and window in function attributes: let go of them here
    emb.cache_weight_mgr.writeback_wait()
    dm.main.model = dm.main.val_loader = dm.main.test_loader = None
    dm.train.window = None
    del emb, seen[:]


# ---- 8. the C refusals on the device: in their order, the table and *step as they were -----------------------------------

@pytest.mark.parametrize("layout", sc.LAYOUTS)
def test_c_refusals_leave_the_table_and_the_step_count_alone(layout):
    L = _lib()
    D = 32
    W0 = ac.initial_weight(D, 3)
    s = ac.once_steps(D, seed=3)[0]
    w = _table(layout, W0, fill=FILL)
    v = torch.full((ac.R,), FILL, device="cuda") if layout == "partial_rowwise_adam" else None
    before, v_before = w.clone(), None if v is None else v.clone()
    step = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    ws = _sorted_ws(len(s["ids"]), D)
    bad, unsup = L.CE_ERR_INVALID, L.CE_ERR_UNSUPPORTED

    def call(step=step, w=w, D=D, s=s, ws=ws, **kw):
        return _call(layout, w, D, s, ws, step, v=v, **kw)

    # every call piles later mistakes on the one that must be named
    late = dict(eps=-1.0, lr=-0.1, D=6)
    assert call(step=None, wd=1.0, wd_mode="l2", grad_clip=-1.0, **late) == bad and "step" in L.last_error()
    assert call(wd=-1.0, wd_mode="l2", grad_clip=-1.0, **late) == bad and "weight_decay" in L.last_error()
    assert call(grad_clip=-1.0, **late) == bad and "grad_clip" in L.last_error()
    if layout == "adagrad":
        assert call(lr_decay=-1.0, **late) == bad and "lr_decay" in L.last_error()
    assert call(**late) == bad and "eps" in L.last_error()
    assert call(lr=-0.1, D=6) == bad and "lr must be" in L.last_error()
    assert call(s=dict(s, hook=7), D=6) == bad and "hook_features" in L.last_error()
    assert call(ws=ws[4:], D=6) == bad and "aligned" in L.last_error()
    assert call(ws=ws[:ws.numel() - 256]) == bad and "workspace too small" in L.last_error()
    assert call(D=6) == unsup and "dim % 4 == 0" in L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(w.view(torch.int32), before.view(torch.int32)) and int(step.item()) == 7
    assert v is None or torch.equal(v.view(torch.int32), v_before.view(torch.int32))
    # and a good call counts one and moves the named rows only
    L.check(call())
    torch.cuda.synchronize()
    assert int(step.item()) == 8 and not torch.equal(w[:ac.ONCE_NAMED], before[:ac.ONCE_NAMED])
    assert torch.equal(w[ac.ONCE_NAMED:].view(torch.int32), before[ac.ONCE_NAMED:].view(torch.int32))
