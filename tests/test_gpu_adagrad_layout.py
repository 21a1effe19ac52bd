"""GPU tests of element-wise Adagrad with its state carried in the row (rows w | h): the forwards bit
for bit against their fp32 siblings, the update entries bit for bit against the fp32 model where every row is looked up
once and within the project's Adam tolerance of the fp64 model (tests/adagrad_layout_ref.py) on the 7-step cases, a
captured step, the module through an evicting cache and a prefetch window, resuming from saved state, quantizing, and the
C entries' refusals."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import adagrad_layout_cases as ac  # noqa: E402
import adagrad_layout_ref as ref  # noqa: E402
import adam_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = ac.RTOL, ac.ATOL     # the fp32 reference alone keeps half of it on these inputs (test_adagrad_layout_cpu.py)
LAYOUT = "adagrad"
DIMS = ac.DIMS
R, NNZ, NB, F = ac.R, ac.NNZ, ac.NB, ac.F
EPS = ac.EPS
WD_CODES = {None: 0, "l2": 1, "decoupled": 2}
CLIP_CODES = {None: 0, "value": 1, "row_norm": 2}


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    """the modules, graphs and streams of a test are collected and the device is idle before the next test starts: what
    a test of this file leaves in flight must surface in this file, not in whichever test comes next"""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()


def _lib():
    from cachedembedding_amd import _lib as L
    return L


def _stream():
    return _lib().stream_ptr()


def _table(W0, fill=0.0):
    """[R, 2 D] device table with the w parts W0 and every h element `fill`"""
    n, D = W0.shape
    t = torch.full((n, 2 * D), fill, dtype=torch.float32)
    t[:, :D] = torch.from_numpy(W0)
    return t.cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the forwards: bit-equal to the fp32 entries over the contiguous w parts --------------------------------------

@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("D", DIMS)
def test_forwards_equal_the_fp32_forwards_bit_for_bit(D, out_dtype):
    from cachedembedding_amd.functional import presort_window
    L = _lib()
    lib, ptr = L.lib, L.ptr
    act = L.ACT_DTYPES[out_dtype]
    as_int = torch.int32 if out_dtype == torch.float32 else torch.int16
    rng = np.random.default_rng(D)
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    table = _table(W0, fill=float("nan"))                           # a stray read of an h part shows
    plain = torch.from_numpy(W0).cuda()
    n = 512
    ids = rng.integers(0, R, n)
    ids[rng.random(n) < 0.1] = -1
    idx = torch.from_numpy(ids.astype(np.int64)).cuda()
    cuts = np.sort(rng.integers(0, n + 1, 99))
    ragged = torch.from_numpy(np.concatenate([[0], cuts, [n]]).astype(np.int64)).cuda()
    psw = torch.from_numpy(rng.uniform(0, 2, n).astype(np.float32)).cuda()
    arange = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    forms = [("sum+psw", ragged, 100, psw, L.CE_MODE_SUM, 0),
             ("mean/int32", ragged.to(torch.int32), 100, None, L.CE_MODE_MEAN, 0),
             ("hook", ragged, 100, None, L.CE_MODE_SUM, F),
             ("one id per bag", arange, n, None, L.CE_MODE_SUM, F),
             ("NULL offsets", None, n, None, L.CE_MODE_SUM, 0)]
    for name, off, nb, p, mode, hook in forms:
        outs = []
        for fn, w in ((lib.ce_bag_forward_adagrad, table), (lib.ce_bag_forward_act, plain)):
            o = torch.full((nb, D), 7.0, dtype=out_dtype, device="cuda")
            L.check(fn(ptr(w), R, D, ptr(idx), n, ptr(off), int(off is not None and off.dtype == torch.int64), nb, 1,
                       ptr(p), mode, hook, ptr(o), act, _stream()))
            outs.append(o)
        assert torch.equal(outs[0].view(as_int), outs[1].view(as_int)), name
        assert not torch.isnan(outs[0].float()).any()
    keys = presort_window(idx.view(1, -1), R, offsets=arange.to(torch.int32), include_last_offset=True,
                          hook_features=0, identity_bags=True)[0]
    outs = []
    for fn, w in ((lib.ce_bag_forward_src_keys_adagrad, table), (lib.ce_bag_forward_src_keys_act, plain)):
        o = torch.full((n, D), 7.0, dtype=out_dtype, device="cuda")
        L.check(fn(ptr(w), R, D, n, ptr(keys.keys), ptr(o), act, _stream()))
        outs.append(o)
    assert torch.equal(outs[0].view(as_int), outs[1].view(as_int)), "src keys"
    assert (outs[0][idx < 0] == 0).all()                            # an ignored key: a zero row
    torch.cuda.synchronize()
    assert torch.isnan(table[:, D:]).all() and torch.equal(table[:, :D], plain)      # the forward writes nothing


# ---- the update entries ----------------------------------------------------------------------------------------------

def _call_update(w, D, s, src, acc_code, ws, step, lr, lr_dev=None, lr_decay=0.0, wd=0.0, wd_mode=None, grad_clip=None,
                 clip_mode=None, eps=EPS, **_):
    """one call of ce_bag_backward_adagrad / _adagrad_src for the step dict s (ids, off, off32, mode, psw, hook, go, act);
    returns the status"""
    from cachedembedding_amd.functional import presort_window
    L = _lib()
    lib, ptr = L.lib, L.ptr
    n_rows = w.shape[0]
    idx = torch.from_numpy(s["ids"]).cuda()
    off = torch.from_numpy(s["off"]).cuda()
    if s.get("off32"):
        off = off.to(torch.int32)
    nb = off.numel() - 1
    go = torch.from_numpy(s["go"]).cuda().to(s.get("act", torch.float32))
    act = L.ACT_DTYPES[go.dtype]
    psw = None if s.get("psw") is None else torch.from_numpy(s["psw"]).cuda()
    nnz = idx.numel()
    clip = grad_clip is not None
    tail = (lr_decay, 0.0 if lr_dev is not None else lr, ptr(lr_dev), eps, wd if wd_mode else 0.0, WD_CODES[wd_mode],
            float(grad_clip) if clip else 0.0, CLIP_CODES[clip_mode if clip else None], ptr(step), acc_code, ptr(ws),
            ws.numel(), _stream())
    if src:
        keys = None if nnz == 0 else presort_window(idx.view(1, -1), n_rows, offsets=off, include_last_offset=True,
                                                    hook_features=s.get("hook", 0))[0].keys
        return lib.ce_bag_backward_adagrad_src(ptr(w), n_rows, D, nnz, ptr(go), act, ptr(keys), *tail)
    return lib.ce_bag_backward_adagrad(ptr(w), n_rows, D, ptr(idx), nnz, ptr(off), int(off.dtype == torch.int64), nb, 1,
                                       ptr(psw), L.CE_MODE_MEAN if s.get("mode") == "mean" else L.CE_MODE_SUM,
                                       s.get("hook", 0), ptr(go), act, None, *tail)


def _workspace(n_rows, nnz, D, acc):
    L = _lib()
    code = L.CE_ACC_STEP if acc == "step" else L.CE_ACC_CACHE
    need = L.lib.ce_bag_backward_adagrad_workspace(n_rows, nnz, D, code)
    assert need == L.lib.ce_bag_backward_adam_workspace(n_rows, nnz, D, code)
    return code, torch.zeros(need, dtype=torch.uint8, device="cuda")


def _run_entries(W0, steps, src, acc, lr_dev, init_acc=0.0, **kw):
    """(table [R, 2 D] numpy) after the steps through the C entries"""
    L = _lib()
    D = W0.shape[1]
    if kw.get("clip_mode") == "row_norm" and kw.get("grad_clip") is None:
        kw = dict(kw, grad_clip=ac.row_norm_threshold(D))
    w = _table(W0, fill=init_acc)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert len({len(s["ids"]) for s in steps}) == 1                  # (a step-sized workspace serves one nnz)
    code, ws = _workspace(R, len(steps[0]["ids"]), D, acc)
    lr_t = torch.zeros(1, dtype=torch.float32, device="cuda") if lr_dev else None
    for s in steps:
        if lr_dev:
            lr_t.fill_(s["lr"])                                      # the rate as a tensor, changed between steps
        L.check(_call_update(w, D, s, src, code, ws, step, s["lr"], lr_dev=lr_t, **kw))
    torch.cuda.synchronize()
    assert int(step.item()) == len(steps)
    if acc == "cache":
        assert not ws.any()                                          # left zero-filled
    return w.cpu().numpy()


# ---- 2. rows looked up once: nothing has an order to choose, so the fp32 model's bits ------------------------------

@pytest.mark.parametrize("setting", list(ac.ONCE_SETTINGS))
@pytest.mark.parametrize("D", DIMS)
def test_rows_looked_up_once_equal_the_fp32_model_bit_for_bit(D, setting):
    kw = ac.ONCE_SETTINGS[setting]
    steps = ac.once_steps(D, seed=D)
    W0 = ac.initial_weight(D, D + 1)
    W, S, named = ac.model(W0, steps, np.float32, **kw)
    assert named[:ac.ONCE_NAMED].all() and not named[ac.ONCE_NAMED:].any()
    default = ac.model(W0, steps, np.float32)
    assert setting == "default" or (W != default[0]).any() or (S != default[1]).any()      # the setting does something
    init = np.float32(kw.get("init_acc", 0.0))
    got = {}
    for acc in ("cache", "step"):
        for src in (False, True):
            t = _run_entries(W0, steps, src, acc, lr_dev=src, **kw)
            tag = f"D={D} {setting} {acc} {'src' if src else 'slots'}"
            np.testing.assert_array_equal(_bits(t[:, :D]), _bits(W), err_msg=f"w {tag}")
            np.testing.assert_array_equal(_bits(t[:, D:]), _bits(S), err_msg=f"s {tag}")
            # rows never named keep their bits
            np.testing.assert_array_equal(_bits(t[ac.ONCE_NAMED:, :D]), _bits(W0[ac.ONCE_NAMED:]), err_msg=tag)
            assert (t[ac.ONCE_NAMED:, D:] == init).all(), tag
            got[acc, src] = t
    np.testing.assert_array_equal(_bits(got["cache", False]), _bits(got["step", False]))
    np.testing.assert_array_equal(_bits(got["cache", True]), _bits(got["step", True]))


# ---- 3. the 7-step cases against the fp64 model ---------------------------------------------------------------------

@pytest.mark.parametrize("case", list(ac.MODEL_CASES))
@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
@pytest.mark.parametrize("D", DIMS)
def test_update_entries_against_the_fp64_model(D, src, case):
    """both accumulators; sum, mean, per-sample weights with zeros, ragged and empty bags, hook_features, an ignored
    lookup, lookups no bag covers, fp32 / bf16 / fp16 gradients (kernel_steps); the rate by value (slots) or as a
    tensor (src), changed between steps"""
    kw = ac.MODEL_CASES[case]
    W0 = ac.initial_weight(D, D)
    steps = ac.kernel_steps(D, src, seed=D)
    W, S, named = ac.model(W0, steps, np.float64, **kw)
    assert not named[R - 5:].any() and named[R - 20:R - 5].any() and named[ac.HOT]
    init = np.float32(kw.get("init_acc", 0.0))
    got = {}
    for acc in ("cache", "step"):
        t = got[acc] = _run_entries(W0, steps, src, acc, lr_dev=src, **kw)
        for name, g, want in (("w", t[:, :D], W), ("s", t[:, D:], S)):
            err = np.abs(g - want) / (ATOL + RTOL * np.abs(want))
            print(f"D={D} {'src' if src else 'slots'} {case} {acc} {name}: max |err| / (atol + rtol |ref|) = "
                  f"{err.max():.3g}")
            np.testing.assert_allclose(g, want, rtol=RTOL, atol=ATOL, err_msg=f"{acc} {name}")
        # the named set is the reference's: rows no covered lookup names -- the row in the uncovered tail among them --
        # keep their bits, decay or not; what the named rows hold is the comparison above
        np.testing.assert_array_equal(_bits(t[~named, :D]), _bits(W0[~named]))
        assert (t[~named, D:] == init).all()
    # rows looked up at most once per step: one atomic add onto zero is exact, so the accumulators agree bit for bit
    once = np.arange(R - 20, R - 5)
    np.testing.assert_array_equal(_bits(got["cache"][once]), _bits(got["step"][once]))


# ---- 4. a captured backward replayed ------------------------------------------------------------------------------

@pytest.mark.parametrize("wd_mode", [None, "decoupled"])
def test_captured_step_replayed_equals_eager_steps_and_counts_on(wd_mode):
    """three replays equal three eager steps bit for bit: the step count (lr_decay) and a device rate changed between
    replays reach clr and, with the decoupled decay, f"""
    from cachedembedding_amd.functional import FusedAdagrad, embedding_bag
    rng = np.random.default_rng(9)
    n_rows, D, n, K = 70, 128, 96, 3
    lrs = [0.05, 0.0125, 0.2]
    W0 = rng.standard_normal((n_rows, D)).astype(np.float32)
    ids = np.concatenate([rng.permutation(n_rows - 5)[:n // 2]] * 2)  # every row at most twice: the atomics cannot reorder
    idx = torch.from_numpy(ids[rng.permutation(n)].astype(np.int64)).cuda()
    off = torch.arange(0, n + 1, 2, dtype=torch.int64, device="cuda")
    go = torch.from_numpy(rng.standard_normal((n // 2, D)).astype(np.float32)).cuda()
    kw = dict(lr_decay=0.5, weight_decay=0.1 if wd_mode else 0.0, weight_decay_mode=wd_mode or "l2")

    def fused(lr):
        return FusedAdagrad(lr, step=torch.zeros(1, dtype=torch.int64, device="cuda"), **kw)

    def one_step(w, f):
        w.requires_grad_(True)
        out = embedding_bag(idx, w, off, mode="sum", include_last_offset=True, fused_sgd=f)
        out.backward(go)
        assert w.grad is None

    we, fe = _table(W0), fused(lrs[0])
    eager = []
    for lr in lrs:
        fe.lr = lr
        one_step(we, fe)
        eager.append(we.detach().clone())
    # the schedule and the step count both matter to the eager run: this is what the replay has to follow
    same_rate, no_count = _table(W0), _table(W0)
    f1, f2 = fused(lrs[0]), fused(lrs[0])
    for lr in lrs:
        one_step(same_rate, f1)
        f2.lr = lr
        f2.step.zero_()
        one_step(no_count, f2)
    assert not torch.equal(same_rate.detach(), eager[-1]) and not torch.equal(no_count.detach(), eager[-1])

    lr_t = torch.full((1,), lrs[0], dtype=torch.float32, device="cuda")
    wg, fg = _table(W0), fused(lr_t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_step(wg, fg)                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():                                            # back to the start: table and step count
        wg.copy_(_table(W0))
        fg.step.zero_()
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
    assert int(fg.step.item()) == K and int(fe.step.item()) == K


# ---- 5. through the module ----------------------------------------------------------------------------------------------

MODULE_KW = dict(lr_decay=0.1, weight_decay=0.01, weight_decay_mode="decoupled")
INIT = 0.1


def _module(cuda_row_num, seed=77, freq=None, strategy="LFU", init_acc=INIT, w=None):
    import cachedembedding_amd as ce
    return ce.CachedEmbeddingBag(cases.N, cases.D, mode="sum", include_last_offset=True, cuda_row_num=cuda_row_num,
                                 evict_strategy=getattr(ce.EvictionStrategy, strategy), fused_optimizer=LAYOUT,
                                 init_seed=seed, ids_freq_mapping=freq, initial_accumulator_value=init_acc, _weight=w)


def _train(emb, steps, use_psw=True):
    for ids, off, go, psw in steps:
        out = emb(torch.from_numpy(ids).cuda(), torch.from_numpy(off).cuda(),
                  per_sample_weights=torch.from_numpy(psw).cuda() if use_psw else None)
        out.backward(torch.from_numpy(go).cuda())


def _state(emb):
    """(w [N, D], s [N, D]) numpy in ROW space after a flush"""
    emb.flush()
    torch.cuda.synchronize()
    assert tuple(emb.weight.shape) == (cases.N, cases.D) and tuple(emb.state_sum.shape) == (cases.N, cases.D)
    return emb.weight.clone().numpy(), emb.state_sum.clone().numpy()


def _whole_table(W0, steps, init_acc=INIT, use_psw=True, lr=cases.LR, **kw):
    """the same steps on the whole table in device memory, no cache: (w, s) numpy in id space"""
    from cachedembedding_amd.functional import FusedAdagrad, embedding_bag
    t = _table(W0, fill=init_acc).requires_grad_(True)
    f = FusedAdagrad(lr, step=torch.zeros(1, dtype=torch.int64, device="cuda"), **kw)
    for ids, off, go, psw in steps:
        out = embedding_bag(torch.from_numpy(ids).cuda(), t, torch.from_numpy(off).cuda(), mode="sum",
                            include_last_offset=True, fused_sgd=f,
                            per_sample_weights=torch.from_numpy(psw).cuda() if use_psw else None)
        out.backward(torch.from_numpy(go).cuda())
    torch.cuda.synchronize()
    assert int(f.step.item()) == len(steps)
    t = t.detach().cpu().numpy()
    return t[:, :cases.D], t[:, cases.D:]


def _reference(W0, steps, init_acc=INIT, use_psw=True, lr=cases.LR, lr_decay=0.0, weight_decay=0.0,
               weight_decay_mode="l2"):
    W = W0.astype(np.float64)
    S = np.full_like(W, np.float64(np.float32(init_acc)))
    for t, (ids, off, go, psw) in enumerate(steps, 1):
        rows, grads = ref.lookup_grads(ids, off, go, cases.N, psw=psw if use_psw else None)
        ref.step(W, S, rows, grads, lr, t, EPS, lr_decay, wd=weight_decay, wd_mode=weight_decay_mode)
    return W, S


def _unique_steps(seed, steps=6):
    """one id per bag, every row at most once per step: nothing for the atomics to reorder.  The window of rows moves on
    so that a cache of 8 rows evicts and sees rows again."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(steps):
        ids = ((k * 4 + rng.permutation(10)[:6]) % 40).astype(np.int64)
        go = rng.standard_normal((6, cases.D)).astype(np.float32)
        out.append((ids, np.arange(7, dtype=np.int64), go, np.ones(6, np.float32)))
    return out


@pytest.mark.parametrize("strategy", ["LFU", "DATASET"])
def test_module_through_an_evicting_cache_with_a_reordered_table(strategy):
    """a cache of 8 rows evicts at every step and sees rows again; its flushed weight and state_sum against the same
    steps on the whole table with no cache -- bit for bit where each step's rows are looked up once, within the
    tolerance (and of the fp64 reference) otherwise.  ids_freq_mapping makes idx_map no identity."""
    u = 6
    freq = torch.from_numpy(np.random.default_rng(1).permutation(cases.N).astype(np.int64))
    for steps, exact in ((cases.zipf_steps(seed=21, max_unique=u), False), (_unique_steps(4, 8), True)):
        emb = _module(u + 2, freq=freq, strategy=strategy)
        assert tuple(emb.cache_weight_mgr.cuda_cached_weight.shape) == (u + 2, 2 * cases.D)
        assert emb.embedding_dim == cases.D
        row_of_id = emb.cache_weight_mgr.idx_map.cpu().numpy().astype(np.int64)
        # (DATASET reorders the table by frequency; LFU preloads the frequent rows and keeps the identity map)
        assert (row_of_id != np.arange(cases.N)).any() == (strategy == "DATASET")
        W0 = emb.weight.clone().numpy()[row_of_id]                  # row space -> id space
        assert (emb.state_sum == INIT).all()
        emb.set_fused_adagrad(cases.LR, **MODULE_KW)
        _train(emb, steps)
        assert emb.cache_weight_mgr.cuda_cached_weight.grad is None and int(emb.adagrad_step.item()) == len(steps)
        assert emb.adagrad_step.is_cuda
        assert sum(n > 0 for n in emb.num_write_back_history) >= len(steps) // 2, emb.num_write_back_history
        got = [x[row_of_id] for x in _state(emb)]
        whole = _whole_table(W0, steps, **MODULE_KW)
        want = _reference(W0, steps, **MODULE_KW)
        for name, g, t, w in zip(("weight", "state_sum"), got, whole, want):
            if exact:
                np.testing.assert_array_equal(_bits(g), _bits(t), err_msg=name)
            np.testing.assert_allclose(g, t, rtol=RTOL, atol=ATOL, err_msg=f"{name} against the whole table")
            np.testing.assert_allclose(g.astype(np.float64), w, rtol=RTOL, atol=ATOL, err_msg=name)
        untouched = np.arange(40, cases.N)
        np.testing.assert_array_equal(_bits(got[0][untouched]), _bits(W0[untouched]))
        assert (got[1][untouched] == np.float32(INIT)).all() and (got[1][:40] != np.float32(INIT)).any()


def test_prefetch_window_step_equals_eager_steps():
    from cachedembedding_amd.pipeline import PrefetchWindow
    steps = cases.zipf_steps(seed=22, max_unique=4)
    off_np = steps[0][1]
    steps = [(ids, off_np, go[:len(off_np) - 1], psw) for ids, _, go, psw in steps]      # one bag layout for the window
    eager, emb = _module(8, seed=78), _module(8, seed=78)
    W0 = emb.weight.clone().numpy()
    for e in (eager, emb):
        e.set_fused_adagrad(cases.LR, accumulator="cache", **MODULE_KW)
    _train(eager, steps, use_psw=False)
    emb.set_cache_op(False)
    off = torch.from_numpy(off_np).to(torch.int32).cuda()
    win = PrefetchWindow(emb, 2, presort=True, bag_layout=(off, True, 0))
    for k in range(0, len(steps), 2):
        slots = win.prepare([torch.from_numpy(s[0]).cuda() for s in steps[k:k + 2]])
        for i in range(2):
            assert type(win.keys[i]).__name__ == "SrcKeys"           # the _src entries
            out = emb(slots[i], off, presorted=win.keys[i])
            out.backward(torch.from_numpy(steps[k + i][2]).cuda())
    assert int(emb.adagrad_step.item()) == len(steps) and sum(emb.num_write_back_history) > 0
    want = _reference(W0, steps, use_psw=False, **MODULE_KW)
    got, got_eager = _state(emb), _state(eager)
    for name, g, e, w in zip(("weight", "state_sum"), got, got_eager, want):
        np.testing.assert_allclose(g.astype(np.float64), w, rtol=RTOL, atol=ATOL, err_msg=name)
        np.testing.assert_allclose(g, e, rtol=RTOL, atol=ATOL, err_msg=f"{name} against eager")


# ---- 6. resume and quantize -------------------------------------------------------------------------------------------

def test_resume_from_loaded_state_continues_bit_identically():
    k = 3
    steps = _unique_steps(4, 2 * k)
    whole = _module(8, seed=5)
    whole.set_fused_adagrad(cases.LR, **MODULE_KW)
    _train(whole, steps)
    first = _module(8, seed=5)
    first.set_fused_adagrad(cases.LR, **MODULE_KW)
    _train(first, steps[:k])
    first.flush()
    saved = (first.weight.clone(), first.state_sum.clone(), int(first.adagrad_step.item()))
    assert saved[2] == k and (saved[1] != INIT).any()
    import cachedembedding_amd as ce
    second = ce.CachedEmbeddingBag.from_pretrained(saved[0], freeze=False, mode="sum", include_last_offset=True,
                                                   cuda_row_num=8, evict_strategy=ce.EvictionStrategy.LFU,
                                                   fused_optimizer=LAYOUT)      # the weights, a fresh state
    assert not second.state_sum.any() and int(second.adagrad_step.item()) == 0
    second.load_adagrad_state(saved[1], saved[2])
    assert int(second.adagrad_step.item()) == k and second.adagrad_step.is_cuda
    assert torch.equal(second.state_sum, saved[1]) and torch.equal(second.weight, saved[0])
    second.set_fused_adagrad(cases.LR, **MODULE_KW)
    _train(second, steps[k:])
    assert int(second.adagrad_step.item()) == 2 * k
    for name, g, w in zip(("weight", "state_sum"), _state(second), _state(whole)):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=name)
    with pytest.raises(ValueError, match="state_sum must be"):
        second.load_adagrad_state(saved[1][:, :4], k)


def test_initialisation_refusals_and_quantization():
    import cachedembedding_amd as ce
    from cachedembedding_amd.functional import quantize_rows
    a = _module(8, seed=4242)
    p = ce.CachedEmbeddingBag(cases.N, cases.D, mode="sum", cuda_row_num=8, init_seed=4242)
    assert torch.equal(a.weight.view(torch.int32), p.weight.view(torch.int32)) and a.weight.abs().sum() > 0
    assert tuple(a.cache_weight_mgr.weight.shape) == (cases.N, 2 * cases.D)
    assert (a.state_sum == INIT).all() and int(a.adagrad_step.item()) == 0
    # padding_idx zeroes the w part of that row only
    pad = ce.CachedEmbeddingBag(cases.N, cases.D, mode="sum", cuda_row_num=8, init_seed=4242, padding_idx=3,
                                fused_optimizer=LAYOUT, initial_accumulator_value=INIT)
    assert not pad.weight[3].any() and (pad.state_sum == INIT).all() and pad.weight[2].any()
    w = torch.randn(cases.N, 16)
    f = ce.CachedEmbeddingBag.from_pretrained(w, freeze=False, cuda_row_num=8, mode="sum", fused_optimizer=LAYOUT,
                                              include_last_offset=True, initial_accumulator_value=0.5)
    assert torch.equal(f.weight, w) and (f.state_sum == 0.5).all() and f.embedding_dim == 16
    for call in (lambda: a.set_fused_sgd(0.1), lambda: a.set_fused_rowwise_adagrad(0.1)):
        with pytest.raises(NotImplementedError, match="Adagrad-layout"):
            call()
    with pytest.raises(ValueError, match="set_fused_adam needs"):
        a.set_fused_adam(0.1)
    with pytest.raises(ValueError, match="set_fused_adagrad needs"):
        p.set_fused_adagrad(0.1)
    with pytest.raises(ValueError, match="load_adagrad_state"):
        p.load_adagrad_state(torch.zeros(cases.N, cases.D), 1)
    with pytest.raises(AttributeError):
        p.state_sum
    with pytest.raises(AttributeError):
        a.exp_avg
    # eval-mode forward needs no optimizer; a backward without one is refused in backward
    ids = torch.arange(6, device="cuda")
    off = torch.arange(0, 7, 2, device="cuda")
    a.eval()
    with torch.no_grad():
        out = a(ids, off)
    want = torch.nn.functional.embedding_bag(ids.cpu(), a.weight, off.cpu()[:-1], mode="sum")
    torch.testing.assert_close(out.cpu(), want, rtol=1e-6, atol=1e-7)
    a.train()
    out = a(ids, off)
    with pytest.raises(RuntimeError, match="no fused Adagrad set"):
        out.sum().backward()
    # functional refusals with the switch, as with FusedAdam
    from cachedembedding_amd.functional import FusedAdagrad, embedding_bag
    fz = FusedAdagrad(0.1, step=torch.zeros(1, dtype=torch.int64, device="cuda"))
    t = torch.zeros(8, 32, device="cuda")
    psw = torch.ones(6, device="cuda", requires_grad=True)
    for kw in (dict(mode="max"), dict(max_norm=1.0), dict(sparse=True), dict(per_sample_weights=psw)):
        with pytest.raises(NotImplementedError, match="Adagrad-layout"):
            embedding_bag(ids, t, off, **{"mode": "sum", "include_last_offset": True, "fused_sgd": fz, **kw})
    # quantized() of a TRAINED module quantizes the w parts: quantize_rows of its .weight
    f.set_fused_adagrad(0.05)
    out = f(ids, off)
    out.backward(torch.ones_like(out))
    q = f.quantized(cuda_row_num=8)
    assert not torch.equal(f.weight, w)                              # (it trained, and quantized() flushed it)
    want_rows = quantize_rows(f.weight.contiguous())
    assert torch.equal(q.cache_weight_mgr.weight, want_rows)


# ---- 7. the C entries' refusals: in the stated order, the table untouched; nnz == 0 counts no step ------------------

@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
def test_c_refusals_leave_the_table_alone_and_an_empty_call_counts_no_step(src):
    L = _lib()
    D = 32
    W0 = ac.initial_weight(D, 3)
    s = ac.once_steps(D, seed=3)[0]
    w = _table(W0, fill=0.25)
    before = w.clone()
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    code, ws = _workspace(R, len(s["ids"]), D, "cache")

    def call(**kw):
        st = kw.pop("step", step)
        return _call_update(kw.pop("w", w), kw.pop("D", D), s, src, kw.pop("acc", code), kw.pop("ws", ws), st, 0.1, **kw)

    bad = L.CE_ERR_INVALID
    # the order: step == NULL before the accumulator code before lr_decay before eps before the dim rule
    assert call(step=None, acc=7, lr_decay=-1.0, eps=-1.0, D=6) == bad and "step" in L.last_error()
    assert call(acc=7, lr_decay=-1.0, eps=-1.0, D=6) == bad and "accumulator" in L.last_error()
    assert call(lr_decay=-1.0, eps=-1.0, D=6) == bad and "lr_decay" in L.last_error()
    assert call(lr_decay=float("nan"), D=6) == bad and "lr_decay" in L.last_error()
    assert call(eps=-1.0, D=6) == bad and "eps" in L.last_error()
    assert call(D=6) == L.CE_ERR_UNSUPPORTED and "dim % 4 == 0" in L.last_error()
    assert call(ws=ws[:ws.numel() - 256]) == bad and "workspace too small" in L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(w.view(torch.int32), before.view(torch.int32)) and int(step.item()) == 0 and not ws.any()
    # nnz == 0: after the checks, no launch, no step counted
    empty = dict(s, ids=np.zeros(0, np.int64), off=np.zeros(1, np.int64), go=np.zeros((1, D), np.float32))
    for acc in ("cache", "step"):
        c, wsp = _workspace(R, 0, D, acc)
        assert _call_update(w, D, empty, src, c, wsp, step, 0.1) == L.CE_OK
        assert _call_update(w, D, empty, src, c, wsp, step, 0.1, eps=-1.0) == bad            # (the checks still run)
    torch.cuda.synchronize()
    assert torch.equal(w.view(torch.int32), before.view(torch.int32)) and int(step.item()) == 0
    # and a good call counts one and moves the named rows
    L.check(call())
    torch.cuda.synchronize()
    assert int(step.item()) == 1 and not torch.equal(w[:ac.ONCE_NAMED], before[:ac.ONCE_NAMED])
    assert torch.equal(w[ac.ONCE_NAMED:].view(torch.int32), before[ac.ONCE_NAMED:].view(torch.int32))


def test_eps_zero_on_a_zero_state_is_nan_as_in_torch():
    L = _lib()
    D = 8
    W0 = ac.initial_weight(D, 1)
    go = np.ones((2, D), np.float32)
    go[1] = 0.0                                                      # row 5: g = 0 on s = 0
    s = dict(ids=np.asarray([4, 5], np.int64), off=np.arange(3, dtype=np.int64), go=go)
    w = _table(W0)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    code, ws = _workspace(R, 2, D, "cache")
    L.check(_call_update(w, D, s, False, code, ws, step, 0.1, eps=0.0))
    torch.cuda.synchronize()
    t = w.cpu().numpy()
    assert np.isnan(t[5, :D]).all() and not np.isnan(t[4]).any() and not t[5, D:].any()
    np.testing.assert_array_equal(t[4, :D], W0[4] - np.float32(0.1))  # g / sqrt(g g) = 1


# ---- the example trainer ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", [
    ["--window_keys", "--embed_weight_decay", "0.001", "--embed_grad_clip", "1.0", "--step_accumulator"],
    ["--graph_step", "--graph_after", "6", "--change_lr", "--lr_change_point", "0.5", "--lr_after_change_point", "0.0025"]],
    ids=["window_keys+decay+clip", "graph_step+change_lr"])
def test_example_trains_the_toy_configuration(extra, capsys):
    """examples/dlrm_main.py --adagrad_elementwise end to end: prefetch windows, the fused element-wise Adagrad on the
    embedding, torch.optim.Adagrad (--graph_step --change_lr: the device-rate step) on the dense part; the sums of
    squares are in the host table afterwards and the step count is the number of batches"""
    import importlib
    import cachedembedding_amd as ce
    sys.path.insert(0, str(HERE.parent / "examples"))
    dm = importlib.import_module("dlrm_main")
    seen = []
    orig = ce.CachedEmbeddingBag.set_fused_adagrad

    def spy(self, *a, **kw):
        seen.append((self, a, kw))
        return orig(self, *a, **kw)
    ce.CachedEmbeddingBag.set_fused_adagrad = spy
    try:
        dm.main(["--dataset", "avazu", "--table_scale", "0.01", "--batch_size", "256", "--embedding_dim", "32",
                 "--dense_arch_layer_sizes", "64,32", "--over_arch_layer_sizes", "64,1", "--use_cache", "--cache_ratio",
                 "0.03", "--use_freq", "--prefetch_num", "4", "--use_overlap", "--overlap_cache_op",
                 "--adagrad_elementwise", "--fold_hook", "--limit_train_batches", "16", "--learning_rate", "0.01"] + extra)
    finally:
        ce.CachedEmbeddingBag.set_fused_adagrad = orig
    out = capsys.readouterr().out
    emb = seen[0][0]
    assert emb.fused_optimizer == LAYOUT and int(emb.adagrad_step.item()) == 16 and "16 iterations" in out
    emb.flush()
    assert emb.state_sum.abs().sum() > 0 and torch.isfinite(emb.weight).all() and torch.isfinite(emb.state_sum).all()
    if "--change_lr" in extra:
        assert "Changing learning rate to: 0.0025" in out and isinstance(seen[0][1][0], torch.Tensor)
        assert float(seen[0][1][0].item()) == np.float32(0.0025)     # the captured step read the rewritten tensor
    else:
        kw = seen[0][2]
        assert kw["weight_decay"] == 0.001 and kw["grad_clip"] == 1.0 and kw["accumulator"] == "step"
    # the trainer keeps its last model, loaders and window in function attributes: let go of them here
    emb.cache_weight_mgr.writeback_wait()
    dm.main.model = dm.main.val_loader = dm.main.test_loader = None
    dm.train.window = None
    del emb, seen[:]
