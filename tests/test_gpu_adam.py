"""GPU tests of the fused Adam of an Adam-layout table (rows w | m | v): the update entries against
the fp64 model (tests/adam_ref.py) for both accumulators, the two forwards bit for bit against their fp32 siblings,
the moments through a cache that evicts at every step (against torch.optim.SparseAdam on the CPU), a captured step
replayed with three learning rates, and the initialisation."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import adam_cases as cases  # noqa: E402
import adam_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6           # the project's own (test_gpu_rowwise_adagrad.py); torch's fp32 run keeps it on the CPU
LR, BETAS, EPS = 0.05, (0.9, 0.999), 1e-8
DIMS = [4, 100, 128, 260, 1024]   # one lane | a masked last chunk | the bench shape | two chunks per lane, masked | 4 x 64
ROWS = [70, 4100]                 # across a 64-position wave | across a CE_COMPACT_BLOCK
STEPS = 6
NNZ = 600
HOT, F = 3, 4


def _lib():
    from cachedembedding_amd import _lib as L
    return L


def _stream():
    return _lib().stream_ptr()


def _table(W0, fill=0.0):
    """[R, 3 D] device table with the w parts W0 and the moments `fill`"""
    R, D = W0.shape
    t = torch.full((R, 3 * D), fill, dtype=torch.float32)
    t[:, :D] = torch.from_numpy(W0)
    return t.cuda()


# ---- kernel level: ce_bag_backward_adam / _adam_src against the fp64 model ----------------------------------------

def _steps(R, D, src, seed):
    """6 steps of <= 600 lookups.  Row HOT is looked up 70 times in every step; rows [R - 20, R - 5) at most once per
    step; rows [R - 5, R) never -- except in the tail no bag covers.  By step: 0 slot -1 and an uncovered tail, 1 mean,
    2 per-sample weights with zeros (one row named ONLY with weight zero), 3 int32 offsets, 4 hook_features, 5 bf16
    grad_out.  Source-row keys hold no per-lookup scale: there steps 1 and 2 are plain sums.

    The gradients of a step have one sign per column and magnitudes in [0.01, 0.03), so a row's folded gradient never
    cancels within a step, and the hot row's 70 terms sum to at most 2.1 in magnitude: the fp32 fold then errs by at
    most 69 u 2.1 = 8.7e-6 (u = 2^-24), a tenth of which reaches m -- inside atol = 1e-6 whatever m has cancelled to over
    the steps (the signs change from step to step).  Adam's step m' / (sqrt(v') + eps) is ill-conditioned where sqrt(v') is of the size of eps -- a first
    gradient of |g| <~ eps / sqrt(1 - beta2) = 3e-7, which two N(0, 1) terms that cancel do reach among 4 million
    elements: there the fp32 rounding of the TERMS (1e-9) moves w by 1e-5 and more in any fp32 implementation, torch's
    included, and no tolerance on w means anything.  The smallest |g| here is 0.01 / 600 (a mean bag of every lookup): sqrt(v') >= 50 eps."""
    rng = np.random.default_rng(seed)
    out = []
    once = np.arange(R - 20, R - 5)
    for k in range(STEPS):
        n_once = 8
        body = rng.integers(0, R - 20, NNZ - 70 - n_once)
        body[body == HOT] = HOT + 1
        ids = np.concatenate([np.full(70, HOT), body, rng.choice(once, n_once, replace=False)])
        ids = ids[rng.permutation(NNZ)].astype(np.int64)
        cover = NNZ
        if k == 0:
            keep = ids >= R - 20                                    # (the once rows stay: they are checked by name)
            ids[(rng.random(NNZ) < 0.1) & ~keep] = -1
            cover = NNZ - 7
            ids[cover:] = R - 1                                     # a row named ONLY where no bag covers it
        nb = 120
        cuts = np.sort(rng.integers(0, cover + 1, nb - 1))
        off = np.concatenate([[0], cuts, [cover]]).astype(np.int64)
        mode, psw, hook = "sum", None, 0
        if k == 1 and not src:
            mode = "mean"
        if k == 2 and not src:
            psw = rng.uniform(0.5, 1.5, NNZ).astype(np.float32)
            psw[rng.random(NNZ) < 0.15] = 0.0
            psw[ids == ids[np.isin(ids, once)][0]] = 0.0            # this once-row has g = 0 and still decays
        if k == 4:
            hook = F
        go = (rng.uniform(0.01, 0.03, (nb // F, F, D) if hook else (nb, D)) * rng.choice([-1.0, 1.0], D)).astype(np.float32)
        if k == 5:
            go = torch.from_numpy(go).to(torch.bfloat16).float().numpy()          # what a bf16 grad_out holds
        out.append(dict(ids=ids, off=off, off32=k == 3, mode=mode, psw=psw, hook=hook, go=go, bf16=k == 5))
    return out


def _model(W0, steps):
    R = W0.shape[0]
    W = W0.astype(np.float64)
    M, V = np.zeros_like(W), np.zeros_like(W)
    named = np.zeros(R, bool)
    for t, s in enumerate(steps, 1):
        rows, grads = ref.lookup_grads(s["ids"], s["off"], s["go"], R, mode=s["mode"], psw=s["psw"],
                                       hook_features=s["hook"])
        named[rows] = True
        ref.step(W, M, V, rows, grads, LR, t, BETAS, EPS)
    return W, M, V, named


def _run_entries(W0, steps, src, acc):
    from cachedembedding_amd.functional import presort_window
    L = _lib()
    lib, ptr = L.lib, L.ptr
    R, D = W0.shape
    w = _table(W0)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    code = L.CE_ACC_STEP if acc == "step" else L.CE_ACC_CACHE
    ws = torch.zeros(lib.ce_bag_backward_adam_workspace(R, NNZ, D, code), dtype=torch.uint8, device="cuda")
    for s in steps:
        idx = torch.from_numpy(s["ids"]).cuda()
        off = torch.from_numpy(s["off"]).cuda()
        if s["off32"]:
            off = off.to(torch.int32)
        nb = off.numel() - 1
        go = torch.from_numpy(s["go"]).cuda()
        if s["bf16"]:
            go = go.to(torch.bfloat16)
        act = L.ACT_DTYPES[go.dtype]
        psw = None if s["psw"] is None else torch.from_numpy(s["psw"]).cuda()
        tail = (BETAS[0], BETAS[1], LR, None, EPS, ptr(step), code, ptr(ws), ws.numel(), _stream())
        if src:
            keys = presort_window(idx.view(1, -1), R, offsets=off, include_last_offset=True, hook_features=s["hook"])[0]
            L.check(lib.ce_bag_backward_adam_src(ptr(w), R, D, NNZ, ptr(go), act, ptr(keys.keys), *tail))
        else:
            L.check(lib.ce_bag_backward_adam(ptr(w), R, D, ptr(idx), NNZ, ptr(off), int(off.dtype == torch.int64), nb, 1,
                                             ptr(psw), L.CE_MODE_MEAN if s["mode"] == "mean" else L.CE_MODE_SUM, s["hook"],
                                             ptr(go), act, None, *tail))
    torch.cuda.synchronize()
    assert int(step.item()) == len(steps)                           # *step has counted the calls
    if acc == "cache":
        assert not ws.any()                                          # the workspace is left zero-filled
    return w.cpu().numpy()


@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("D", DIMS)
def test_update_entries_against_the_fp64_model(D, R, src):
    rng = np.random.default_rng(100 * D + R)
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    steps = _steps(R, D, src, seed=D + R)
    W, M, V, named = _model(W0, steps)
    assert not named[R - 5:].any() and named[R - 20:R - 5].any() and named[HOT]
    got = {}
    for acc in ("cache", "step"):
        t = _run_entries(W0, steps, src, acc)
        got[acc] = t
        w, m, v = t[:, :D], t[:, D:2 * D], t[:, 2 * D:]
        for name, g, want in (("w", w, W), ("m", m, M), ("v", v, V)):
            err = np.abs(g - want) - RTOL * np.abs(want)
            print(f"D={D} R={R} {'src' if src else 'slots'} {acc} {name}: max (|err| - rtol |ref|) = {err.max():.3g}")
            np.testing.assert_allclose(g, want, rtol=RTOL, atol=ATOL, err_msg=f"{acc} {name}")
        # rows no lookup names: bit for bit (the row in the uncovered tail among them)
        np.testing.assert_array_equal(w[~named].view(np.uint32), W0[~named].view(np.uint32))
        assert not m[~named].any() and not v[~named].any()
    # rows looked up at most once per step: one atomic add onto zero is exact, so the accumulators agree bit for bit
    once = np.arange(R - 20, R - 5)
    assert named[once].any()
    np.testing.assert_array_equal(got["cache"][once].view(np.uint32), got["step"][once].view(np.uint32))


# ---- the forwards: bit-equal to the fp32 siblings over the contiguous w parts ---------------------------------------

@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", DIMS)
def test_forwards_equal_the_fp32_forwards_bit_for_bit(D, out_dtype):
    from cachedembedding_amd.functional import presort_window
    L = _lib()
    lib, ptr = L.lib, L.ptr
    act = L.ACT_DTYPES[out_dtype]
    rng = np.random.default_rng(D)
    for R in ROWS:
        W0 = rng.standard_normal((R, D)).astype(np.float32)
        table = _table(W0, fill=float("nan"))                       # a stray read of a moment shows
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
            for fn, w in ((lib.ce_bag_forward_adam, table), (lib.ce_bag_forward_act, plain)):
                o = torch.full((nb, D), 7.0, dtype=out_dtype, device="cuda")
                L.check(fn(ptr(w), R, D, ptr(idx), n, ptr(off), int(off is not None and off.dtype == torch.int64), nb, 1,
                           ptr(p), mode, hook, ptr(o), act, _stream()))
                outs.append(o)
            assert torch.equal(outs[0].view(torch.int32 if out_dtype == torch.float32 else torch.int16),
                               outs[1].view(torch.int32 if out_dtype == torch.float32 else torch.int16)), (name, R)
            assert not torch.isnan(outs[0].float()).any()
        keys = presort_window(idx.view(1, -1), R, offsets=arange.to(torch.int32), include_last_offset=True,
                              hook_features=0, identity_bags=True)[0]
        outs = []
        for fn, w in ((lib.ce_bag_forward_src_keys_adam, table), (lib.ce_bag_forward_src_keys_act, plain)):
            o = torch.full((n, D), 7.0, dtype=out_dtype, device="cuda")
            L.check(fn(ptr(w), R, D, n, ptr(keys.keys), ptr(o), act, _stream()))
            outs.append(o)
        assert torch.equal(outs[0].view(torch.int16 if out_dtype == torch.bfloat16 else torch.int32),
                           outs[1].view(torch.int16 if out_dtype == torch.bfloat16 else torch.int32)), ("src keys", R)
        assert (outs[0][idx < 0] == 0).all()                        # an ignored key: a zero row
        torch.cuda.synchronize()
        assert torch.isnan(table[:, D:]).all() and torch.equal(table[:, :D], plain)      # the forward writes nothing


# ---- through the cache: the moments leave for the host and come back ------------------------------------------------

def _check_against_sparse_adam(emb, W0, steps, use_psw, untouched):
    emb.flush()
    torch.cuda.synchronize()
    w, m, v = cases.sparse_adam_run(W0, steps, torch.float64, use_psw=use_psw)
    for name, got, want in (("weight", emb.weight, w), ("exp_avg", emb.exp_avg, m), ("exp_avg_sq", emb.exp_avg_sq, v)):
        assert tuple(got.shape) == (cases.N, cases.D)
        np.testing.assert_allclose(got.numpy().astype(np.float64), want, rtol=RTOL, atol=ATOL, err_msg=name)
    np.testing.assert_array_equal(emb.weight.numpy()[untouched].view(np.uint32), W0[untouched].view(np.uint32))
    assert not emb.exp_avg.numpy()[untouched].any() and not emb.exp_avg_sq.numpy()[untouched].any()
    assert emb.exp_avg.numpy()[:40].any()


@pytest.mark.parametrize("strategy", ["LFU", "LRU"])
def test_moments_survive_eviction_and_admission(strategy):
    import cachedembedding_amd as ce
    steps = cases.zipf_steps(seed=21, max_unique=6)
    emb = ce.CachedEmbeddingBag(cases.N, cases.D, mode="sum", include_last_offset=True, cuda_row_num=8,
                                evict_strategy=getattr(ce.EvictionStrategy, strategy), fused_optimizer="adam",
                                init_seed=77)
    assert tuple(emb.cache_weight_mgr.cuda_cached_weight.shape) == (8, 3 * cases.D) and emb.embedding_dim == cases.D
    W0 = emb.weight.clone().numpy()
    emb.set_fused_adam(cases.LR, cases.BETAS, cases.EPS)
    for ids, off, go, psw in steps:
        out = emb(torch.from_numpy(ids).cuda(), torch.from_numpy(off).cuda(),
                  per_sample_weights=torch.from_numpy(psw).cuda())
        out.backward(torch.from_numpy(go).cuda())
    assert emb.cache_weight_mgr.cuda_cached_weight.grad is None
    assert int(emb.adam_step.item()) == len(steps)
    # evictions at every step after the first (whose rows the warm-up had preloaded)
    assert sum(n > 0 for n in emb.num_write_back_history) >= len(steps) - 1, emb.num_write_back_history
    _check_against_sparse_adam(emb, W0, steps, True, np.arange(40, cases.N))


def test_moments_through_a_prefetch_window_with_source_row_keys():
    import cachedembedding_amd as ce
    from cachedembedding_amd.pipeline import PrefetchWindow
    steps = cases.zipf_steps(seed=22, max_unique=4)
    off_np = steps[0][1]
    steps = [(ids, off_np, go[:len(off_np) - 1], psw) for ids, _, go, psw in steps]      # one bag layout for the window
    emb = ce.CachedEmbeddingBag(cases.N, cases.D, mode="sum", include_last_offset=True, cuda_row_num=8,
                                evict_strategy=ce.EvictionStrategy.LFU, fused_optimizer="adam", init_seed=78)
    W0 = emb.weight.clone().numpy()
    emb.set_fused_adam(cases.LR, cases.BETAS, cases.EPS, accumulator="cache")
    emb.set_cache_op(False)
    off = torch.from_numpy(off_np).to(torch.int32).cuda()
    win = PrefetchWindow(emb, 2, presort=True, bag_layout=(off, True, 0))
    for k in range(0, len(steps), 2):
        slots = win.prepare([torch.from_numpy(s[0]).cuda() for s in steps[k:k + 2]])
        for i in range(2):
            assert type(win.keys[i]).__name__ == "SrcKeys"
            out = emb(slots[i], off, presorted=win.keys[i])
            out.backward(torch.from_numpy(steps[k + i][2]).cuda())
    assert int(emb.adam_step.item()) == len(steps)
    assert sum(emb.num_write_back_history) > 0
    _check_against_sparse_adam(emb, W0, steps, False, np.arange(40, cases.N))


# ---- a captured step, replayed with three learning rates ----------------------------------------------------------------

def test_captured_step_follows_the_rate_and_counts_its_steps():
    from cachedembedding_amd.functional import FusedAdam, embedding_bag
    rng = np.random.default_rng(9)
    R, D, n = 70, 128, 96
    lrs = [0.05, 0.0125, 0.2]
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    ids = np.concatenate([rng.permutation(R - 5)[:n // 2]] * 2)       # every row at most twice: the atomics cannot reorder
    idx = torch.from_numpy(ids[rng.permutation(n)].astype(np.int64)).cuda()
    off = torch.arange(0, n + 1, 2, dtype=torch.int64, device="cuda")
    go = torch.from_numpy(rng.standard_normal((n // 2, D)).astype(np.float32)).cuda()

    def one_step(w, fused):
        w.requires_grad_(True)
        out = embedding_bag(idx, w, off, mode="sum", include_last_offset=True, fused_sgd=fused)
        out.backward(go)
        assert w.grad is None

    we = _table(W0)
    fe = FusedAdam(lrs[0], step=torch.zeros(1, dtype=torch.int64, device="cuda"))
    eager = []
    for lr in lrs:
        fe.lr = lr
        one_step(we, fe)
        eager.append(we.detach().clone())

    lr_t = torch.full((1,), lrs[0], dtype=torch.float32, device="cuda")
    wg = _table(W0)
    fg = FusedAdam(lr_t, step=torch.zeros(1, dtype=torch.int64, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_step(wg, fg)                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():                                            # back to the start: table, moments, step count
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
    assert int(fg.step.item()) == 3 and int(fe.step.item()) == 3


# ---- initialisation and the module's refusals ---------------------------------------------------------------------------

def test_initialisation_equals_the_plain_module_and_refusals():
    import cachedembedding_amd as ce
    a = ce.CachedEmbeddingBag(cases.N, cases.D, mode="sum", cuda_row_num=8, fused_optimizer="adam", init_seed=4242)
    p = ce.CachedEmbeddingBag(cases.N, cases.D, mode="sum", cuda_row_num=8, init_seed=4242)
    assert torch.equal(a.weight.view(torch.int32), p.weight.view(torch.int32)) and a.weight.abs().sum() > 0
    assert not a.exp_avg.any() and not a.exp_avg_sq.any() and int(a.adam_step.item()) == 0
    w = torch.randn(cases.N, 16)
    f = ce.CachedEmbeddingBag.from_pretrained(w, freeze=False, cuda_row_num=8, mode="sum", fused_optimizer="adam")
    assert torch.equal(f.weight, w) and not f.exp_avg.any() and not f.exp_avg_sq.any()
    for call in (lambda: a.set_fused_sgd(0.1), lambda: a.set_fused_rowwise_adagrad(0.1)):
        with pytest.raises(NotImplementedError, match="Adam-layout"):
            call()
    with pytest.raises(ValueError, match="fused_optimizer='adam'"):
        p.set_fused_adam(0.1)
    with pytest.raises(NotImplementedError, match="deterministic"):
        a.set_fused_adam(0.1, deterministic=True)
    with pytest.raises(AttributeError):
        p.exp_avg
    # eval-mode forward needs no optimizer; a backward without one is refused in backward
    ids = torch.arange(6, device="cuda")
    off = torch.arange(0, 7, 2, device="cuda")
    a.eval()
    with torch.no_grad():
        out = a(ids, off)
    want = torch.nn.functional.embedding_bag(ids.cpu(), a.weight, off.cpu(), mode="sum")
    torch.testing.assert_close(out.cpu(), want, rtol=1e-6, atol=1e-7)
    a.train()
    out = a(ids, off)
    with pytest.raises(RuntimeError, match="no fused Adam set"):
        out.sum().backward()
    # quantized() quantizes the w parts
    q = f.quantized(cuda_row_num=8)
    with torch.no_grad():
        oq = q(ids, off)
    torch.testing.assert_close(oq.cpu(), torch.nn.functional.embedding_bag(ids.cpu(), w, off.cpu(), mode="sum"),
                               rtol=0, atol=3 * float(w.abs().max()) / 255 * 2)


def test_dlrm_example_trains_with_adam(capsys):
    """examples/dlrm_main.py --adam end to end: prefetch windows with source-row keys, the fused Adam on the embedding,
    torch.optim.Adam on the dense part; the moments are in the host table afterwards"""
    import importlib
    import cachedembedding_amd as ce
    sys.path.insert(0, str(HERE.parent / "examples"))
    dm = importlib.import_module("dlrm_main")
    seen = []
    orig = ce.CachedEmbeddingBag.set_fused_adam

    def spy(self, *a, **kw):
        seen.append(self)
        return orig(self, *a, **kw)
    ce.CachedEmbeddingBag.set_fused_adam = spy
    try:
        dm.main(["--dataset", "avazu", "--table_scale", "0.01", "--batch_size", "256", "--embedding_dim", "32",
                 "--dense_arch_layer_sizes", "64,32", "--over_arch_layer_sizes", "64,1", "--use_cache", "--cache_ratio",
                 "0.03", "--use_freq", "--prefetch_num", "4", "--use_overlap", "--overlap_cache_op", "--adam", "--fold_hook",
                 "--window_keys", "--limit_train_batches", "16", "--learning_rate", "0.01"])
    finally:
        ce.CachedEmbeddingBag.set_fused_adam = orig
    emb = seen[0]
    assert emb.fused_optimizer == "adam" and int(emb.adam_step.item()) == 16
    emb.flush()
    assert emb.exp_avg.abs().sum() > 0 and emb.exp_avg_sq.abs().sum() > 0 and torch.isfinite(emb.weight).all()
