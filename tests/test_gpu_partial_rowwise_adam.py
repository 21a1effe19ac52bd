"""GPU tests of partial row-wise Adam (rows w | m, one second moment per table row): the forwards bit
for bit against their fp32 siblings, the update entries bit for bit against the Adam-layout entries where the two
arithmetics coincide and within the project's Adam tolerance of the fp64 model (tests/partial_rowwise_adam_ref.py)
everywhere else, slots outside the second moment, the module through an evicting cache, a prefetch window, a captured
step, and resuming from saved state."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import adam_cases as cases  # noqa: E402
import partial_rowwise_adam_cases as kc  # noqa: E402
import partial_rowwise_adam_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6           # the project's Adam tolerance; the fp32 reference alone keeps it on these inputs
                                  # (tests/test_partial_rowwise_adam_cpu.py)
LAYOUT = "partial_rowwise_adam"
# one lane | two | 8 | 16 | 32 lanes | 48 chunks on 64 lanes: masked chunks in the sum of squares | 64 lanes | 2 and 4
# chunks per lane
DIMS = [4, 8, 32, 64, 128, 192, 256, 512, 1024]
R, NNZ, NB, F = kc.R, kc.NNZ, kc.NB, kc.F
WD_MODES = {None: 0, "l2": 1, "decoupled": 2}


def _lib():
    from cachedembedding_amd import _lib as L
    return L


def _stream():
    return _lib().stream_ptr()


def _table(W0, span=2, fill=0.0):
    """[R, span D] device table with the w parts W0 and the moments `fill`"""
    n, D = W0.shape
    t = torch.full((n, span * D), fill, dtype=torch.float32)
    t[:, :D] = torch.from_numpy(W0)
    return t.cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the forwards: bit-equal to the fp32 entries over the contiguous w parts ---------------------------------------

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
    table = _table(W0, fill=float("nan"))                           # a stray read of an m part shows
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
        for fn, w in ((lib.ce_bag_forward_pradam, table), (lib.ce_bag_forward_act, plain)):
            o = torch.full((nb, D), 7.0, dtype=out_dtype, device="cuda")
            L.check(fn(ptr(w), R, D, ptr(idx), n, ptr(off), int(off is not None and off.dtype == torch.int64), nb, 1,
                       ptr(p), mode, hook, ptr(o), act, _stream()))
            outs.append(o)
        assert torch.equal(outs[0].view(as_int), outs[1].view(as_int)), name
        assert not torch.isnan(outs[0].float()).any()
    keys = presort_window(idx.view(1, -1), R, offsets=arange.to(torch.int32), include_last_offset=True,
                          hook_features=0, identity_bags=True)[0]
    outs = []
    for fn, w in ((lib.ce_bag_forward_src_keys_pradam, table), (lib.ce_bag_forward_src_keys_act, plain)):
        o = torch.full((n, D), 7.0, dtype=out_dtype, device="cuda")
        L.check(fn(ptr(w), R, D, n, ptr(keys.keys), ptr(o), act, _stream()))
        outs.append(o)
    assert torch.equal(outs[0].view(as_int), outs[1].view(as_int)), "src keys"
    assert (outs[0][idx < 0] == 0).all()                            # an ignored key: a zero row
    torch.cuda.synchronize()
    assert torch.isnan(table[:, D:]).all() and torch.equal(table[:, :D], plain)      # the forward writes nothing


# ---- the update entries ----------------------------------------------------------------------------------------------

def _call_update(w, D, s, src, acc_code, ws, step, layout, lr, lr_dev=None, v=None, row_of=None, wd=0.0, wd_mode=None):
    """one call of ce_bag_backward_pradam* (layout "partial_rowwise_adam") or ce_bag_backward_adam* ("adam") for the
    step dict s (ids, off, off32, mode, psw, hook, go, act)"""
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
    rate = (BETAS[0], BETAS[1], 0.0 if lr_dev is not None else lr, ptr(lr_dev), EPS)
    end = (ptr(step), acc_code, ptr(ws), ws.numel(), _stream())
    if layout == LAYOUT:
        tail = (ptr(row_of), ptr(v), v.numel()) + rate + (wd, WD_MODES[wd_mode]) + end
        fn_src, fn = lib.ce_bag_backward_pradam_src, lib.ce_bag_backward_pradam
    else:
        tail = rate + end
        fn_src, fn = lib.ce_bag_backward_adam_src, lib.ce_bag_backward_adam
    if src:
        keys = presort_window(idx.view(1, -1), n_rows, offsets=off, include_last_offset=True,
                              hook_features=s.get("hook", 0))[0]
        L.check(fn_src(ptr(w), n_rows, D, nnz, ptr(go), act, ptr(keys.keys), *tail))
    else:
        L.check(fn(ptr(w), n_rows, D, ptr(idx), nnz, ptr(off), int(off.dtype == torch.int64), nb, 1, ptr(psw),
                   L.CE_MODE_MEAN if s.get("mode") == "mean" else L.CE_MODE_SUM, s.get("hook", 0), ptr(go), act, None,
                   *tail))


LR, BETAS, EPS = kc.LR, kc.BETAS, kc.EPS


def _workspace(n_rows, nnz, D, acc):
    L = _lib()
    code = L.CE_ACC_STEP if acc == "step" else L.CE_ACC_CACHE
    need = L.lib.ce_bag_backward_pradam_workspace(n_rows, nnz, D, code)
    assert need == L.lib.ce_bag_backward_adam_workspace(n_rows, nnz, D, code)
    return code, torch.zeros(need, dtype=torch.uint8, device="cuda")


def _exact_steps(D, seed, n_rows=128, steps=3):
    """every row's folded gradient is +-2^e in every element times 1, 2 or 4: row r is looked up k_r in {1, 2, 4} times
    by one-lookup bags that share ONE gradient row sigma * 2^(e_r).  Every sum and every square sum is exact in fp32
    whatever the order, so the mean of the squares IS each element's square and Adam's per-element v is the row's
    scalar in every column.  The last 8 rows are never looked up."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        rows = rng.permutation(n_rows - 8)[:96]
        mult = rng.choice([1, 2, 4], len(rows))
        e = rng.integers(-6, 3, len(rows))
        sigma = rng.choice([-1.0, 1.0], (len(rows), D))
        ids = np.repeat(rows, mult)
        go = np.repeat(sigma * np.exp2(e)[:, None], mult, axis=0).astype(np.float32)
        p = rng.permutation(len(ids))
        out.append(dict(ids=ids[p].astype(np.int64), off=np.arange(len(ids) + 1, dtype=np.int64), go=go[p]))
    return out


@pytest.mark.parametrize("D", DIMS)
def test_update_is_bit_equal_to_the_adam_entry_on_gradients_of_one_magnitude(D):
    """no tolerance: a wrong reduction, a wrong mean or a wrong stride cannot hide.  Three consecutive steps, both
    accumulators, both entry forms; the second moment is indexed through a row_of_slot that is no identity."""
    n_rows = 128
    steps = _exact_steps(D, seed=D)
    W0 = np.random.default_rng(D + 1).standard_normal((n_rows, D)).astype(np.float32)
    row_of_np = np.random.default_rng(D + 2).permutation(n_rows).astype(np.int32)
    row_of = torch.from_numpy(row_of_np).cuda()
    nnz_max = max(len(s["ids"]) for s in steps)
    assert nnz_max <= 2048
    for acc in ("cache", "step"):
        for src in (False, True):
            wa, wp = _table(W0, span=3), _table(W0, span=2)
            v = torch.zeros(n_rows, dtype=torch.float32, device="cuda")
            sa = torch.zeros(1, dtype=torch.int64, device="cuda")
            sp = torch.zeros(1, dtype=torch.int64, device="cuda")
            for k, s in enumerate(steps):
                nnz = len(s["ids"])
                code, ws = _workspace(n_rows, nnz, D, acc)
                _call_update(wa, D, s, src, code, ws, sa, "adam", LR)
                _call_update(wp, D, s, src, code, ws, sp, LAYOUT, LR, v=v, row_of=row_of)
                torch.cuda.synchronize()
                a, p, vv = wa.cpu().numpy(), wp.cpu().numpy(), v.cpu().numpy()
                tag = f"D={D} {acc} {'src' if src else 'slots'} step {k}"
                np.testing.assert_array_equal(_bits(p[:, :D]), _bits(a[:, :D]), err_msg=f"w {tag}")
                np.testing.assert_array_equal(_bits(p[:, D:]), _bits(a[:, D:2 * D]), err_msg=f"m {tag}")
                np.testing.assert_array_equal(_bits(np.repeat(vv[row_of_np][:, None], D, axis=1)), _bits(a[:, 2 * D:]),
                                              err_msg=f"v {tag}")
                assert acc == "step" or not ws.any(), tag            # the cache-sized workspace is left zero-filled
            assert int(sp.item()) == 3 and int(sa.item()) == 3
            assert vv.any() and not vv[row_of_np[n_rows - 8:]].any()
            np.testing.assert_array_equal(_bits(p[n_rows - 8:, :D]), _bits(W0[n_rows - 8:]))


def _run_entries(W0, steps, src, acc, wd_mode, lr_dev):
    D = W0.shape[1]
    w = _table(W0)
    v = torch.zeros(R, dtype=torch.float32, device="cuda")
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    code, ws = _workspace(R, NNZ, D, acc)
    lr_t = torch.zeros(1, dtype=torch.float32, device="cuda") if lr_dev else None
    for s in steps:
        if lr_dev:
            lr_t.fill_(s["lr"])                                      # the rate as a tensor, changed between steps
        _call_update(w, D, s, src, code, ws, step, LAYOUT, s["lr"], lr_dev=lr_t, v=v, wd=kc.WD if wd_mode else 0.0,
                     wd_mode=wd_mode)
    torch.cuda.synchronize()
    assert int(step.item()) == len(steps)
    if acc == "cache":
        assert not ws.any()
    return w.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("wd_mode", [None, "l2", "decoupled"])
@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
@pytest.mark.parametrize("D", DIMS)
def test_update_entries_against_the_fp64_model(D, src, wd_mode):
    """both accumulators; sum, mean, per-sample weights with zeros, ragged and empty bags, hook_features, an ignored
    lookup, lookups no bag covers, fp32 / bf16 / fp16 gradients (kernel_steps); the rate by value (slots) or as a
    tensor (src), changed between steps"""
    W0 = kc.initial_weight(D, D)
    steps = kc.kernel_steps(D, src, seed=D)
    W, M, V, named = kc.model(W0, steps, wd=kc.WD if wd_mode else 0.0, wd_mode=wd_mode or "l2")
    assert not named[R - 5:].any() and named[R - 20:R - 5].any() and named[kc.HOT]
    got = {}
    for acc in ("cache", "step"):
        t, v = _run_entries(W0, steps, src, acc, wd_mode, lr_dev=src)
        got[acc] = (t, v)
        for name, g, want in (("w", t[:, :D], W), ("m", t[:, D:], M), ("v", v, V)):
            err = np.abs(g - want) / (ATOL + RTOL * np.abs(want))
            print(f"D={D} {'src' if src else 'slots'} wd={wd_mode} {acc} {name}: max |err| / (atol + rtol |ref|) = "
                  f"{err.max():.3g}")
            np.testing.assert_allclose(g, want, rtol=RTOL, atol=ATOL, err_msg=f"{acc} {name}")
        # rows no lookup names -- the row in the uncovered tail among them: bit for bit, decay or not
        np.testing.assert_array_equal(_bits(t[~named, :D]), _bits(W0[~named]))
        assert not t[~named, D:].any() and not v[~named].any()
    # rows looked up at most once per step: one atomic add onto zero is exact, so the accumulators agree bit for bit
    once = np.arange(R - 20, R - 5)
    np.testing.assert_array_equal(_bits(got["cache"][0][once]), _bits(got["step"][0][once]))
    np.testing.assert_array_equal(_bits(got["cache"][1][once]), _bits(got["step"][1][once]))


@pytest.mark.parametrize("wd_mode", ["l2", "decoupled"])
@pytest.mark.parametrize("D", [128, 192])
def test_slots_outside_the_second_moment_are_left_alone(D, wd_mode):
    """row_of_slot -1 or beyond v_rows: the slot keeps w and m bit for bit, with decay on (row-wise Adagrad's rule)"""
    n_rows, v_rows = 70, 40
    rng = np.random.default_rng(D)
    W0 = rng.standard_normal((n_rows, D)).astype(np.float32)
    M0 = rng.standard_normal((n_rows, D)).astype(np.float32)
    row_of_np = np.arange(n_rows, dtype=np.int32)                     # slots [40, 70) lie beyond v_rows ...
    row_of_np[:6] = -1                                                # ... and slots [0, 6) map to no row
    row_of_np[6:12] = [45, 69, 1 << 20, v_rows, 2 ** 31 - 1, -7]
    inside = (row_of_np >= 0) & (row_of_np < v_rows)
    ids = np.concatenate([np.arange(n_rows), rng.integers(0, n_rows, 130)]).astype(np.int64)      # every slot is named
    s = dict(ids=ids, off=np.arange(0, 201, 2, dtype=np.int64),
             go=(rng.uniform(0.01, 0.03, (100, D)) * rng.choice([-1.0, 1.0], D)).astype(np.float32))
    for acc in ("cache", "step"):
        for src in (False, True):
            w = _table(W0)
            w[:, D:] = torch.from_numpy(M0).cuda()
            v = torch.full((v_rows,), 0.25, dtype=torch.float32, device="cuda")
            step = torch.zeros(1, dtype=torch.int64, device="cuda")
            code, ws = _workspace(n_rows, len(ids), D, acc)
            _call_update(w, D, s, src, code, ws, step, LAYOUT, LR, v=v, row_of=torch.from_numpy(row_of_np).cuda(),
                         wd=0.1, wd_mode=wd_mode)
            torch.cuda.synchronize()
            t, vv = w.cpu().numpy(), v.cpu().numpy()
            np.testing.assert_array_equal(_bits(t[~inside, :D]), _bits(W0[~inside]))
            np.testing.assert_array_equal(_bits(t[~inside, D:]), _bits(M0[~inside]))
            assert (t[inside, :D] != W0[inside]).any(axis=1).all() and (t[inside, D:] != M0[inside]).any(axis=1).all()
            moved = np.zeros(v_rows, bool)
            moved[row_of_np[inside]] = True
            assert (vv[moved] != 0.25).all() and (vv[~moved] == 0.25).all()
            assert (acc == "step" or not ws.any()) and int(step.item()) == 1


# ---- through the module ----------------------------------------------------------------------------------------------

def _module(cuda_row_num, seed=77, freq=None, strategy="LFU"):
    import cachedembedding_amd as ce
    return ce.CachedEmbeddingBag(cases.N, cases.D, mode="sum", include_last_offset=True, cuda_row_num=cuda_row_num,
                                 evict_strategy=getattr(ce.EvictionStrategy, strategy), fused_optimizer=LAYOUT,
                                 init_seed=seed, ids_freq_mapping=freq)


def _train(emb, steps, use_psw=True):
    for ids, off, go, psw in steps:
        out = emb(torch.from_numpy(ids).cuda(), torch.from_numpy(off).cuda(),
                  per_sample_weights=torch.from_numpy(psw).cuda() if use_psw else None)
        out.backward(torch.from_numpy(go).cuda())


def _state(emb):
    """(w [N, D], m [N, D], v [N]) numpy in ROW space after a flush"""
    emb.flush()
    torch.cuda.synchronize()
    assert emb.exp_avg_sq.is_cuda and tuple(emb.exp_avg_sq.shape) == (cases.N,) and emb.exp_avg_sq.dtype == torch.float32
    assert tuple(emb.weight.shape) == (cases.N, cases.D) and tuple(emb.exp_avg.shape) == (cases.N, cases.D)
    return emb.weight.clone().numpy(), emb.exp_avg.clone().numpy(), emb.exp_avg_sq.cpu().numpy()


def _reference(W0, steps, use_psw=True, lr=cases.LR, **kw):
    W = W0.astype(np.float64)
    M, V = np.zeros_like(W), np.zeros(cases.N)
    for t, (ids, off, go, psw) in enumerate(steps, 1):
        rows, grads = ref.lookup_grads(ids, off, go, cases.N, psw=psw if use_psw else None)
        ref.step(W, M, V, rows, grads, lr, t, cases.BETAS, cases.EPS, **kw)
    return W, M, V


def test_module_through_an_evicting_cache_with_a_reordered_table():
    """a cache of u + 2 rows evicts at every step and sees rows again; against a cache that holds everything and against
    the reference.  ids_freq_mapping (DATASET) makes idx_map no identity: exp_avg_sq is indexed by host row like weight."""
    u = 6
    steps = cases.zipf_steps(seed=21, max_unique=u)
    freq = torch.from_numpy(np.random.default_rng(1).permutation(cases.N).astype(np.int64))
    small, big = _module(u + 2, freq=freq, strategy="DATASET"), _module(cases.N, freq=freq, strategy="DATASET")
    assert tuple(small.cache_weight_mgr.cuda_cached_weight.shape) == (u + 2, 2 * cases.D) and small.embedding_dim == cases.D
    row_of_id = small.cache_weight_mgr.idx_map.cpu().numpy().astype(np.int64)
    assert (row_of_id != np.arange(cases.N)).any()
    assert np.array_equal(row_of_id, big.cache_weight_mgr.idx_map.cpu().numpy())
    W0 = small.weight.clone().numpy()[row_of_id]                    # row space -> id space
    assert not small.exp_avg.any() and not small.exp_avg_sq.any()
    for emb in (small, big):
        emb.set_fused_adam(cases.LR, cases.BETAS, cases.EPS, weight_decay=0.01, weight_decay_mode="decoupled")
        _train(emb, steps)
        assert emb.cache_weight_mgr.cuda_cached_weight.grad is None and int(emb.adam_step.item()) == len(steps)
    assert sum(n > 0 for n in small.num_write_back_history) >= len(steps) - 1, small.num_write_back_history
    want = _reference(W0, steps, wd=0.01, wd_mode="decoupled")
    got_small = [x[row_of_id] for x in _state(small)]
    got_big = [x[row_of_id] for x in _state(big)]
    for name, a, b, w in zip(("weight", "exp_avg", "exp_avg_sq"), got_small, got_big, want):
        np.testing.assert_allclose(a.astype(np.float64), w, rtol=RTOL, atol=ATOL, err_msg=name)
        np.testing.assert_allclose(b.astype(np.float64), w, rtol=RTOL, atol=ATOL, err_msg=f"{name}, everything cached")
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, err_msg=f"{name}, evicting against everything cached")
    untouched = np.arange(40, cases.N)
    w, m, v = got_small
    np.testing.assert_array_equal(_bits(w[untouched]), _bits(W0[untouched]))
    assert not m[untouched].any() and not v[untouched].any() and v[:40].any() and m[:40].any()


def test_prefetch_window_step_equals_eager_steps():
    from cachedembedding_amd.pipeline import PrefetchWindow
    steps = cases.zipf_steps(seed=22, max_unique=4)
    off_np = steps[0][1]
    steps = [(ids, off_np, go[:len(off_np) - 1], psw) for ids, _, go, psw in steps]      # one bag layout for the window
    eager, emb = _module(8, seed=78), _module(8, seed=78)
    W0 = emb.weight.clone().numpy()
    for e in (eager, emb):
        e.set_fused_adam(cases.LR, cases.BETAS, cases.EPS, accumulator="cache")
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
    assert int(emb.adam_step.item()) == len(steps) and sum(emb.num_write_back_history) > 0
    want = _reference(W0, steps, use_psw=False)
    got, got_eager = _state(emb), _state(eager)
    for name, g, e, w in zip(("weight", "exp_avg", "exp_avg_sq"), got, got_eager, want):
        np.testing.assert_allclose(g.astype(np.float64), w, rtol=RTOL, atol=ATOL, err_msg=name)
        np.testing.assert_allclose(g, e, rtol=RTOL, atol=ATOL, err_msg=f"{name} against eager")


def test_captured_step_replayed_equals_eager_steps_and_counts_on():
    from cachedembedding_amd.functional import FusedAdam, embedding_bag
    rng = np.random.default_rng(9)
    n_rows, D, n, K = 70, 128, 96, 3
    lrs = [0.05, 0.0125, 0.2]
    W0 = rng.standard_normal((n_rows, D)).astype(np.float32)
    ids = np.concatenate([rng.permutation(n_rows - 5)[:n // 2]] * 2)  # every row at most twice: the atomics cannot reorder
    idx = torch.from_numpy(ids[rng.permutation(n)].astype(np.int64)).cuda()
    off = torch.arange(0, n + 1, 2, dtype=torch.int64, device="cuda")
    go = torch.from_numpy(rng.standard_normal((n // 2, D)).astype(np.float32)).cuda()
    row_of = torch.from_numpy(rng.permutation(n_rows).astype(np.int32)).cuda()

    def fused(lr):
        return FusedAdam(lr, step=torch.zeros(1, dtype=torch.int64, device="cuda"), layout=LAYOUT, row_of_slot=row_of,
                         exp_avg_sq=torch.zeros(n_rows, dtype=torch.float32, device="cuda"))

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
        eager.append((we.detach().clone(), fe.exp_avg_sq.clone()))

    lr_t = torch.full((1,), lrs[0], dtype=torch.float32, device="cuda")
    wg, fg = _table(W0), fused(lr_t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_step(wg, fg)                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():                                            # back to the start: table, moments, step count
        wg.copy_(_table(W0))
        fg.exp_avg_sq.zero_()
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
        assert torch.equal(wg.detach().view(torch.int32), eager[k][0].view(torch.int32)), k
        assert torch.equal(fg.exp_avg_sq.view(torch.int32), eager[k][1].view(torch.int32)), k
    assert int(fg.step.item()) == K and int(fe.step.item()) == K and fg.exp_avg_sq.any()


# ---- resume ----------------------------------------------------------------------------------------------------------

def _unique_steps(seed, steps=6):
    """one id per bag, every row at most once per step: nothing for the atomics to reorder"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        ids = rng.permutation(40)[:6].astype(np.int64)
        go = rng.standard_normal((6, cases.D)).astype(np.float32)
        out.append((ids, np.arange(7, dtype=np.int64), go, np.ones(6, np.float32)))
    return out


@pytest.mark.parametrize("layout", ["adam", LAYOUT])
def test_resume_from_loaded_state(layout):
    import cachedembedding_amd as ce
    k = 3

    def module(w=None):
        return ce.CachedEmbeddingBag(cases.N, cases.D, mode="sum", include_last_offset=True, cuda_row_num=8,
                                     evict_strategy=ce.EvictionStrategy.LFU, fused_optimizer=layout, init_seed=5,
                                     _weight=w)

    for steps, exact in ((cases.zipf_steps(seed=23, steps=2 * k, max_unique=6), False), (_unique_steps(4, 2 * k), True)):
        whole = module()
        whole.set_fused_adam(cases.LR, cases.BETAS, cases.EPS)
        _train(whole, steps)
        first = module()
        first.set_fused_adam(cases.LR, cases.BETAS, cases.EPS)
        _train(first, steps[:k])
        first.flush()
        saved = (first.weight.clone(), first.exp_avg.clone(), first.exp_avg_sq.clone().cpu(), int(first.adam_step.item()))
        assert saved[3] == k
        second = module(saved[0])
        assert not second.exp_avg.any() and not second.exp_avg_sq.any()
        second.load_adam_state(saved[1], saved[2], saved[3])
        assert int(second.adam_step.item()) == k and second.adam_step.is_cuda
        assert torch.equal(second.exp_avg, saved[1]) and torch.equal(second.exp_avg_sq.cpu(), saved[2])
        assert torch.equal(second.weight, saved[0])                  # the weights are not touched
        second.set_fused_adam(cases.LR, cases.BETAS, cases.EPS)
        _train(second, steps[k:])
        assert int(second.adam_step.item()) == 2 * k
        for e in (whole, second):
            e.flush()
        torch.cuda.synchronize()
        for name in ("weight", "exp_avg", "exp_avg_sq"):
            g, w = getattr(second, name).cpu(), getattr(whole, name).cpu()
            np.testing.assert_allclose(g.numpy(), w.numpy(), rtol=RTOL, atol=ATOL, err_msg=name)
            if exact:
                assert torch.equal(g.view(torch.int32), w.view(torch.int32)), name
        with pytest.raises(ValueError, match="exp_avg must be"):
            second.load_adam_state(saved[1][:, :4], saved[2], k)
        with pytest.raises(ValueError, match="exp_avg_sq must be"):
            second.load_adam_state(saved[1], saved[2][:5], k)


# ---- initialisation, the module's refusals, quantization -----------------------------------------------------------------

def test_initialisation_refusals_and_quantization():
    import cachedembedding_amd as ce
    a = _module(8, seed=4242)
    p = ce.CachedEmbeddingBag(cases.N, cases.D, mode="sum", cuda_row_num=8, init_seed=4242)
    assert torch.equal(a.weight.view(torch.int32), p.weight.view(torch.int32)) and a.weight.abs().sum() > 0
    assert tuple(a.cache_weight_mgr.weight.shape) == (cases.N, 2 * cases.D)
    assert not a.exp_avg.any() and not a.exp_avg_sq.any() and int(a.adam_step.item()) == 0
    assert a.exp_avg_sq.device == a.cache_weight_mgr.cuda_cached_weight.device
    w = torch.randn(cases.N, 16)
    f = ce.CachedEmbeddingBag.from_pretrained(w, freeze=False, cuda_row_num=8, mode="sum", fused_optimizer=LAYOUT)
    assert torch.equal(f.weight, w) and not f.exp_avg.any() and not f.exp_avg_sq.any() and f.embedding_dim == 16
    for call in (lambda: a.set_fused_sgd(0.1), lambda: a.set_fused_rowwise_adagrad(0.1)):
        with pytest.raises(NotImplementedError, match="Adam-layout"):
            call()
    with pytest.raises(NotImplementedError, match="deterministic"):
        a.set_fused_adam(0.1, deterministic=True)
    with pytest.raises(ValueError, match="load_adam_state"):
        p.load_adam_state(torch.zeros(cases.N, cases.D), torch.zeros(cases.N), 1)
    with pytest.raises(AttributeError):
        p.exp_avg_sq
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
    with pytest.raises(RuntimeError, match="no fused Adam set"):
        out.sum().backward()
    # quantized() quantizes the w parts
    q = f.quantized(cuda_row_num=8)
    off3 = torch.arange(0, 6, 2, device="cuda")
    with torch.no_grad():
        oq = q(ids, off3)
    torch.testing.assert_close(oq.cpu(), torch.nn.functional.embedding_bag(ids.cpu(), w, off3.cpu(), mode="sum"),
                               rtol=0, atol=3 * float(w.abs().max()) / 255 * 2)
