"""GPU tests of the 16-bit embedding table (bf16 / fp16 rows in the host table and in the cache) against
tests/table_dtype_ref.py: the general and the key-driven forward, the rounding update (nearest and stochastic), the
cache while it evicts, the prefetch windows with a hipGraph replay, and a checkpoint round trip.  The kernels only ever
see in-range slots and the documented ignored slot -1."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import table_dtype_ref as ref  # noqa: E402
from activation_dtype_ref import assert_cast_equal, bag_ref64, forward_bound  # noqa: E402
from test_gpu_rowwise_adagrad import _Track  # noqa: E402  (its tolerances are the Adagrad bound here, no wider)

pytestmark = pytest.mark.gpu
W16 = [torch.bfloat16, torch.float16]
OUT = [torch.float32, torch.bfloat16, torch.float16]
NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _equal_cast(got: torch.Tensor, want32: torch.Tensor) -> None:
    """got == the cast of the fp32 values want32 to got's dtype (exact for fp32: the up-conversion loses nothing)"""
    if got.dtype == torch.float32:
        assert torch.equal(_bits(got), _bits(want32))
    else:
        assert_cast_equal(got.detach().cpu(), want32.to(got.dtype))


# ---- 1. general forward ----------------------------------------------------------------------------------------------

_FWD = {}


def _fwd_case(D, wt):
    """shared inputs of one (D, table type): the table, one-id bags and a multi-id layout, built once"""
    key = (D, wt)
    if key not in _FWD:
        rng = np.random.default_rng(100 + D)
        R, nb = 257, 130
        table = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(wt)
        single = rng.integers(0, R, nb)
        lens = rng.integers(0, 21, nb)
        lens[3], lens[7] = 0, 9                                   # an empty bag, a 9-id bag
        off = np.concatenate([[0], np.cumsum(lens)])
        idx = rng.integers(0, R, int(off[-1]))
        idx[int(off[7]) + 2] = -1                                 # one ignored lookup
        psw = rng.random(len(idx)).astype(np.float32) + 0.5
        _FWD[key] = dict(R=R, nb=nb, table=table, single=single, off=off, idx=idx, psw=psw, refs={})
    return _FWD[key]


@pytest.mark.parametrize("ot", OUT, ids=lambda d: "out_" + NAMES[d])
@pytest.mark.parametrize("wt", W16, ids=lambda d: "table_" + NAMES[d])
@pytest.mark.parametrize("D", [8, 40, 128, 264])
def test_general_forward(D, wt, ot):
    from cachedembedding_amd.functional import embedding_bag
    c = _fwd_case(D, wt)
    w = c["table"].cuda()
    nb = c["nb"]
    # (a) one id per bag, sum: the cast of the row
    ids = torch.from_numpy(c["single"]).cuda()
    for hook in (0, 5):
        out = embedding_bag(ids, w, torch.arange(nb + 1, device="cuda"), mode="sum", include_last_offset=True,
                            hook_features=hook, output_dtype=ot)
        rows = c["table"][torch.from_numpy(c["single"])].float()
        if hook:
            rows = rows.view(hook, nb // hook, D).transpose(0, 1).contiguous()       # bag f * B + b -> [b, f]
        _equal_cast(out.view(-1, D), rows.view(-1, D))
    # (b) bags of 0..20 ids
    idx = torch.from_numpy(c["idx"]).cuda()
    t32 = c["table"].float().numpy()
    for mode, use_psw in (("sum", False), ("sum", True), ("mean", False)):
        for hook in (0, 5):
            rk = (mode, use_psw, hook)
            if rk not in c["refs"]:
                c["refs"][rk] = bag_ref64(t32, c["idx"], c["off"], c["psw"] if use_psw else None, mode, True, hook)
            r64, asum, L = c["refs"][rk]
            for odt in (torch.int32, torch.int64):
                out = embedding_bag(idx, w, torch.from_numpy(c["off"]).to(odt).cuda(), mode=mode,
                                    include_last_offset=True, hook_features=hook, output_dtype=ot,
                                    per_sample_weights=torch.from_numpy(c["psw"]).cuda() if use_psw else None,
                                    masked_indices=mode == "sum")
                assert out.dtype == ot
                got = out.detach().cpu().double().numpy().reshape(r64.shape)
                if ot == torch.float32:
                    bound = np.asarray(L, np.float64).reshape(-1, 1) * ref.U32 * asum        # the fp32 term alone
                else:
                    bound = forward_bound(r64, asum, L, ot)
                bad = int((np.abs(got - r64) > bound).sum())
                assert bad == 0, (mode, use_psw, hook, odt, bad)


def test_forward_defaults_to_the_tables_dtype():
    from cachedembedding_amd.functional import embedding_bag
    c = _fwd_case(8, torch.bfloat16)
    out = embedding_bag(torch.from_numpy(c["single"]).cuda(), c["table"].cuda(),
                        torch.arange(c["nb"] + 1, device="cuda"), mode="sum", include_last_offset=True)
    assert out.dtype == torch.bfloat16


# ---- 2. key-driven forward -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wt", W16, ids=lambda d: "table_" + NAMES[d])
@pytest.mark.parametrize("nnz", [300, 16384 + 5])
def test_key_driven_forward(nnz, wt):
    """one partial segment / two segments with padding, two batches.  hook_features must divide the number of bags:
    4 for 300 bags, 3 for 16389 (which 4 does not divide)."""
    from cachedembedding_amd.functional import embedding_bag, presort_window
    rng = np.random.default_rng(nnz)
    R, D, P = 257, 64, 2
    t = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(wt)
    t[5, 0], t[5, 1], t[5, 2] = -0.0, float("inf"), torch.finfo(wt).max
    t[6, 3] = -torch.finfo(wt).max
    w = t.cuda()
    slots = rng.integers(0, R, (P, nnz))
    slots[:, :8] = [5, 6, 5, 5, 6, 0, 256, 5]
    slots[1, 11] = -1                                            # an ignored lookup: a zero row
    sl = torch.from_numpy(slots).cuda()
    off = torch.arange(nnz + 1, dtype=torch.int32, device="cuda")
    for hook in (0, 4 if nnz % 4 == 0 else 3):
        keys = presort_window(sl, R, offsets=off, include_last_offset=True, hook_features=hook, identity_bags=True)
        for b in range(P):
            rows = t[torch.from_numpy(np.maximum(slots[b], 0))].clone()
            rows[torch.from_numpy(slots[b] < 0)] = 0
            if hook:
                rows = rows.view(hook, nnz // hook, D).transpose(0, 1).contiguous()
            rows = rows.view(-1, D)
            for ot in OUT:
                out = embedding_bag(sl[b], w, off, mode="sum", include_last_offset=True, hook_features=hook,
                                    presorted=keys[b], output_dtype=ot)
                if ot == wt:
                    assert torch.equal(_bits(out.view(-1, D)), _bits(rows)), (hook, b, "not a bit copy")
                else:
                    _equal_cast(out.view(-1, D), rows.float())


# ---- 3. update, nearest ----------------------------------------------------------------------------------------------

def _update_layout(rng):
    """64 bags of 16: rows 0..99 and 160..200 looked up once, rows 100..138 2..40 times, row 150 in every bag, the rest
    (201.. among them) never"""
    others = np.concatenate([np.arange(100), np.arange(160, 201)] + [np.full(k + 2, 100 + k) for k in range(39)])
    assert len(others) == 960
    others = rng.permutation(others).reshape(64, 15)
    idx = np.concatenate([np.full((64, 1), 150), others], axis=1).reshape(-1)
    return idx, np.arange(0, 1025, 16)


@pytest.mark.parametrize("g16", [False, True], ids=["grad_fp32", "grad_16"])
@pytest.mark.parametrize("form", ["slots", "src"])
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("wt", W16, ids=lambda d: "table_" + NAMES[d])
@pytest.mark.parametrize("D", [8, 128])
def test_update_nearest(D, wt, opt, form, g16):
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD, embedding_bag, presort_window
    rng = np.random.default_rng(31)
    R, lr, calls = 300, 2.0 ** -3, 2
    idx, off = _update_layout(rng)
    t0 = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(wt)
    w = t0.clone().cuda()
    mom = torch.zeros(R, device="cuda")
    fused = FusedRowwiseAdagrad(lr, momentum=mom) if opt == "adagrad" else FusedSGD(lr)
    fused.rounding = "nearest"
    ids = torch.from_numpy(idx).cuda()
    offs = torch.from_numpy(off).cuda()
    pre = None
    if form == "src":
        pre = presort_window(ids.view(1, -1), R, offsets=offs.to(torch.int32), include_last_offset=True)[0]
    u = ref.UNIT_ROUNDOFF[wt]
    cur = t0.clone()                                                   # the 16-bit table as the steps leave it
    track = _Track(t0.float().numpy(), R, lr) if opt == "adagrad" else None
    for k in range(calls):
        go = torch.from_numpy(rng.standard_normal((64, D)).astype(np.float32))
        if g16:
            go = go.to(wt)
        w.requires_grad_(True)
        o = embedding_bag(ids, w, offs, mode="sum", include_last_offset=True, fused_sgd=fused, presorted=pre,
                          output_dtype=go.dtype)
        o.backward(go.cuda())
        assert w.grad is None
        w.requires_grad_(False)
        got = w.detach().cpu()
        rows, grads = ref.adagrad.lookup_grads(idx, off, go.float().numpy(), R)
        g64, cnt, gabs = ref.fold_rows(rows, grads, R)
        old = cur.float().numpy().astype(np.float64)
        touched = cnt > 0
        if opt == "sgd":
            x64 = old - lr * g64
            E = ref.sgd_fp32_error(np.abs(old), lr, gabs, cnt)
            once = np.nonzero(cnt == 1)[0]
            want = (cur[once].float().numpy() - np.float32(lr) * g64[once].astype(np.float32)).astype(np.float32)
            assert torch.equal(_bits(got[once]), _bits(torch.from_numpy(want).to(wt))), "rows looked up once"
        else:
            track.W[:] = old                                           # the update starts from the 16-bit old row
            track.tol_w[:] = 0
            track.step(rows, grads)
            x64 = track.W
            E = track.tol_w[:, None] + 1e-5 * np.abs(x64) + 1e-6
            M = mom.cpu().double().numpy()
            bad = np.nonzero(np.abs(M - track.M) > track.tol_m + 1e-6 * np.abs(track.M))[0]
            assert bad.size == 0, (bad[:5], M[bad[:5]], track.M[bad[:5]])
        err = np.abs(got.double().numpy() - x64)
        lim = ref.update_bound(x64, E, wt)
        bad = np.nonzero(touched[:, None] & (err > lim))
        assert bad[0].size == 0, (k, bad[0][:5], err[bad][:5], lim[bad][:5])
        assert torch.equal(_bits(got[~torch.from_numpy(touched)]), _bits(cur[~torch.from_numpy(touched)])), \
            "rows never looked up must not move"
        assert (~touched).sum() >= 100 and (cnt == 1).sum() == 141 and cnt[150] == 64 and cnt[138] == 40
        cur = got.clone()
    ws = fused._ws16
    assert int(torch.count_nonzero(ws[:-256])) == 0, "the workspace must be left zero-filled"
    assert int(ws[-256:-248].view(torch.int64).item()) == calls and int(torch.count_nonzero(ws[-248:])) == 0


# ---- 4. update, stochastic -------------------------------------------------------------------------------------------

class _Sr:
    """2048 rows x 128 elements of 1.0, every row looked up once (identity layout), SGD with lr = 1 through the C entry"""
    R, D = 2048, 128

    def __init__(self, wt, rmap=None):
        from cachedembedding_amd import _lib
        self._lib, self.wt = _lib, wt
        self.w = torch.ones(self.R, self.D, dtype=wt, device="cuda")
        self.ws = torch.zeros(_lib.lib.ce_bag_backward_w16_workspace(self.R, self.D), dtype=torch.uint8, device="cuda")
        self.ids = torch.randperm(self.R, generator=torch.Generator().manual_seed(1)).cuda()
        self.off = torch.arange(self.R + 1, device="cuda")
        self.rmap = rmap
        self.go = torch.zeros(self.R, self.D, device="cuda")

    def reset(self, zero_ws=False):
        self.w.fill_(1.0)
        if zero_ws:
            self.ws.zero_()

    def call(self, seed):
        _lib = self._lib
        _lib.check(_lib.lib.ce_bag_backward_update_w16(
            self.w.data_ptr(), _lib.ACT_DTYPES[self.wt], self.R, self.D, self.ids.data_ptr(), self.R,
            self.off.data_ptr(), 1, self.R, 1, None, _lib.CE_MODE_SUM, 0, self.go.data_ptr(), _lib.CE_ACT_F32, None,
            _lib.ptr(self.rmap), None, 0, 1.0, 0.0, _lib.CE_OPT_SGD, _lib.CE_ROUND_STOCHASTIC, seed,
            self.ws.data_ptr(), self.ws.numel(), _lib.stream_ptr()))

    def run(self, seed):
        self.call(seed)
        return self.w.detach().cpu().float()


@pytest.mark.parametrize("wt", W16, ids=lambda d: "table_" + NAMES[d])
def test_update_stochastic(wt):
    step = 2.0 ** (ref.DROPPED_BITS[wt] - 23)                       # spacing of the type above 1.0
    s = _Sr(wt)
    n = s.R * s.D
    assert n == 262144
    first = None
    for p in (0.25, 0.5, 0.875):
        s.reset(zero_ws=True)
        s.go.fill_(-p * step)                                         # x = 1 + p * step, exact in fp32
        got = s.run(seed=11)
        up = got == 1.0 + step
        assert bool(((got == 1.0) | up).all()), "a result that is neither neighbour"
        share = float(up.double().mean())
        assert abs(share - p) <= 6 * np.sqrt(p * (1 - p) / n), (p, share)
        if p == 0.25:
            first = got
    # a representable x never moves off it
    s.reset(zero_ws=True)
    s.go.fill_(-step)
    assert bool((s.run(seed=11) == 1.0 + step).all())
    s.go.fill_(0.0)
    assert bool((s.run(seed=11) == 1.0 + step).all())
    # the step counter: a second identical call draws other bits; a zeroed workspace + the same seed reproduces
    s.reset(zero_ws=True)
    s.go.fill_(-0.25 * step)
    a = s.run(seed=11)
    assert torch.equal(a, first)
    s.reset()
    b = s.run(seed=11)
    assert not torch.equal(a, b)
    assert int(s.ws[-256:-248].view(torch.int64).item()) == 2
    s.reset(zero_ws=True)
    assert not torch.equal(s.run(seed=12), a)
    # the bits follow the host-table row, not the slot: slot q holds row rmap[q]
    rmap = torch.randperm(s.R, generator=torch.Generator().manual_seed(2)).to(torch.int32)
    s2 = _Sr(wt, rmap=rmap.cuda())
    s2.go.fill_(-0.25 * step)
    c = s2.run(seed=11)
    assert torch.equal(c, a[rmap.long()])
    # one captured backward replayed twice draws two patterns
    s.reset(zero_ws=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.call(11)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.call(11)
    pats = []
    for _ in range(2):
        s.reset()
        graph.replay()
        torch.cuda.synchronize()
        pats.append(s.w.detach().cpu().float())
    assert not torch.equal(pats[0], pats[1])
    for g in pats:
        assert bool(((g == 1.0) | (g == 1.0 + step)).all())


# ---- 5-7. through the cache, the windows, a checkpoint ---------------------------------------------------------------

N_TOY, D_TOY, B_TOY, LR_TOY, SEED_TOY = 2000, 32, 64, 2.0 ** -3, 77


def _toy_batches(steps, D=D_TOY):
    """ids unique within a step: half from 100 hot ids, half from the rest -- a 200-row cache evicts from step 4 on"""
    rng = np.random.default_rng(9)
    ids = [np.concatenate([rng.choice(100, B_TOY // 2, replace=False),
                           100 + rng.choice(N_TOY - 100, B_TOY // 2, replace=False)]) for _ in range(steps)]
    grads = [rng.standard_normal((B_TOY, D)).astype(np.float32) for _ in range(steps)]
    return ids, grads


def _fp32_fill(D=D_TOY):
    from cachedembedding_amd import _lib
    f = np.zeros(N_TOY * D, np.float32)
    _lib.check(_lib.lib.ce_host_fill_uniform(f.ctypes.data, f.size, -1.0 / N_TOY, 1.0 / N_TOY, SEED_TOY, 1))
    return torch.from_numpy(f).view(N_TOY, D)


def _replica(wt, ids, grads, D=D_TOY):
    """a torch-CPU 16-bit [N, D] tensor under the reference update, step by step"""
    t = _fp32_fill(D).to(wt)
    for i, g in zip(ids, grads):
        ref.sgd_step_nearest(t, i, g, LR_TOY)
    return t


def _toy_module(strategy, transport, table_dtype, C=200, D=D_TOY, **kw):
    import cachedembedding_amd as ce
    st = ce.EvictionStrategy.LFU if strategy == "lfu" else ce.EvictionStrategy.DATASET
    emb = ce.CachedEmbeddingBag(N_TOY, D, mode="sum", include_last_offset=True, cuda_row_num=C, warmup_ratio=0.0,
                                evict_strategy=st, init_seed=SEED_TOY, table_dtype=table_dtype, **kw)
    if transport is not None:
        emb.cache_weight_mgr.set_transport(transport)
    return emb


@pytest.mark.parametrize("transport", ["zerocopy", "worker"])
@pytest.mark.parametrize("strategy", ["dataset", "lfu"])
def test_through_the_cache_sgd(strategy, transport):
    wt = torch.bfloat16
    ids, grads = _toy_batches(30)
    emb = _toy_module(strategy, transport, wt)
    assert emb.weight.dtype == wt and emb.element_size() == 2 and emb.output_dtype == wt
    assert next(emb.parameters()).dtype == wt and next(emb.parameters()).shape == (200, D_TOY)
    assert torch.equal(_bits(emb.weight), _bits(_fp32_fill().to(wt))), "the 16-bit fill is the cast of the fp32 fill"
    plain = _toy_module(strategy, transport, None)
    off = torch.arange(B_TOY + 1, device="cuda")
    for m in (emb, plain):
        m.set_fused_sgd(LR_TOY)
    emb.set_weight_rounding("nearest")
    for i, g in zip(ids, grads):
        out = emb(torch.from_numpy(i).cuda(), off)
        out.backward(torch.from_numpy(g).cuda().to(out.dtype))
        o32 = plain(torch.from_numpy(i).cuda(), off)
        o32.backward(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    assert sum(emb.num_write_back_history[:3]) == 0 and sum(emb.num_write_back_history[3:]) > 0
    emb.flush()
    plain.flush()
    g16 = [torch.from_numpy(g).to(wt).float().numpy() for g in grads]        # the gradient as the bf16 output's autograd delivers it
    want = _replica(wt, ids, g16)
    assert torch.equal(_bits(emb.weight), _bits(want)), "residency must be invisible: the cache moves bits"
    untouched = np.setdiff1d(np.arange(N_TOY), np.concatenate(ids))
    assert untouched.size > 0
    assert torch.equal(_bits(emb.weight[untouched]), _bits(_fp32_fill().to(wt)[untouched]))
    assert emb.num_hits_history == plain.num_hits_history and emb.num_miss_history == plain.num_miss_history
    assert emb.num_write_back_history == plain.num_write_back_history


@pytest.mark.parametrize("transport", ["zerocopy", "worker"])
@pytest.mark.parametrize("strategy", ["dataset", "lfu"])
def test_through_the_cache_sgd_wide_rows(strategy, transport):
    """test_through_the_cache_sgd at D = 1024, the top of the 16-bit dim rule: the cache op is driven with 512 fp32
    elements per row, 128 16-byte units -- two whole passes of the row movers' 64-lane group, where D = 32 is 4 lanes of
    one"""
    wt, D = torch.bfloat16, 1024
    ids, grads = _toy_batches(30, D)
    emb = _toy_module(strategy, transport, wt, D=D)
    assert emb.cache_weight_mgr._lib_dim == 512 and emb.cache_weight_mgr.transport_name == transport
    assert emb.weight.dtype == wt and emb.element_size() == 2 and emb.output_dtype == wt
    assert next(emb.parameters()).dtype == wt and next(emb.parameters()).shape == (200, D)
    fill = _fp32_fill(D).to(wt)
    assert torch.equal(_bits(emb.weight), _bits(fill)), "the 16-bit fill is the cast of the fp32 fill"
    plain = _toy_module(strategy, transport, None, D=D)
    off = torch.arange(B_TOY + 1, device="cuda")
    for m in (emb, plain):
        m.set_fused_sgd(LR_TOY)
    emb.set_weight_rounding("nearest")
    for i, g in zip(ids, grads):
        out = emb(torch.from_numpy(i).cuda(), off)
        out.backward(torch.from_numpy(g).cuda().to(out.dtype))
        o32 = plain(torch.from_numpy(i).cuda(), off)
        o32.backward(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    assert sum(emb.num_write_back_history[:3]) == 0 and sum(emb.num_write_back_history[3:]) > 0
    emb.flush()
    plain.flush()
    g16 = [torch.from_numpy(g).to(wt).float().numpy() for g in grads]        # the gradient as the bf16 output's autograd delivers it
    want = _replica(wt, ids, g16, D)
    assert torch.equal(_bits(emb.weight), _bits(want)), "residency must be invisible: the cache moves bits"
    untouched = np.setdiff1d(np.arange(N_TOY), np.concatenate(ids))
    assert untouched.size > 0
    assert torch.equal(_bits(emb.weight[untouched]), _bits(fill[untouched]))
    assert emb.num_hits_history == plain.num_hits_history and emb.num_miss_history == plain.num_miss_history
    assert emb.num_write_back_history == plain.num_write_back_history


def test_through_the_cache_rowwise_adagrad():
    wt = torch.bfloat16
    ids, grads = _toy_batches(30)
    emb = _toy_module("dataset", "zerocopy", wt, output_dtype=torch.float32)
    emb.set_fused_rowwise_adagrad(LR_TOY)
    emb.set_weight_rounding("nearest")
    off = torch.arange(B_TOY + 1, device="cuda")
    w0 = _fp32_fill().to(wt).float().numpy()
    track = _Track(w0, N_TOY, LR_TOY)
    u = ref.UNIT_ROUNDOFF[wt]
    round_tol = np.zeros((N_TOY, D_TOY))
    for i, g in zip(ids, grads):
        out = emb(torch.from_numpy(i).cuda(), off)
        out.backward(torch.from_numpy(g).cuda())
        track.step(i, g.astype(np.float64))
        round_tol[i] += u * np.abs(track.W[i])                  # one rounding per step a row is updated in
    torch.cuda.synchronize()
    emb.flush()
    mgr = emb.cache_weight_mgr
    # the bound of test_update_nearest, accumulated over the steps a row took part in
    E = track.tol_w[:, None] + 1e-5 * np.abs(track.W) + 1e-6
    err = np.abs(mgr.weight.double().numpy() - track.W)
    assert not (err > round_tol + (1 + u) * E).any()
    M = mgr.momentum1.cpu().double().numpy()
    assert not (np.abs(M - track.M) > track.tol_m + 1e-6 * np.abs(track.M)).any()
    never = np.setdiff1d(np.arange(N_TOY), np.concatenate(ids))
    assert torch.equal(_bits(mgr.weight[never]), _bits(torch.from_numpy(w0[never]).to(wt)))


@pytest.mark.parametrize("mode", ["overlap", "graph"])
def test_prefetch_and_graphed_windows(mode):
    """keys forward, keys backward and the captured step on a 16-bit module; 8 windows of 4 batches, a cache of 600
    rows (two consecutive windows must fit), one static gradient (a captured step reads static tensors)"""
    from cachedembedding_amd.pipeline import GraphedWindow, PrefetchWindow
    wt = torch.bfloat16
    P, nwin = 4, 8
    ids, grads = _toy_batches(P * nwin)
    go = torch.from_numpy(grads[0]).to(wt)
    emb = _toy_module("dataset", None, wt, C=600, strict=False)
    emb.set_fused_sgd(LR_TOY)
    emb.set_weight_rounding("nearest")
    emb.set_cache_op(False)
    off = torch.arange(B_TOY + 1, dtype=torch.int32, device="cuda")
    layout = (off, True, 0)
    grad = go.cuda()
    windows = [[torch.from_numpy(ids[w * P + i]) for i in range(P)] for w in range(nwin)]
    seq = []

    def step(slots, i, keys=None):
        out = emb(slots, off, presorted=keys)
        out.backward(grad)

    if mode == "graph":
        gw = GraphedWindow(emb, P, B_TOY, step, overlap=True, warmup_values=[v.cuda() for v in windows[0]],
                           presort=True, transport="worker", bag_layout=layout, arrangement="overlap")
        seq += [v.numpy() for v in windows[0]]                   # the capture's eager warm-up trained on window 0 once
        gw.submit([v.cuda() for v in windows[0]], 0)
        for w in range(nwin):
            if w + 1 < nwin:
                gw.submit([v.cuda() for v in windows[w + 1]], (w + 1) % 2)
            gw.run(w % 2)
    else:
        win = PrefetchWindow(emb, P, overlap=True, presort=True, transport="worker", bag_layout=layout,
                             arrangement="overlap")
        win.submit([v.cuda() for v in windows[0]])
        for w in range(nwin):
            slots = win.collect()
            if w + 1 < nwin:
                win.submit([v.cuda() for v in windows[w + 1]])
            for i in range(P):
                step(slots[i], i, win.keys[i])
    seq += [v.numpy() for w in windows for v in w]
    torch.cuda.synchronize()
    mgr = emb.cache_weight_mgr
    assert mgr.sync_stats().status == 0
    assert sum(emb.num_write_back_history) > 0, "the cache never evicted"
    emb.flush()
    want = _replica(wt, seq, [go.float().numpy()] * len(seq))
    assert torch.equal(_bits(mgr.weight), _bits(want))


def test_checkpoint_round_trip(tmp_path):
    """train, flush(), save .weight, rebuild with from_pretrained(table_dtype=), continue: bit-equal to a module that
    never stopped (nearest rounding)"""
    import cachedembedding_amd as ce
    wt = torch.bfloat16
    ids, grads = _toy_batches(16)
    off = torch.arange(B_TOY + 1, device="cuda")
    kw = dict(mode="sum", include_last_offset=True, cuda_row_num=200, warmup_ratio=0.0, table_dtype=wt)

    def train(m, lo, hi):
        outs = []
        for i, g in zip(ids[lo:hi], grads[lo:hi]):
            o = m(torch.from_numpy(i).cuda(), off)
            o.backward(torch.from_numpy(g).cuda().to(o.dtype))
            outs.append(o.detach().cpu())
        return outs

    def prepare(m):
        m.set_fused_sgd(LR_TOY)
        m.set_weight_rounding("nearest")
        return m

    w0 = _fp32_fill()
    a = prepare(ce.CachedEmbeddingBag.from_pretrained(w0.clone(), freeze=False, **kw))      # fp32 in: cast once
    assert a.weight.dtype == wt and torch.equal(_bits(a.weight), _bits(w0.to(wt)))
    train(a, 0, 8)
    a.flush()
    path = tmp_path / "table.pt"
    torch.save(a.weight.clone(), path)
    saved = torch.load(path)
    assert saved.dtype == wt
    b = prepare(ce.CachedEmbeddingBag.from_pretrained(saved, freeze=False, **kw))           # 16-bit in: pinned in place
    assert b.weight.data_ptr() == saved.data_ptr()
    oa, ob = train(a, 8, 16), train(b, 8, 16)
    for x, y in zip(oa, ob):
        assert torch.equal(_bits(x), _bits(y))
    a.flush()
    b.flush()
    assert torch.equal(_bits(a.weight), _bits(b.weight))
    g16 = [torch.from_numpy(g).to(wt).float().numpy() for g in grads]
    assert torch.equal(_bits(a.weight), _bits(_replica(wt, ids, g16)))
