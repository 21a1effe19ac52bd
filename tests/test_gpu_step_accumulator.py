"""GPU tests of the step-sized accumulator of the atomic fused updates (accumulator="step",
ce_bag_backward_update_compact*): bit equality with the cache-sized path, the compaction's edges, stale cidx entries,
hot rows against the fp64 reference, graph capture, the memory bound and the module under eviction and GraphedWindow.

Bit equality rests on id streams in which a row is looked up at most twice per step: two fp32 terms sum the same in
either order, so the atomics of the two paths cannot differ -- and the compaction numbers the slots in ascending order,
so the scatter's tiles, shares and runs are the same on both.  The module test uses gradients on a 2^-6 grid instead,
whose sums are exact in fp32 in any order.

The kernels only ever see in-range slots and the documented ignored slot -1."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import rowwise_adagrad_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
U = np.finfo(np.float32).eps / 2
F = 4
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# table dtype - optimizer [- stochastic rounding]
KINDS = ["fp32-adagrad", "bf16-adagrad", "fp16-adagrad", "bf16-sgd", "fp16-sgd", "bf16-sgd-stoch", "fp16-sgd-stoch"]
FORMS = ["sum", "mean", "psw", "padding", "presorted", "src"]


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _layout(C, nnz, D):
    """byte offsets inside the workspace (include/ce_api.h: the counter, U, flags, acc, cidx, the scan's counts, list;
    every part padded to 256 bytes)"""
    from cachedembedding_amd import _lib

    def al(x):
        return (x + 255) // 256 * 256
    cap = min(nnz, C)
    o = 512
    lay = dict(cap=cap, n_list=256, flags=o)
    o = al(o + C)
    lay["acc"] = o
    o = al(o + cap * D * 4)
    o = al(o + 4 * C)                                                            # cidx
    o = al(o + 4 * ((C + _lib.CE_COMPACT_BLOCK - 1) // _lib.CE_COMPACT_BLOCK))    # the scan's counts
    lay["list"] = o
    return lay


def _ws_state(ws, C, nnz, D):
    """(U, list[:U], flags and acc all zero?) read back from the workspace tensor"""
    lay = _layout(C, nnz, D)
    n = int(ws[lay["n_list"]:lay["n_list"] + 4].view(torch.int32).item())
    lst = ws[lay["list"]:lay["list"] + 4 * lay["cap"]].view(torch.int32)[:n].cpu().numpy()
    clean = int(torch.count_nonzero(ws[lay["flags"]:lay["flags"] + C])) == 0 and \
        int(torch.count_nonzero(ws[lay["acc"]:lay["acc"] + lay["cap"] * D * 4])) == 0
    return n, lst, clean


def _fused(kind, accumulator, R, lr=0.05, seed=5):
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD
    parts = kind.split("-")
    if parts[1] == "adagrad":
        f = FusedRowwiseAdagrad(lr, momentum=torch.zeros(R, device="cuda"), accumulator=accumulator)
    else:
        f = FusedSGD(lr, accumulator=accumulator)
    f.rounding, f.seed = ("stochastic" if parts[-1] == "stoch" else "nearest"), seed
    return f


def _step(w, idx, offs, go, fused, mode="sum", psw=None, hook=0, pre=None, masked=False):
    from cachedembedding_amd.functional import embedding_bag
    w.requires_grad_(True)
    o = embedding_bag(idx, w, offs, mode=mode, include_last_offset=True, per_sample_weights=psw, hook_features=hook,
                      fused_sgd=fused, presorted=pre, masked_indices=masked, output_dtype=go.dtype)
    o.backward(go.view_as(o))
    assert w.grad is None                                         # the update happened inside backward
    w.requires_grad_(False)


def _twice_stream(rng, R, twice, once, pad):
    """ids in which `twice` rows occur twice, `once` rows once, and `pad` ignored lookups (-1), shuffled"""
    perm = rng.permutation(R)
    ids = np.concatenate([perm[:twice], perm[:twice], perm[twice:twice + once], np.full(pad, -1)])
    return ids[rng.permutation(len(ids))]


def _form_step(rng, form, R, D, gdt, twice=2000, once=1000, pad=120):
    """one step's inputs of a form, on the device; (idx, offs, go, kw of _step, ids, off, go32)"""
    from cachedembedding_amd.functional import presort_slots, presort_window
    masked = form in ("padding", "presorted", "src")
    ids = _twice_stream(rng, R, twice, once, pad if masked else 0)
    nnz = len(ids)
    psw = None
    if form in ("mean", "psw"):
        off = np.unique(np.concatenate([rng.choice(np.arange(1, nnz), nnz // 3, replace=False), [0, nnz]]))
        hook = 0
    else:
        off = np.arange(nnz + 1)
        hook = F
    nb = len(off) - 1
    go32 = rng.standard_normal((nb // F, F, D) if hook else (nb, D)).astype(np.float32)
    go = torch.from_numpy(go32).to(gdt).cuda()
    if form == "psw":
        psw = rng.random(nnz).astype(np.float32)
    idx = torch.from_numpy(ids).cuda()
    offs = torch.from_numpy(off).cuda()
    pre = None
    if form == "presorted":
        pre = presort_slots(idx, R)
    elif form == "src":
        pre = presort_window(idx.view(1, -1), R, offsets=offs.to(torch.int32), include_last_offset=True,
                             hook_features=hook, identity_bags=True)[0]
    kw = dict(mode="mean" if form == "mean" else "sum", psw=None if psw is None else torch.from_numpy(psw).cuda(),
              hook=hook, pre=pre, masked=masked)
    return idx, offs, go, kw, dict(ids=ids, off=off, go=go.float().cpu().numpy(), psw=psw, hook=hook)


def _pair(kind, form, D, gdt=torch.float32, R=9000, steps=3):
    """the same steps under accumulator="cache" and "step", from the same start: bits of (weight, momentum) per step"""
    wt = DT[kind.split("-")[0]]
    W0 = torch.from_numpy(np.random.default_rng(21).standard_normal((R, D)).astype(np.float32)).to(wt)
    out = {}
    for acc in ("cache", "step"):
        rng = np.random.default_rng(22)
        w = W0.clone().cuda()
        fused = _fused(kind, acc, R)
        mom = getattr(fused, "momentum", None)
        trace = []
        for _ in range(steps):
            idx, offs, go, kw, _ = _form_step(rng, form, R, D, gdt)
            _step(w, idx, offs, go, fused, **kw)
            trace.append((_bits(w), None if mom is None else _bits(mom)))
        torch.cuda.synchronize()
        if acc == "step":
            assert fused._ws is None and fused._ws16 is None, "the cache-sized accumulators must never be allocated"
            assert fused._ws_step is not None
        else:
            assert fused._ws_step is None
        out[acc] = trace
    for k in range(steps):
        a, b = out["cache"][k], out["step"][k]
        if a[1] is not None:
            assert torch.equal(a[1], b[1]), (k, "momentum")
        assert torch.equal(a[0], b[0]), (k, "weight")
    assert not torch.equal(out["step"][0][0], _bits(W0))
    assert not torch.equal(out["step"][0][0], out["step"][1][0])


# ---- 1. bit equality with the cache-sized path -----------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_bit_equal_to_the_cache_sized_path(kind, form):
    _pair(kind, form, 128)


@pytest.mark.parametrize("form", ["sum", "src"])
@pytest.mark.parametrize("gdt", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["fp32-adagrad", "fp16-adagrad", "bf16-sgd-stoch"])
def test_bit_equal_with_16_bit_gradients(kind, gdt, form):
    _pair(kind, form, 128, gdt=DT[gdt])


@pytest.mark.parametrize("form", ["padding", "src"])
@pytest.mark.parametrize("D,kind", [(8, "fp32-adagrad"), (8, "bf16-adagrad"), (8, "fp16-sgd-stoch"), (6, "fp32-adagrad"),
                                    (512, "fp32-adagrad"), (512, "bf16-adagrad"), (768, "fp32-adagrad"),
                                    (768, "fp16-sgd"), (1024, "fp32-adagrad"), (1024, "fp16-adagrad"),
                                    (1024, "bf16-sgd-stoch")])
def test_bit_equal_on_every_lane_shape(D, kind, form):
    """vector lanes with 1 (D = 8, 128), 2 (512), 3-of-4 (768) and 4 (1024) chunks per lane, and the scalar form (6)"""
    _pair(kind, form, D, R=6000)


# ---- 2. compaction edges ---------------------------------------------------------------------------------------------

class _Track:
    """fp64 reference state + per-row tolerances accumulated over the steps: the per-row accumulation bound of
    tests/test_gpu_rowwise_adagrad.py, restated (as tests/test_gpu_deterministic_adagrad.py does).  Atomics add a row's
    terms in some order: a recursive summation, every term passing through at most n - 1 additions, so
    |fp32 fold - exact| <= (n - 1) u S whatever the order."""

    def __init__(self, W0, N, lr, eps=1e-8):
        self.W, self.M = W0.astype(np.float64).copy(), np.zeros(N)
        self.lr, self.eps = lr, eps
        R = W0.shape[0]
        self.tol_w, self.tol_m = np.zeros(R), np.zeros(N)
        self.multi = np.zeros(R, bool)
        self.touched = np.zeros(R, bool)

    def bounds(self, rows, grads):
        R, D = self.W.shape
        cnt = np.bincount(rows, minlength=R)
        s = np.zeros((R, D))
        np.add.at(s, rows, np.abs(grads))
        g = np.zeros((R, D))
        np.add.at(g, rows, grads)
        return cnt, s.max(axis=1), np.abs(g).max(axis=1)

    def step(self, rows, grads):
        D = self.W.shape[1]
        cnt, s, gmax = self.bounds(rows, grads)
        ref.step(self.W, self.M, rows, grads, self.lr, self.eps)
        m_now = np.maximum(self.M, 1e-30)
        t = cnt > 0
        self.touched |= t
        self.multi |= cnt > 1
        # the fold's error e moves m by <= 2 |g| e (+ the rounding of a D-term sum of squares and of the add), and the
        # update lr g / sqrt(m) by <= lr e / sqrt(m) plus |update| * dm / (2 m), |update| <= lr sqrt(D)
        e = np.maximum(cnt - 1, 0) * U * s
        dm = 2 * gmax * e * 2 + 4 * (D + 2) * U * m_now
        dw = 2 * self.lr * e / np.sqrt(m_now) + self.lr * np.sqrt(D) * dm / m_now + 8 * self.lr * U * np.sqrt(D)
        self.tol_w += np.where(t, dw, 0)
        self.tol_m[t] += dm[t]
        return dw, dm

    def check(self, W, M):
        W, M = np.asarray(W, np.float64), np.asarray(M, np.float64)
        once = self.touched & ~self.multi
        np.testing.assert_allclose(W[once], self.W[once], rtol=1e-5, atol=1e-6)
        err = np.abs(W - self.W)
        lim = self.tol_w[:, None] + 1e-5 * np.abs(self.W) + 1e-6
        bad = np.nonzero(self.touched & (err > lim).any(1))[0]
        assert bad.size == 0, (bad[:5], err[bad[:5]].max(1), lim[bad[:5]].min(1))
        assert np.array_equal(W[~self.touched], self.W[~self.touched].astype(np.float32))
        bad = np.nonzero(np.abs(M - self.M) > self.tol_m + 1e-6 * np.abs(self.M))[0]
        assert bad.size == 0, (bad[:5], M[bad[:5]], self.M[bad[:5]], self.tol_m[bad[:5]])


def _edge_ids(case, C, rng):
    from cachedembedding_amd import _lib
    blk = _lib.CE_COMPACT_BLOCK
    if case == "ends":                       # slots 0 and C - 1 flagged, ignored lookups in between
        return np.concatenate([[0, C - 1, -1, C - 1], rng.integers(1, C - 1, 700), np.full(19, -1)])
    if case == "full_and_empty":             # the second scan workgroup entirely flagged, the third empty
        ids = np.concatenate([np.arange(blk, 2 * blk), rng.integers(0, blk, 300), rng.integers(3 * blk, C, 9)])
        return ids[rng.permutation(len(ids))]
    if case == "all_distinct":               # U == cap == nnz
        return rng.permutation(C)[:3001]
    if case == "one":                        # U == 1
        return np.full(777, 2 * blk + 63)
    if case == "more_lookups_than_slots":    # nnz > C, every slot flagged: U == cap == C
        ids = np.concatenate([np.arange(C), rng.integers(0, C, 16384 - C)])
        return ids[rng.permutation(len(ids))]
    raise KeyError(case)


@pytest.mark.parametrize("case", ["ends", "full_and_empty", "all_distinct", "one", "more_lookups_than_slots"])
def test_compaction_edges(case):
    """C = 3 scan workgroups + 17 slots: list = the sorted distinct valid slots, U their number, the update within the
    fp64 bounds, and flags and acc zero again"""
    from cachedembedding_amd import _lib
    C, D, lr = 3 * _lib.CE_COMPACT_BLOCK + 17, 8, 0.05
    rng = np.random.default_rng(31)
    ids = _edge_ids(case, C, rng)
    nnz = len(ids)
    want = np.unique(ids[ids >= 0])
    if case in ("all_distinct", "more_lookups_than_slots"):
        assert len(want) == min(nnz, C)
    if case == "more_lookups_than_slots":
        assert nnz > C
    W0 = rng.standard_normal((C, D)).astype(np.float32)
    go = rng.standard_normal((nnz, D)).astype(np.float32)
    w = torch.from_numpy(W0).cuda()
    fused = _fused("fp32-adagrad", "step", C, lr=lr)
    _step(w, torch.from_numpy(ids).cuda(), torch.arange(nnz + 1, device="cuda"), torch.from_numpy(go).cuda(), fused,
          masked=True)
    torch.cuda.synchronize()
    ws = fused._ws_step
    assert ws.numel() == _lib.lib.ce_bag_backward_update_compact_workspace(C, nnz, D)
    n, lst, clean = _ws_state(ws, C, nnz, D)
    assert n == len(want), (n, len(want))
    assert np.array_equal(lst, want)
    assert clean, "flags and acc must be left zero-filled"
    track = _Track(W0, C, lr)
    keep = ids >= 0
    track.step(ids[keep], go[keep].astype(np.float64))
    track.check(w.cpu().numpy(), fused.momentum.cpu().numpy())
    assert int(torch.count_nonzero(fused.momentum)) == len(want)


# ---- 3. stale cidx ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["fp32-adagrad", "bf16-sgd"])
def test_stale_cidx_entries_are_never_read(kind):
    """step 2 looks up slots disjoint from step 1's (every cidx entry it does not write is stale), step 3 half of
    step 2's and half new ones: bit-equal to the cache-sized path, and flags and acc zero after every call"""
    C, D, n = 3 * 4096 + 17, 16, 1500
    wt = DT[kind.split("-")[0]]
    perm = np.random.default_rng(41).permutation(C)
    sets = [perm[:n], perm[n:2 * n], np.concatenate([perm[n:n + n // 2], perm[2 * n:2 * n + n // 2]])]
    assert not np.intersect1d(sets[0], sets[1]).size and np.intersect1d(sets[1], sets[2]).size == n // 2
    W0 = torch.from_numpy(np.random.default_rng(42).standard_normal((C, D)).astype(np.float32)).to(wt)
    res = {}
    for acc in ("cache", "step"):
        rng = np.random.default_rng(43)
        w = W0.clone().cuda()
        fused = _fused(kind, acc, C)
        for rows in sets:
            ids = np.concatenate([rows, rows[: n // 3]])                 # a third of them twice
            ids = ids[rng.permutation(len(ids))]
            go = torch.from_numpy(rng.standard_normal((len(ids), D)).astype(np.float32)).cuda()
            _step(w, torch.from_numpy(ids).cuda(), torch.arange(len(ids) + 1, device="cuda"), go, fused)
            if acc == "step":
                torch.cuda.synchronize()
                k, lst, clean = _ws_state(fused._ws_step, C, len(ids), D)
                assert k == n and np.array_equal(lst, np.sort(rows)) and clean
        torch.cuda.synchronize()
        res[acc] = (_bits(w), None if not hasattr(fused, "momentum") else _bits(fused.momentum))
    assert torch.equal(res["cache"][0], res["step"][0])
    if res["cache"][1] is not None:
        assert torch.equal(res["cache"][1], res["step"][1])
    touched = np.unique(np.concatenate(sets))
    rest = np.setdiff1d(np.arange(C), touched)
    assert torch.equal(res["step"][0][rest], _bits(W0)[rest])
    assert not (res["step"][0][touched] == _bits(W0)[touched]).all(1).any()


def test_steps_of_other_sizes_rezero_the_workspace_and_keep_the_counter():
    """the workspace's layout belongs to one nnz: a larger step allocates a new one, a smaller one re-zeroes it in
    place; flags and acc are zero after every call and the step counter goes on counting, so a stochastically rounded
    SGD step draws the bits of the cache-sized path, whose workspace -- and counter -- stays where it is"""
    C, D = 3 * 4096 + 17, 16
    W0 = torch.from_numpy(np.random.default_rng(45).standard_normal((C, D)).astype(np.float32)).to(torch.bfloat16)
    res = {}
    for acc in ("cache", "step"):
        rng = np.random.default_rng(46)
        w = W0.clone().cuda()
        fused = _fused("bf16-sgd-stoch", acc, C)
        sizes = []
        for k, (twice, once) in enumerate(((300, 400), (900, 1100), (200, 100), (900, 1100))):
            ids = _twice_stream(rng, C, twice, once, 0)
            go = torch.from_numpy(rng.standard_normal((len(ids), D)).astype(np.float32)).cuda() * 2.0 ** -10
            _step(w, torch.from_numpy(ids).cuda(), torch.arange(len(ids) + 1, device="cuda"), go, fused)
            if acc == "step":
                torch.cuda.synchronize()
                ws = fused._ws_step
                n, lst, clean = _ws_state(ws, C, len(ids), D)
                assert n == twice + once and np.array_equal(lst, np.unique(ids)) and clean
                assert int(ws[:8].view(torch.int64).item()) == k + 1
                sizes.append(ws.numel())
        if acc == "step":
            assert sizes[1] > sizes[0] and sizes[2] == sizes[1] == sizes[3]
        torch.cuda.synchronize()
        res[acc] = _bits(w)
    assert torch.equal(res["cache"], res["step"])
    assert not torch.equal(res["step"], _bits(W0))


# ---- 4. hot rows -----------------------------------------------------------------------------------------------------

def _hot_stream(rng, R, nnz, hot_row, hot_n):
    """hot_n lookups of hot_row, the rest a bounded Zipf tail: rank k = 1 .. R - 1 with probability ~ 1 / k, ranks spread
    over the other rows by a fixed permutation"""
    p = 1.0 / np.arange(1, R)
    others = np.setdiff1d(np.arange(R), [hot_row])[np.random.default_rng(50).permutation(R - 1)]
    tail = others[rng.choice(R - 1, nnz - hot_n, p=p / p.sum())]
    ids = np.concatenate([np.full(hot_n, hot_row), tail])
    return ids[rng.permutation(nnz)]


@pytest.mark.parametrize("form", ["sum", "src"])
def test_hot_rows_against_fp64_reference(form):
    """one row with 5000 lookups per step and a Zipf tail, 3 steps"""
    from cachedembedding_amd.functional import presort_window
    R, D, nnz, lr, hot = 20000, 32, 16384, 0.05, 12345
    rng = np.random.default_rng(51)
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    steps = [(_hot_stream(rng, R, nnz, hot, 5000), rng.standard_normal((nnz // F, F, D)).astype(np.float32))
             for _ in range(3)]
    # the stream on the CPU first: it has the hot row, a tail of repeated rows and rows seen once; the bound holds for
    # an fp32 evaluation of the specification on it (so a miss on the GPU is the kernels', not the bound's), and it does
    # not hold for the wrong form, one update per lookup (so it can tell the two apart)
    track = _Track(W0, R, lr)
    W32, M32 = W0.copy(), np.zeros(R, np.float32)
    Wbad, Mbad = W0.astype(np.float64), np.zeros(R)
    for ids, go in steps:
        assert (ids == hot).sum() == 5000 and len(np.unique(ids)) > 1000
        cnt = np.bincount(ids, minlength=R)
        assert (cnt > 50).sum() >= 5 and (cnt == 1).sum() > 500
        grads = go.transpose(1, 0, 2).reshape(nnz, D)
        track.step(ids, grads.astype(np.float64))
        ref.step(W32, M32, ids, grads, lr, dtype=np.float32)
        ref.step_per_lookup(Wbad, Mbad, ids, grads.astype(np.float64), lr)
    track.check(W32, M32)
    with pytest.raises(AssertionError):
        track.check(Wbad, Mbad)
    w = torch.from_numpy(W0).cuda()
    fused = _fused("fp32-adagrad", "step", R, lr=lr)
    off = torch.arange(nnz + 1, device="cuda")
    for ids, go in steps:
        idx = torch.from_numpy(ids).cuda()
        pre = None
        if form == "src":
            pre = presort_window(idx.view(1, -1), R, offsets=off.to(torch.int32), include_last_offset=True,
                                 hook_features=F, identity_bags=True)[0]
        _step(w, idx, off, torch.from_numpy(go).cuda(), fused, hook=F, pre=pre)
    torch.cuda.synchronize()
    track.check(w.cpu().numpy(), fused.momentum.cpu().numpy())
    assert _ws_state(fused._ws_step, R, nnz, D)[2]


# ---- 5. graph capture ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["fp32-adagrad", "bf16-adagrad", "fp16-sgd", "bf16-sgd-stoch"])
def test_captured_backward_replayed_equals_eager_steps(kind):
    """one captured forward + backward (source-row keys) replayed 4 times == 4 eager steps, bit for bit (a row at most
    twice per step); stochastic rounding draws fresh bits per replay because the counter lives in the workspace"""
    from cachedembedding_amd.functional import embedding_bag
    R, D = 9000, 64
    wt = DT[kind.split("-")[0]]
    rng = np.random.default_rng(61)
    W0 = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(wt)
    idx, offs, go, kw, _ = _form_step(rng, "src", R, D, torch.float32)
    if kind.endswith("stoch"):
        go = go * 2.0 ** -12                                     # steps far below a bf16 ulp: the rounding decides

    def make():
        w = W0.clone().cuda().requires_grad_(True)
        return w, _fused(kind, "step", R)

    def call(w, fused):
        o = embedding_bag(idx, w, offs, mode="sum", include_last_offset=True, hook_features=kw["hook"], fused_sgd=fused,
                          presorted=kw["pre"], masked_indices=True, output_dtype=torch.float32)
        o.backward(go.view_as(o))

    we, fe = make()
    eager = []
    for _ in range(4):
        call(we, fe)
        eager.append((_bits(we), None if not hasattr(fe, "momentum") else _bits(fe.momentum)))
    assert not torch.equal(eager[0][0], eager[1][0])
    wg, fg = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(wg, fg)                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():
        wg.copy_(W0)                                                  # back to the start: table, state, step counter
        if hasattr(fg, "momentum"):
            fg.momentum.zero_()
        fg._ws_step[:8].zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(wg, fg)
    deltas = []
    for k in range(4):
        before = wg.detach().float().cpu()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(wg), eager[k][0]), k
        if eager[k][1] is not None:
            assert torch.equal(_bits(fg.momentum), eager[k][1]), k
        deltas.append(wg.detach().float().cpu() - before)
    assert int(fg._ws_step[:8].view(torch.int64).item()) == (0 if kind.startswith("fp32") else 4)
    if kind.endswith("stoch"):
        # the same gradient every replay: with one pattern of bits every replay would move the same elements
        assert not torch.equal(deltas[0] != 0, deltas[1] != 0) and not torch.equal(deltas[1] != 0, deltas[2] != 0)


# ---- 6. memory -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["fp32-adagrad", "bf16-sgd"])
def test_peak_memory_of_a_step_stays_below_one_cache_sized_tensor(kind):
    C, D, nnz = 200000, 128, 4096
    one = C * D * 4
    wt = DT[kind.split("-")[0]]
    rng = np.random.default_rng(71)
    idx = torch.from_numpy(rng.integers(0, C, nnz)).cuda()
    off = torch.arange(nnz + 1, device="cuda")
    go = torch.randn(nnz, D, device="cuda")
    peak = {}
    for acc in ("step", "cache"):
        w = torch.zeros(C, D, dtype=wt, device="cuda")
        fused = _fused(kind, acc, C)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _step(w, idx, off, go, fused)                                 # the first step: it allocates the workspace
        _step(w, idx, off, go, fused)
        torch.cuda.synchronize()
        peak[acc] = torch.cuda.max_memory_allocated() - base
        del w, fused
    assert peak["step"] < one < peak["cache"], (peak, one)


# ---- 7. module level -------------------------------------------------------------------------------------------------

def _module(N, D, C, strategy, freq, V0, table_dtype=None):
    import cachedembedding_amd as ce
    st = ce.EvictionStrategy.LFU if strategy == "lfu" else ce.EvictionStrategy.DATASET
    return ce.CachedEmbeddingBag(N, D, _weight=torch.from_numpy(V0.copy()), mode="sum", include_last_offset=True,
                                 cuda_row_num=C, ids_freq_mapping=freq, warmup_ratio=0.5, evict_strategy=st,
                                 strict=False, table_dtype=table_dtype, output_dtype=torch.float32)


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("strategy", ["dataset", "lfu"])
@pytest.mark.parametrize("kind", ["fp32-adagrad", "bf16-sgd"])
def test_module_under_eviction_equals_the_cache_sized_module(kind, strategy, mode):
    """N = 20000, a 3 % cache (600 rows), B = 512, F = 4, P = 4; every call draws its ids from a fresh pool of rows, so
    the cache evicts on every call; eager (the cache op inside forward, slots + offsets) and GraphedWindow with window
    keys.  Gradients lie on a 2^-6 grid (|g| <= 1): a row's sum over a step's 2048 lookups is exact in fp32 in any
    order, so the two modules see the same folded gradient whatever their atomics do."""
    import cachedembedding_amd as ce
    from cachedembedding_amd.pipeline import GraphedWindow
    N, D, B, P, lr = 20000, 32, 512, 4, 0.05
    C = int(0.03 * N)
    rng = np.random.default_rng(81)
    V0 = rng.standard_normal((N, D)).astype(np.float32)
    freq = rng.integers(0, 100, N) if strategy == "dataset" else None
    go = torch.from_numpy((rng.integers(-64, 65, (B, F, D)) / 64.0).astype(np.float32)).cuda()
    nwin = 6
    # the cache op runs once per call (eager) or once per window (graph): each draws its lookups from a fresh pool of
    # 280 rows -- two consecutive windows fit the 600 rows, the third cache op on evicts
    pool = 280
    windows = []
    for _ in range(nwin):
        win = []
        for i in range(P):
            if i == 0 or mode == "eager":
                rows = rng.choice(N, pool, replace=False)
            win.append(torch.from_numpy(rows[rng.integers(0, pool, F * B)]))
        windows.append(win)
    off = torch.arange(F * B + 1, dtype=torch.int32, device="cuda")
    hist, tables = [], []
    for acc in ("cache", "step"):
        emb = _module(N, D, C, strategy, freq, V0, DT[kind.split("-")[0]] if kind.startswith("bf16") else None)
        if kind.endswith("adagrad"):
            emb.set_fused_rowwise_adagrad(lr, accumulator=acc)
        else:
            emb.set_weight_rounding("nearest")
            emb.set_fused_sgd(lr, accumulator=acc)

        def step(slots, i, keys=None):
            out = emb(slots, off, hook_features=F, presorted=keys)
            out.backward(go)

        if mode == "graph":
            emb.set_cache_op(False)
            gw = GraphedWindow(emb, P, F * B, step, overlap=True, warmup_values=[v.cuda() for v in windows[0]],
                               presort=True, transport="worker", bag_layout=(off, True, F), arrangement="overlap")
            gw.submit([v.cuda() for v in windows[0]], 0)
            for k in range(nwin):
                if k + 1 < nwin:
                    gw.submit([v.cuda() for v in windows[k + 1]], (k + 1) % 2)
                gw.run(k % 2)
        else:
            for win in windows:
                for v in win:
                    step(v.cuda(), 0)
        torch.cuda.synchronize()
        mgr = emb.cache_weight_mgr
        assert mgr.sync_stats().status == 0
        wb = emb.num_write_back_history
        # (the first cache ops fill the cache; GraphedWindow's warm-up and first window both hold window 0)
        assert all(x > 0 for x in wb[4:]) and len(wb) >= nwin, ("the cache must evict on every call", wb)
        f = emb._fused()
        assert f.accumulator == acc
        if acc == "step":
            assert f._ws is None and f._ws16 is None and f._ws_step is not None
        emb.flush()
        hist.append((list(emb.num_hits_history), list(emb.num_miss_history), list(wb)))
        mom = getattr(mgr, "momentum1", None)
        tables.append((_bits(mgr.weight), None if mom is None else _bits(mom)))
        del emb
    assert hist[0] == hist[1]
    assert torch.equal(tables[0][0], tables[1][0])
    if tables[0][1] is not None:
        assert torch.equal(tables[0][1], tables[1][1])
    assert not torch.equal(tables[0][0], _bits(torch.from_numpy(V0).to(DT[kind.split("-")[0]])))
