"""GPU tests of the deterministic, accumulator-free fused row-wise Adagrad (ce_bag_backward_update_sorted): the fold
order, the fp64 reference, run-to-run and residency independence, bit equality with the atomic path for rows looked up
once, the -1 / last-row collision of the sort, 16-bit gradients and tables, graph capture, and the workspace.

A 16-bit table is rounded to nearest throughout: the sorted update refuses stochastic rounding (the last test).

The kernels only ever see in-range slots and the documented ignored slot -1."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import rowwise_adagrad_ref as ref  # noqa: E402
import table_dtype_ref as tref  # noqa: E402

pytestmark = pytest.mark.gpu
U = np.finfo(np.float32).eps / 2
W16 = [torch.bfloat16, torch.float16]
NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _bounds(rows, grads, R):
    """per row: lookups in the step, sum |terms| and |folded g| (max over d) -- the fp32 accumulation bound's inputs"""
    cnt = np.bincount(rows, minlength=R)
    s = np.zeros((R, grads.shape[1]))
    np.add.at(s, rows, np.abs(grads))
    g = np.zeros((R, grads.shape[1]))
    np.add.at(g, rows, grads)
    return cnt, s.max(axis=1), np.abs(g).max(axis=1)


class _Track:
    """fp64 reference state + per-row tolerances accumulated over the steps: the bound of
    tests/test_gpu_rowwise_adagrad.py, restated.  The sorted fold is a recursive summation too -- chunks of 64 in lookup
    order, then the partial sums in chunk order: every term passes through fewer than n - 1 additions -- so the same
    (n - 1) u S covers it."""

    def __init__(self, W0, N, lr, eps=1e-8, row_of=None):
        self.W, self.M = W0.astype(np.float64).copy(), np.zeros(N)
        self.lr, self.eps, self.row_of = lr, eps, row_of
        R = W0.shape[0]
        self.tol_w, self.tol_m = np.zeros(R), np.zeros(N)
        self.multi = np.zeros(R, bool)
        self.touched = np.zeros(R, bool)

    def step(self, rows, grads):
        R = self.W.shape[0]
        D = self.W.shape[1]
        cnt, s, gmax = _bounds(rows, grads, R)
        ref.step(self.W, self.M, rows, grads, self.lr, self.eps)
        idx = np.arange(R) if self.row_of is None else self.row_of
        m_now = np.maximum(self.M[idx], 1e-30)
        t = cnt > 0
        self.touched |= t
        self.multi |= cnt > 1
        # |fp32 fold - exact| <= (n - 1) u S per element (recursive summation): it moves m by <= 2 |g| e (+ the
        # rounding of a D-term sum of squares and of the add), and the update lr g / sqrt(m) by <= lr e / sqrt(m) plus
        # |update| * dm / (2 m), |update| <= lr sqrt(D)
        e = np.maximum(cnt - 1, 0) * U * s
        dm = 2 * gmax * e * 2 + 4 * (D + 2) * U * m_now
        dw = 2 * self.lr * e / np.sqrt(m_now) + self.lr * np.sqrt(D) * dm / m_now + 8 * self.lr * U * np.sqrt(D)
        self.tol_w += np.where(t, dw, 0)
        self.tol_m[idx[t]] += dm[t]

    def check(self, W, M):
        W, M = np.asarray(W, np.float64), np.asarray(M, np.float64)
        once = self.touched & ~self.multi
        np.testing.assert_allclose(W[once], self.W[once], rtol=1e-5, atol=1e-6)
        err = np.abs(W - self.W)
        lim = self.tol_w[:, None] + 1e-5 * np.abs(self.W) + 1e-6
        bad = np.nonzero(self.touched & (err > lim).any(1))[0]
        assert bad.size == 0, (bad[:5], err[bad[:5]].max(1), lim[bad[:5]].min(1))
        bad = np.nonzero(np.abs(M - self.M) > self.tol_m + 1e-6 * np.abs(self.M))[0]
        assert bad.size == 0, (bad[:5], M[bad[:5]], self.M[bad[:5]], self.tol_m[bad[:5]])


def _identity_grads(slots, go, R, hook=0):
    """ref.lookup_grads for one id per bag, without its Python loop: (rows, gradient rows) of the valid lookups"""
    slots = np.asarray(slots, np.int64)
    go = np.asarray(go, np.float64)
    D = go.shape[-1]
    if hook:
        go = go.reshape(-1, hook, D).transpose(1, 0, 2)
    go = go.reshape(-1, D)
    keep = (slots >= 0) & (slots < R)
    return slots[keep], go[keep]


def _step(w, idx, offs, go, fused, mode="sum", psw=None, hook=0, pre=None, masked=False):
    from cachedembedding_amd.functional import embedding_bag
    w.requires_grad_(True)
    o = embedding_bag(idx, w, offs, mode=mode, include_last_offset=True, per_sample_weights=psw, hook_features=hook,
                      fused_sgd=fused, presorted=pre, masked_indices=masked, output_dtype=go.dtype)
    o.backward(go.view_as(o))
    assert w.grad is None                                         # the update happened inside backward
    w.requires_grad_(False)


# ---- 1. fold order is lookup order ------------------------------------------------------------------------------------

@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("D", [8, 6])
def test_fold_order_is_lookup_order(D, swapped):
    """Row a at lookups 5, 20000, 40000 with constant gradient rows 1e8, 1, -1e8: the sequential fp32 sum is exactly 0,
    so W[a] and m[a] stay 0.  Row b at 7, 20001, 40001 with 1e8, -1e8, 1: g = 1 exactly, m[b] = 1, W[b] = -1.  Any
    other order of either sum gives another result.  swapped: a and b exchange their ids at 20000 / 20001 and at
    40000 / 40001, which exchanges the two gradient sequences and so the outcomes.

    eps: the issue asks for eps = 0, with which row a's update is 0 * (lr / (sqrt(0) + 0)) = 0 * inf = NaN under the
    arithmetic every path shares, and which every Adagrad entry refuses (eps > 0).  The smallest normal fp32 stands in:
    sqrt(m) + eps == sqrt(m) bit for bit for m = 1, so W[b] = -1 and m[b] = 1 stay exact."""
    from cachedembedding_amd.functional import FusedRowwiseAdagrad
    rng = np.random.default_rng(1)
    R, nnz = 70000, 3 * 16384
    a, b = 31234, 69999
    pool = np.setdiff1d(np.arange(R), [a, b])
    ids = rng.permutation(pool)[:nnz]
    go = rng.standard_normal((nnz, D)).astype(np.float32)
    for row, pos, vals in ((a, (5, 20000, 40000), (1e8, 1.0, -1e8)), (b, (7, 20001, 40001), (1e8, -1e8, 1.0))):
        for p, v in zip(pos, vals):
            ids[p] = row
            go[p] = v
    if swapped:
        ids[[20000, 40000]], ids[[20001, 40001]] = b, a
    assert len(np.unique(ids)) == nnz - 4
    w = torch.zeros(R, D, device="cuda")
    mom = torch.zeros(R, device="cuda")
    fused = FusedRowwiseAdagrad(1.0, eps=float(np.finfo(np.float32).tiny), momentum=mom, deterministic=True)
    _step(w, torch.from_numpy(ids).cuda(), torch.arange(nnz + 1, device="cuda"), torch.from_numpy(go).cuda(), fused)
    torch.cuda.synchronize()
    zero, one = (b, a) if swapped else (a, b)
    W, M = w.cpu().numpy(), mom.cpu().numpy()
    assert np.array_equal(W[zero], np.zeros(D, np.float32)) and M[zero] == 0.0, (W[zero], M[zero])
    assert np.array_equal(W[one], np.full(D, -1.0, np.float32)) and M[one] == 1.0, (W[one], M[one])
    other = ids[100]
    assert M[other] > 0 and np.abs(W[other]).min() > 0.0


# ---- 2. against the fp64 reference ------------------------------------------------------------------------------------

_RUNS = {}


def _run_form(form, D, K=3, fresh=False):
    """the shapes and forms of test_kernels_against_fp64_reference on the deterministic path: nnz = 4 segments of 16384
    lookups; rows 0..7 hot (a quarter of all lookups: ~2000 each per step), 1000 rows never looked up.  Cached per
    (form, D): the reference is computed once and left unchanged."""
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, presort_window
    if (form, D) in _RUNS and not fresh:
        return _RUNS[(form, D)]
    rng = np.random.default_rng(7)
    R, lr, F = 60000, 0.05, 4
    nnz = 4 * 16384
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    w = torch.from_numpy(W0).cuda()
    mom = torch.zeros(R, device="cuda")
    fused = FusedRowwiseAdagrad(lr, momentum=mom, deterministic=True)
    track = None if fresh else _Track(W0, R, lr)
    for k in range(K):
        ids = rng.integers(8, R - 1000, nnz)
        hot = rng.random(nnz) < 0.25
        ids[hot] = rng.integers(0, 8, int(hot.sum()))
        psw = None
        if form in ("sum", "psw", "src", "padding"):
            off = np.arange(nnz + 1)                                 # one id per bag, [B, F] output
            hook = F
        else:
            off = np.concatenate([np.sort(rng.choice(np.arange(1, nnz), nnz // 3 - 1, replace=False)), [0, nnz]])
            off = np.unique(off)
            hook = 0
        nb = len(off) - 1
        go = rng.standard_normal((nb // F, F, D) if hook else (nb, D)).astype(np.float32)
        if form == "psw":
            psw = rng.random(nnz).astype(np.float32)
        slots = ids.copy()
        if form == "padding":
            slots[rng.random(nnz) < 0.1] = -1                         # ignored lookups
        idx = torch.from_numpy(slots).cuda()
        offs = torch.from_numpy(off).cuda()
        pre = None
        if form == "src":                                             # keys are passed and ignored
            pre = presort_window(idx.view(1, -1), R, offsets=offs.to(torch.int32), include_last_offset=True,
                                 hook_features=hook, identity_bags=True)[0]
        _step(w, idx, offs, torch.from_numpy(go).cuda(), fused, mode="mean" if form == "mean" else "sum",
              psw=None if psw is None else torch.from_numpy(psw).cuda(), hook=hook, pre=pre, masked=form == "padding")
        if track is not None:
            if form in ("mean", "psw"):
                rows, grads = ref.lookup_grads(slots, off, go, R, psw=psw, mode="mean" if form == "mean" else "sum",
                                               include_last_offset=True, hook_features=hook)
            else:
                rows, grads = _identity_grads(slots, go, R, hook)
                if k == 0 and form == "padding" and D == 6:          # the vectorised form is lookup_grads
                    r2, g2 = ref.lookup_grads(slots, off, go, R, include_last_offset=True, hook_features=hook)
                    assert np.array_equal(rows, r2) and np.array_equal(grads, g2)
            track.step(rows, grads)
    torch.cuda.synchronize()
    assert fused._ws is None and fused._ws16 is None, "the accumulator workspaces must never be allocated"
    res = dict(W0=W0, W=w.cpu(), M=mom.cpu(), track=track, R=R)
    if not fresh:
        _RUNS[(form, D)] = res
    return res


@pytest.mark.parametrize("D", [128, 6])
@pytest.mark.parametrize("form", ["sum", "mean", "psw", "padding", "src"])
def test_against_fp64_reference(form, D):
    r = _run_form(form, D)
    R, track = r["R"], r["track"]
    Wg, Mg = r["W"].numpy(), r["M"].numpy()
    never = np.arange(R - 1000, R)
    assert np.array_equal(Wg[never], r["W0"][never]) and np.all(Mg[never] == 0)
    assert track.multi[:8].all() and (track.touched & ~track.multi).sum() > 1000
    track.check(Wg, Mg)


# ---- 3. run to run, and independent of residency ----------------------------------------------------------------------

def test_run_to_run_bit_equal():
    first = _run_form("sum", 128)
    again = _run_form("sum", 128, fresh=True)
    assert torch.equal(_bits(first["W"]), _bits(again["W"])) and torch.equal(_bits(first["M"]), _bits(again["M"]))


def test_independent_of_cache_size_and_eviction():
    """the 24-step id stream of test_through_cache_that_evicts through a 3 % DATASET cache and a 10 % LFU cache.  The
    DATASET cache keeps the host table in frequency order (id i lives in row idx_map[i]), the LFU cache in id order, so
    both tables are filled id by id with the same values first; after flush() the two host tables and the two momentum1
    are bit-equal id by id, and within the fp64 bounds."""
    import cachedembedding_amd as ce
    N, D, F, B, lr = 20000, 32, 4, 128, 0.1
    V0 = np.random.default_rng(11).standard_normal((N, D)).astype(np.float32)        # row i: the value of id i
    freq = np.random.default_rng(12).integers(0, 100, N)
    out = []
    for share, strategy, fq in ((0.03, ce.EvictionStrategy.DATASET, freq), (0.10, ce.EvictionStrategy.LFU, None)):
        emb = ce.CachedEmbeddingBag(N, D, sparse=True, _weight=torch.from_numpy(V0.copy()), mode="sum",
                                    include_last_offset=True, cuda_row_num=int(share * N), ids_freq_mapping=fq,
                                    warmup_ratio=0.5, evict_strategy=strategy, strict=False)
        mgr = emb.cache_weight_mgr
        imap = mgr.idx_map.cpu().numpy().astype(np.int64)
        emb.flush()                                                   # empty the warmed cache, then fill by id
        mgr.weight[torch.from_numpy(imap)] = torch.from_numpy(V0)
        emb.set_fused_rowwise_adagrad(lr, deterministic=True)
        track = _Track(V0, N, lr)                                     # the reference runs in id space
        rng = np.random.default_rng(13)
        off = torch.arange(F * B + 1, device="cuda")
        for it in range(24):
            ids = (rng.random(F * B) ** 2 * N).astype(np.int64)
            go = rng.standard_normal((B, F, D)).astype(np.float32)
            o = emb(torch.from_numpy(ids).cuda(), off, hook_features=F)
            o.backward(torch.from_numpy(go).cuda())
            track.step(*_identity_grads(ids, go, N, F))
        torch.cuda.synchronize()
        assert mgr.cuda_cached_weight.grad is None
        assert sum(emb.num_write_back_history) > 0, "the cache never evicted"
        emb.flush()
        f = emb.fused_adagrad
        assert f._ws is None and f._ws16 is None and f._ws_sorted is not None
        Wi, Mi = mgr.weight.numpy()[imap].copy(), mgr.momentum1.cpu().numpy()[imap].copy()
        track.check(Wi, Mi)
        out.append((Wi, Mi, imap))
    assert not np.array_equal(out[0][2], out[1][2])                 # the two caches do hold their rows differently
    assert np.array_equal(out[0][0].view(np.int32), out[1][0].view(np.int32))
    assert np.array_equal(out[0][1].view(np.int32), out[1][1].view(np.int32))


# ---- 4. single-lookup rows equal the atomic / accumulator path bit for bit --------------------------------------------

def _once(D, kind, R, n, pad):
    from cachedembedding_amd.functional import FusedRowwiseAdagrad
    wt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[kind.split("-")[0]]
    rng = np.random.default_rng(21)
    W0 = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(wt)
    state = []
    for det in (False, True):
        w = W0.clone().cuda()
        mom = torch.zeros(R, device="cuda")
        fused = FusedRowwiseAdagrad(0.05, momentum=mom, deterministic=det)
        fused.rounding = "nearest"
        srng = np.random.default_rng(22)
        steps = []
        for k in range(2):
            slots = np.concatenate([srng.permutation(R)[:n], np.full(pad, -1)])
            slots = slots[srng.permutation(n + pad)]
            go = srng.standard_normal((n + pad, D)).astype(np.float32)
            _step(w, torch.from_numpy(slots).cuda(), torch.arange(n + pad + 1, device="cuda"),
                  torch.from_numpy(go).cuda(), fused, masked=True)
            steps.append((_bits(w), _bits(mom)))
        state.append(steps)
        if det:
            assert fused._ws is None and fused._ws16 is None
    for k in range(2):
        assert torch.equal(state[0][k][1], state[1][k][1]), (k, "momentum")
        assert torch.equal(state[0][k][0], state[1][k][0]), (k, "weight")
    assert not torch.equal(state[1][0][0], _bits(W0))


@pytest.mark.parametrize("kind", ["fp32", "bf16-nearest", "fp16-nearest"])
@pytest.mark.parametrize("D", [128, 8])
def test_rows_looked_up_once_equal_the_atomic_path(D, kind):
    """2 * 16384 + 5 lookups of pairwise distinct rows + 251 ignored slots, two consecutive steps: the Adagrad
    arithmetic and the rounding to nearest are the same"""
    _once(D, kind, 40000, 2 * 16384 + 5, 251)


@pytest.mark.parametrize("D,kind", [(512, "fp32"), (512, "bf16-nearest"), (768, "fp32"), (1024, "fp32"),
                                    (1024, "fp16-nearest"), (6, "fp32"), (70, "fp32"), (130, "fp32"), (250, "fp32")])
def test_rows_looked_up_once_every_lane_shape(D, kind):
    """the same on the other lane shapes -- the sum of squares is spelled out per shape (lane_sq_sum): the vector form
    with 2 chunks per lane (D = 512), 3 rounded up to 4 (768) and 4 (1024), and the scalar form (dim % 4 != 0) with 1, 2,
    3-of-4 and 4 chunks per lane (D = 6, 70, 130, 250); 2500 distinct rows + 37 ignored slots of a table of 3000"""
    _once(D, kind, 3000, 2500, 37)


# ---- 5. the -1 / last-row collision -----------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [65536, 65537])
def test_ignored_lookups_do_not_split_the_last_rows_run(R):
    """R = 2^16: a raw -1 key shares all 16 sorted bits with row 65535, and a stable sort would interleave the two in
    lookup order -- several run heads for row 65535, several Adagrad updates.  Row 65535 (and, for R = 2^16 + 1, the last
    row 65536 as well) is looked up 40 times among 400 ignored slots and random other rows; m equals the reference's SINGLE update (R = 2^16 + 1: one more sorted bit)."""
    from cachedembedding_amd.functional import FusedRowwiseAdagrad
    rng = np.random.default_rng(R)
    D, nnz, lr = 8, 8192, 0.05
    slots = rng.integers(0, 65535, nnz)
    last = sorted({65535, R - 1})
    special = rng.permutation(nnz)[:400 + 40 * len(last)]           # random places: interleaved in lookup order
    slots[special[:400]] = -1
    for k, row in enumerate(last):
        slots[special[400 + 40 * k:440 + 40 * k]] = row
    assert all((slots == row).sum() == 40 for row in last) and (slots == -1).sum() == 400
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    go = rng.standard_normal((nnz, D)).astype(np.float32)
    w = torch.from_numpy(W0).cuda()
    mom = torch.zeros(R, device="cuda")
    fused = FusedRowwiseAdagrad(lr, momentum=mom, deterministic=True)
    _step(w, torch.from_numpy(slots).cuda(), torch.arange(nnz + 1, device="cuda"), torch.from_numpy(go).cuda(), fused,
          masked=True)
    torch.cuda.synchronize()
    track = _Track(W0, R, lr)
    rows, grads = _identity_grads(slots, go, R)
    track.step(rows, grads)
    Wg, Mg = w.cpu().numpy(), mom.cpu().numpy()
    track.check(Wg, Mg)
    for row in last:
        g = grads[rows == row].sum(0)
        single = float((g * g).sum() / D)
        per_lookup = float((grads[rows == row] ** 2).sum() / D)     # what one update per lookup would leave in m
        assert abs(Mg[row] - single) <= track.tol_m[row] + 1e-6 * single, (row, Mg[row], single)
        assert abs(per_lookup - single) > 100 * (track.tol_m[row] + 1e-6 * single)
    untouched = np.setdiff1d(np.arange(R), rows)
    assert np.array_equal(Wg[untouched], W0[untouched]) and np.all(Mg[untouched] == 0)


# ---- 6. 16-bit gradient and 16-bit table ------------------------------------------------------------------------------

@pytest.mark.parametrize("gt", [torch.float32] + W16, ids=lambda d: "grad_" + NAMES[d])
@pytest.mark.parametrize("wt", [torch.float32] + W16, ids=lambda d: "table_" + NAMES[d])
def test_16_bit_gradient_and_table(wt, gt):
    """test 2's sum shape at D = 128, 2 steps, nearest rounding: within table_dtype_ref's update_bound with E from the
    Adagrad fp32 evaluation (the bound of tests/test_gpu_table_dtype.py's Adagrad case, restated; an fp32 table is held
    to E itself), and a 16-bit grad_out gives the bits of its exact .float() upcast fed as fp32"""
    from cachedembedding_amd.functional import FusedRowwiseAdagrad
    rng = np.random.default_rng(7)
    R, D, lr, F, nnz = 60000, 128, 0.05, 4, 4 * 16384
    t0 = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(wt)
    runs = [gt] if gt == torch.float32 else [gt, torch.float32]      # the second run: the upcast gradient as fp32
    ws = [t0.clone().cuda() for _ in runs]
    moms = [torch.zeros(R, device="cuda") for _ in runs]
    fuseds = [FusedRowwiseAdagrad(lr, momentum=m, deterministic=True) for m in moms]
    for f in fuseds:
        f.rounding = "nearest"
    offs = torch.arange(nnz + 1, device="cuda")
    cur = t0.clone()
    track = _Track(t0.float().numpy(), R, lr)
    for k in range(2):
        ids = rng.integers(8, R - 1000, nnz)
        hot = rng.random(nnz) < 0.25
        ids[hot] = rng.integers(0, 8, int(hot.sum()))
        go = torch.from_numpy(rng.standard_normal((nnz // F, F, D)).astype(np.float32)).to(gt)
        idx = torch.from_numpy(ids).cuda()
        for w, f, dt in zip(ws, fuseds, runs):
            _step(w, idx, offs, go.to(dt).cuda(), f, hook=F)
        got = ws[0].detach().cpu()
        rows, grads = _identity_grads(ids, go.float().numpy(), R, F)
        old = cur.float().numpy().astype(np.float64)
        track.W[:] = old                                              # the update starts from the table's old row
        track.tol_w[:] = 0
        track.step(rows, grads)
        x64 = track.W
        E = track.tol_w[:, None] + 1e-5 * np.abs(x64) + 1e-6
        lim = E if wt == torch.float32 else tref.update_bound(x64, E, wt)
        touched = np.bincount(rows, minlength=R) > 0
        err = np.abs(got.double().numpy() - x64)
        bad = np.nonzero(touched[:, None] & (err > lim))
        assert bad[0].size == 0, (k, bad[0][:5], err[bad][:5], lim[bad][:5])
        M = moms[0].cpu().double().numpy()
        bad = np.nonzero(np.abs(M - track.M) > track.tol_m + 1e-6 * np.abs(track.M))[0]
        assert bad.size == 0, (k, bad[:5], M[bad[:5]], track.M[bad[:5]])
        assert torch.equal(_bits(got[~torch.from_numpy(touched)]), _bits(cur[~torch.from_numpy(touched)])), \
            "rows never looked up must not move"
        assert (~touched).sum() >= 1000 and track.multi[:8].all()
        cur = got.clone()
    if len(runs) == 2:
        assert torch.equal(_bits(ws[0]), _bits(ws[1])) and torch.equal(_bits(moms[0]), _bits(moms[1]))


# ---- 7. graph capture -------------------------------------------------------------------------------------------------

def test_graph_replay_equals_eager_steps():
    """a captured step (static index / gradient buffers, bf16 table, rounded to nearest) replayed 3 times equals 3 eager
    steps, bit for bit: sort, memset node, fold and combine are capture-safe and carry nothing over in the workspace"""
    from cachedembedding_amd import _lib
    lib = _lib.lib
    rng = np.random.default_rng(41)
    R, D, nnz, seed = 5000, 64, 3000, 99
    slots = rng.integers(0, R, nnz)
    slots[rng.random(nnz) < 0.3] = 17                               # a run of ~900 lookups: chunks and partial rows
    slots[rng.random(nnz) < 0.05] = -1
    assert (slots == 17).sum() > 5 * _lib.CE_SORTED_CHUNK
    idx = torch.from_numpy(slots).cuda()
    off = torch.arange(nnz + 1, device="cuda")
    go = torch.from_numpy(rng.standard_normal((nnz, D)).astype(np.float32)).to(torch.bfloat16).cuda()
    W0 = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(torch.bfloat16)
    need = lib.ce_bag_backward_update_sorted_workspace(R, nnz, D)

    def make():
        return W0.clone().cuda(), torch.zeros(R, device="cuda"), torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(w, mom, ws):
        _lib.check(lib.ce_bag_backward_update_sorted(
            w.data_ptr(), _lib.CE_ACT_BF16, R, D, idx.data_ptr(), nnz, off.data_ptr(), 1, nnz, 1, None,
            _lib.CE_MODE_SUM, 0, go.data_ptr(), _lib.CE_ACT_BF16, None, mom.data_ptr(), R, 0.05, 1e-8,
            _lib.CE_OPT_ROWWISE_ADAGRAD, _lib.CE_ROUND_NEAREST, seed, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))

    we, me, wse = make()
    eager = []
    for _ in range(3):
        call(we, me, wse)
        eager.append((_bits(we), _bits(me)))
    assert not torch.equal(eager[0][0], eager[1][0])
    wg, mg, wsg = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(wg, mg, wsg)                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    wg.copy_(W0)                                                      # back to the start
    mg.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(wg, mg, wsg)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(wg), eager[k][0]) and torch.equal(_bits(mg), eager[k][1]), k


# ---- 8. workspace -----------------------------------------------------------------------------------------------------

def test_workspace_size_and_no_accumulator():
    from cachedembedding_amd import _lib
    from cachedembedding_amd.functional import FusedRowwiseAdagrad
    lib = _lib.lib
    f = lib.ce_bag_backward_update_sorted_workspace
    assert f(2 ** 20, 425984, 128) == f(2 ** 27, 425984, 128) > 0
    assert f(1779442, 425984, 128) < lib.ce_bag_backward_rowwise_adagrad_workspace(1779442, 128) // 8
    rng = np.random.default_rng(3)
    R, D, nnz = 3000, 16, 700
    for wt in (torch.float32, torch.bfloat16):
        w = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(wt).cuda()
        mom = torch.zeros(R, device="cuda")
        fused = FusedRowwiseAdagrad(0.1, momentum=mom, deterministic=True)
        fused.rounding = "nearest"
        before = w.clone()
        idx = torch.from_numpy(rng.integers(0, 50, nnz)).cuda()
        _step(w, idx, torch.arange(nnz + 1, device="cuda"), torch.randn(nnz, D, device="cuda"), fused)
        torch.cuda.synchronize()
        assert fused._ws is None and fused._ws16 is None
        assert fused._ws_sorted.numel() == f(R, nnz, D)
        assert int(torch.count_nonzero(mom)) == int(torch.unique(idx).numel())
        assert not torch.equal(w[:50], before[:50]) and torch.equal(w[50:], before[50:])
        # a larger step: the workspace grows
        big = torch.from_numpy(rng.integers(0, 50, 4 * nnz)).cuda()
        _step(w, big, torch.arange(4 * nnz + 1, device="cuda"), torch.randn(4 * nnz, D, device="cuda"), fused)
        assert fused._ws_sorted.numel() == f(R, 4 * nnz, D)


# ---- 9. stochastic rounding is refused ---------------------------------------------------------------------------------

@pytest.mark.parametrize("wt", W16, ids=lambda d: "table_" + NAMES[d])
def test_stochastic_rounding_is_refused_before_any_kernel(wt):
    """a 16-bit table with rounding = "stochastic" (the default) is a NotImplementedError of the forward: nothing has
    run, the table and the state are untouched and no workspace exists; the C entry answers CE_ERR_UNSUPPORTED"""
    from cachedembedding_amd import _lib
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, embedding_bag
    R, D, nnz = 300, 16, 64
    w = torch.ones(R, D, dtype=wt, device="cuda")
    mom = torch.zeros(R, device="cuda")
    fused = FusedRowwiseAdagrad(0.1, momentum=mom, deterministic=True)
    assert fused.rounding == "stochastic"
    idx = torch.arange(nnz, device="cuda")
    off = torch.arange(nnz + 1, device="cuda")
    w.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="stochastic"):
        embedding_bag(idx, w, off, mode="sum", include_last_offset=True, fused_sgd=fused)
    go = torch.ones(nnz, D, device="cuda")
    ws = torch.zeros(_lib.lib.ce_bag_backward_update_sorted_workspace(R, nnz, D), dtype=torch.uint8, device="cuda")
    rc = _lib.lib.ce_bag_backward_update_sorted(
        w.data_ptr(), _lib.ACT_DTYPES[wt], R, D, idx.data_ptr(), nnz, off.data_ptr(), 1, nnz, 1, None, _lib.CE_MODE_SUM,
        0, go.data_ptr(), _lib.CE_ACT_F32, None, mom.data_ptr(), R, 0.1, 1e-8, _lib.CE_OPT_ROWWISE_ADAGRAD,
        _lib.CE_ROUND_STOCHASTIC, 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    assert rc == _lib.CE_ERR_UNSUPPORTED and "CE_ROUND_STOCHASTIC" in _lib.last_error()
    torch.cuda.synchronize()
    assert fused._ws_sorted is None and int(torch.count_nonzero(ws)) == 0 and int(torch.count_nonzero(mom)) == 0
    assert bool((w.detach() == 1).all())


# ---- 10. CE_OPT_SGD at the C level -------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [32, 6])
def test_sgd_through_the_c_entry(D):
    """x = w - lr * g without momentum, row_of_slot or eps: 3000 lookups of 400 rows of a table of 1000 (row 5 has 700 of
    them: chunks and the combine pass), 5 % ignored, against fp64.  Bound per element: the fold's (n - 1) u S (recursive
    summation, S = sum |terms|), times lr, plus the rounding of lr * g and of the subtraction, 2 u (|w| + lr |g|); rows
    never looked up keep their bits."""
    from cachedembedding_amd import _lib
    lib = _lib.lib
    rng = np.random.default_rng(51)
    R, nnz, lr = 1000, 3000, 0.25
    slots = rng.integers(0, 400, nnz)
    slots[rng.random(nnz) < 0.25] = 5
    slots[rng.random(nnz) < 0.05] = -1
    assert (slots == 5).sum() > 5 * _lib.CE_SORTED_CHUNK
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    go = rng.standard_normal((nnz, D)).astype(np.float32)
    w = torch.from_numpy(W0).cuda()
    idx, off, g = torch.from_numpy(slots).cuda(), torch.arange(nnz + 1, device="cuda"), torch.from_numpy(go).cuda()
    ws = torch.empty(lib.ce_bag_backward_update_sorted_workspace(R, nnz, D), dtype=torch.uint8, device="cuda")
    _lib.check(lib.ce_bag_backward_update_sorted(
        w.data_ptr(), _lib.CE_ACT_F32, R, D, idx.data_ptr(), nnz, off.data_ptr(), 1, nnz, 1, None, _lib.CE_MODE_SUM, 0,
        g.data_ptr(), _lib.CE_ACT_F32, None, None, 0, lr, 0.0, _lib.CE_OPT_SGD, _lib.CE_ROUND_NEAREST, 0,
        ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    rows, grads = _identity_grads(slots, go, R)
    cnt = np.bincount(rows, minlength=R)
    G = np.zeros((R, D))
    S = np.zeros((R, D))
    np.add.at(G, rows, grads)
    np.add.at(S, rows, np.abs(grads))
    want = W0.astype(np.float64) - lr * G
    lim = lr * np.maximum(cnt - 1, 0)[:, None] * U * S + 2 * U * (np.abs(W0) + lr * np.abs(G)) + 1e-30
    got = w.cpu().numpy()
    err = np.abs(got - want)
    assert (err <= lim).all(), (np.argwhere(err > lim)[:5], err.max())
    assert np.array_equal(got[cnt == 0], W0[cnt == 0]) and (cnt == 0).sum() >= 600
    assert not np.array_equal(got[5], W0[5])
