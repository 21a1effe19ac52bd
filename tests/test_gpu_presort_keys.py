"""The keys every presort producer writes, held to the numpy model of the key contract (tests/presort_ref.py) -- not to
another kernel -- and the consumers of flagged keys and of layouts with lookups that no bag covers.

Producers: presort_slots, presort_window plain / offsets= / ids=, CachedParamMgr.prepare_ids_keys.  Only the documented
ignored slots (-1, num_rows, num_rows + 3) are used, and no kernel is handed a key array a presort did not write."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import presort_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

R = 70000
SEG = pr.SEG
NS = [1, 15, 16, 17, 1000, 16383, 16384, 16385, 2 * 16384 + 5]
PATTERNS = ["distinct", "one_row", "hot_but_lookup_1000", "shared_bucket", "bucket_32_and_33", "run_ends_on_15",
            "run_crosses_15_16", "only_ignored", "num_rows_1", "power_law"]


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def _with_ignored(core, n, num_rows, rng, fill):
    """core rows + the three ignored slots (a batch of 8 lookups or more) + rows from `fill` up to n lookups; the first
    segment, which holds all of core, is shuffled.  A batch too short for core is the front of it."""
    bad = np.array([-1, num_rows, num_rows + 3] if n >= 8 else [], np.int64)
    core = np.asarray(core, np.int64)
    if n < core.size + bad.size:
        return np.concatenate([bad, core])[:n]
    s = np.concatenate([core, bad, fill[:n - core.size - bad.size]]).astype(np.int64)
    assert s.size == n
    s[:SEG] = rng.permutation(s[:SEG])
    return s


def _slots(pattern, n, batch, rng):
    """(slots of one batch, num_rows)"""
    free = np.arange(100, R)
    free = rng.permutation(free[(free & 8191) >= 16])               # rows of their own, outside buckets 0..15
    none = np.zeros(0, np.int64)
    if pattern == "distinct":
        return _with_ignored(none, n, R, rng, free), R
    if pattern == "one_row":                                        # whole waves hold one bucket: 64 places, one atomic
        return _with_ignored(none, n, R, rng, np.full(n, 4097 + batch)), R
    if pattern == "hot_but_lookup_1000":
        s = _with_ignored(none, n, R, rng, np.full(n, 12345))
        if n > 1000:
            if s[1000] != 12345:                                    # an ignored slot landed there: it moves on
                s[np.nonzero(s[1001:] == 12345)[0][0] + 1001] = s[1000]
            s[1000] = 12346 + batch
        return s, R
    if pattern == "shared_bucket":                                  # r, r + 8192, r + 16384: three runs of two per bucket
        base = 16 + np.arange(-(-n // 6))
        rows = np.concatenate([base, base + 8192, base + 16384] * 2)
        return _with_ignored(none, n, R, rng, rng.permutation(rows)), R
    if pattern == "bucket_32_and_33":
        core = np.concatenate([np.repeat([5, 8197], 16), np.repeat([6, 8198], [17, 16])])
        return _with_ignored(core, n, R, rng, free), R
    if pattern == "run_ends_on_15":                                 # bucket 0 comes first: row 0 at 0..9, row 8192 at 10..15
        return _with_ignored(np.repeat([0, 8192], [10, 6]), n, R, rng, free), R
    if pattern == "run_crosses_15_16":                              # ... row 8192 at 10..16
        return _with_ignored(np.repeat([0, 8192], [10, 7]), n, R, rng, free), R
    if pattern == "only_ignored":
        return np.resize(np.array([-1, R, R + 3]), n).astype(np.int64), R
    if pattern == "num_rows_1":
        s = np.zeros(n, np.int64)
        if n >= 8:
            s[[1, 4, 6]] = [-1, 1, 4]
        return s, 1
    if pattern == "power_law":
        s = (rng.random(n) ** 3 * R).astype(np.int64).clip(0, R - 1)
        if n >= 8:
            s[[2, 5, n - 1]] = [-1, R, R + 3]
        return s, R
    raise AssertionError(pattern)


def _divisor(n):
    return next((f for f in range(2, 30) if n % f == 0), 0) if n > 1 else 0


def _check_src(keys, slots, num_rows, n, form, offsets, last, nb, F, ids=None):
    """every batch of a list of SrcKeys against the model; returns the flags found"""
    flags = 0
    for b, k in enumerate(keys):
        off = None if offsets is None else (offsets[b] if offsets.ndim == 2 else offsets)
        plan = pr.lookup_plan(slots[b], num_rows, off, last, nb, F)
        assert (k.num_bags, k.include_last_offset, k.hook_features) == (nb, last, F)
        assert (k.ranges is None) == (form != "src_excl")
        st = pr.check_keys(k.keys.cpu().numpy(), plan, n, form, ids=None if ids is None else ids[b],
                           ranges=None if k.ranges is None else k.ranges.cpu().numpy())
        flags += st["flags"]
    return flags


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_producer_keeps_the_key_contract(pattern, n):
    from cachedembedding_amd.functional import presort_slots, presort_window
    for P in (1, 3):
        rng = np.random.default_rng([PATTERNS.index(pattern), n, P])
        per = [_slots(pattern, n, b, rng) for b in range(P)]
        num_rows = per[0][1]
        slots = np.stack([s for s, _ in per])
        if n < 8 and P == 3 and pattern != "num_rows_1":            # too short for the three of them: one each
            slots[1, 0], slots[2, 0] = -1, num_rows + 3
        sd = _dev(slots)
        plain = [pr.lookup_plan(slots[b], num_rows, None, True, n, 0) for b in range(P)]
        # ---- constructed runs: the model decides before the GPU is asked
        want_run = {"run_ends_on_15": (10, 15, True), "run_crosses_15_16": (10, 16, False)}.get(pattern)
        if want_run and n >= 1000:
            for b in range(P):
                model = pr.build_keys(plain[b], n, "src_excl", rng=np.random.default_rng(b))
                assert pr.run_of(model, num_rows, 0, 0) == (0, 9, True)
                assert pr.run_of(model, num_rows, 0, 8192) == want_run
        # ---- row << 32 | lookup: one batch, and the window
        pr.check_keys(presort_slots(sd[0], num_rows).cpu().numpy(), plain[0], n, "lookup")
        kw = presort_window(sd, num_rows).cpu().numpy()
        assert kw.shape == (P, pr.presort_len(n))
        for b in range(P):
            pr.check_keys(kw[b], plain[b], n, "lookup")
        # ---- source-row keys, one id per bag: stated / read from int32 shared, int64 per-batch offsets
        F = _divisor(n)
        ar = np.arange(n + 1)
        o32 = _dev(ar, torch.int32)
        o64 = _dev(np.tile(ar, (P, 1)))
        got = presort_window(sd, num_rows, offsets=o32, include_last_offset=True, hook_features=F, identity_bags=True)
        assert all(k.identity for k in got)
        _check_src(got, slots, num_rows, n, "src", None, True, n, F)
        got = presort_window(sd, num_rows, offsets=o64, include_last_offset=True, hook_features=0)
        _check_src(got, slots, num_rows, n, "src", np.tile(ar, (P, 1)), True, n, 0)
        got = presort_window(sd, num_rows, offsets=o32[:n], include_last_offset=False, hook_features=F)
        _check_src(got, slots, num_rows, n, "src", ar[:n], False, n, F)
        # ---- owner-exclusive keys + id ranges (ids: a map of the slots that keeps ignored lookups apart)
        ids = slots * 3 + 11
        idd = _dev(ids)
        got = presort_window(sd, num_rows, offsets=o32, include_last_offset=True, hook_features=F, ids=idd)
        flags = _check_src(got, slots, num_rows, n, "src_excl", ar, True, n, F, ids)
        got = presort_window(sd, num_rows, offsets=o64, include_last_offset=True, hook_features=0, ids=idd,
                             identity_bags=True)
        assert flags == _check_src(got, slots, num_rows, n, "src_excl", None, True, n, 0, ids)
        if pattern in ("distinct", "shared_bucket", "run_ends_on_15", "run_crosses_15_16", "bucket_32_and_33"):
            assert flags > 0, "the flag checks must run on inputs that have flags"
        if pattern in ("one_row", "only_ignored") and 32 + 3 < n <= SEG:      # (a short last segment is one small run)
            assert flags == 0
        if want_run and n >= 1000:
            for b in range(P):
                k = got[b].keys.cpu().numpy()
                assert pr.run_of(k, num_rows, 0, 0) == (0, 9, True) and pr.run_of(k, num_rows, 0, 8192) == want_run


@pytest.mark.parametrize("hook", [0, 4])
@pytest.mark.parametrize("off_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("shared", [False, True])
def test_ragged_layouts(shared, off_dtype, hook):
    """the ragged layout of test_source_row_keys_backward_matches_tile_backward (3000 bags of 0..8 lookups, some
    empty, 17000 lookups per batch) and the same bags read as [750, 4] samples x features"""
    from cachedembedding_amd.functional import presort_window
    g = torch.Generator().manual_seed(20 + hook)
    C, P, nb, n = 5000, 3, 3000, 17000
    lens = torch.randint(0, 9, (P, nb), generator=g)
    lens[:, -1] += n - lens.sum(1)
    assert (lens >= 0).all() and (lens == 0).sum() > 100
    offs = torch.cat([torch.zeros(P, 1, dtype=torch.int64), lens.cumsum(1)], 1)
    if shared:
        offs = offs[0]
    slots = torch.randint(0, C, (P, n), generator=g)
    slots = torch.where(torch.rand(P, n, generator=g) < 0.3, torch.randint(0, 8, (P, n), generator=g), slots)
    slots[:, 5], slots[:, 77], slots[:, 16390] = -1, C + 3, C
    sd, od = slots.cuda().contiguous(), offs.to(off_dtype).cuda().contiguous()
    s, o = slots.numpy(), offs.numpy()
    got = presort_window(sd, C, offsets=od, include_last_offset=True, hook_features=hook)
    _check_src(got, s, C, n, "src", o, True, nb, hook)
    ids = s + 1000
    got = presort_window(sd, C, offsets=od, include_last_offset=True, hook_features=hook, ids=_dev(ids))
    assert _check_src(got, s, C, n, "src_excl", o, True, nb, hook, ids) > 1000
    # without the last offset: the last bag ends with the batch
    got = presort_window(sd, C, offsets=od[..., :nb].contiguous(), include_last_offset=False, hook_features=hook)
    _check_src(got, s, C, n, "src", o[..., :nb], False, nb, hook)


@pytest.mark.parametrize("src", [False, True])
def test_prepare_ids_keys(src):
    """the cache op's fused form: slots and keys out of its last kernel, the keys checked against the slots it wrote;
    then a window that overflows the cache (non-strict): every slot -1, every key an ignored one"""
    import cachedembedding_amd as ce
    rng = np.random.default_rng(12)
    N, C, D, P, n, nb = 20000, 14000, 8, 3, 17000, 3400       # ~11,900 distinct ids per window
    mgr = ce.CachedParamMgr(torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32)), C,
                            evict_strategy=ce.EvictionStrategy.LFU)
    mgr.reorder(rng.integers(0, 100, N), 0.6)
    klen = pr.presort_len(n)
    layouts = [dict()]
    if src:
        lens = rng.multinomial(n, np.ones(nb) / nb, size=P)
        ragged = np.concatenate([np.zeros((P, 1), np.int64), lens.cumsum(1)], 1)
        layouts = [dict(offsets=np.arange(n + 1), include_last_offset=True, hook_features=4, identity_bags=True),
                   dict(offsets=ragged, include_last_offset=True, hook_features=4),
                   dict(offsets=ragged[0, :nb], include_last_offset=False, hook_features=0)]
    for it, lay in enumerate(layouts + layouts[-1:]):
        overflow = it == len(layouts)
        if overflow:
            mgr.strict = False
            ids = (np.arange(P * n).reshape(P, n) * 7) % N
        else:
            ids = (rng.random((P, n)) ** 6 * N).astype(np.int64)
        slots = torch.empty(P, n, dtype=torch.int64, device="cuda")
        keys = torch.empty(P, klen, dtype=torch.int64, device="cuda")
        kw = dict(lay)
        off = kw.pop("offsets", None)
        if off is not None:
            kw["offsets"] = _dev(off, torch.int32 if it % 2 else torch.int64)
        mgr.prepare_ids_keys(_dev(ids), slots, keys, **kw)
        torch.cuda.synchronize()
        s, k = slots.cpu().numpy(), keys.cpu().numpy()
        assert (s == -1).all() if overflow else ((s >= 0) & (s < C)).all()
        for b in range(P):
            if not src:
                plan = pr.lookup_plan(s[b], C, None, True, n, 0)
            else:
                ob = None if lay.get("identity_bags") else (off[b] if off.ndim == 2 else off)
                last = lay["include_last_offset"]
                plan = pr.lookup_plan(s[b], C, ob, last, n if ob is None else len(ob) - int(last), lay["hook_features"])
            st = pr.check_keys(k[b], plan, n, "src" if src else "lookup")
            assert st["live"] == (0 if overflow else n)
    mgr.sync_stats()


# ---- consumers of flagged keys --------------------------------------------------------------------------------------------

def _disjoint(P, B, F, C, seed):
    """the "disjoint" construction of test_owner_exclusive_rows_backward: every 16384-lookup segment (one feature)
    draws from its own slice of the rows; lookup 7 is ignored and its id still counts for the range"""
    g = torch.Generator().manual_seed(seed)
    per = C // F
    base = torch.arange(F).repeat_interleave(B) * per
    slots = ((torch.rand(P, B * F, generator=g) ** 3 * per).long().clamp_(0, per - 1) + base).contiguous()
    slots[:, 7] = -1
    ids = slots.clone()
    ids[:, 7] = 3
    return slots, ids, g


def _sgd_bound(ref, cnt):
    return 1e-5 * ref.abs() + 2e-6 + 3e-7 * cnt.sqrt()               # test_owner_exclusive_rows_backward's


def test_flagged_keys_fused_sgd_and_forward():
    """(a) fused SGD from flagged keys against fp64 index_add_, and a second launch from the same rows and keys: a row
    whose only run is flagged is one lane group's plain read-modify-write, so its bits do not move from run to run.
    (c) the same keys, built for the identity layout, through the key-driven forward: every output row is its cache row
    bit for bit -- the flag is no part of the output row."""
    import cachedembedding_amd as ce
    from cachedembedding_amd.functional import presort_window
    P, B, F, C, D, lr = 2, 16384, 3, 60000, 8, 0.5
    n = B * F
    slots, ids, g = _disjoint(P, B, F, C, 3)
    offs = torch.arange(n + 1, dtype=torch.int32).cuda()
    keys = presort_window(slots.cuda(), C, offsets=offs, include_last_offset=True, hook_features=F, ids=ids.cuda(),
                          identity_bags=True)
    flags = _check_src(keys, slots.numpy(), C, n, "src_excl", None, True, n, F, ids.numpy())
    assert flags > 1000, "the model must see owner-exclusive runs here"
    w0 = torch.randn(C, D, generator=g)
    for b in range(P):
        r = keys[b].ranges.cpu()
        assert bool((r[:-1, 1] < r[1:, 0]).all()), "the segments' id ranges must be disjoint for the plain stores"
        go = torch.randn(B, F, D, generator=g) * 0.1
        sb = slots[b].cuda()
        res = []
        for _ in range(2):
            w = w0.clone().cuda().requires_grad_(True)
            out = ce.embedding_bag(sb, w, offs, mode="sum", include_last_offset=True, sparse=True, hook_features=F,
                                   fused_sgd=ce.FusedSGD(lr), presorted=keys[b])
            # (c): forward from the keys (identity layout): out[b, f] = W[slot of lookup f * B + b], zero when ignored
            want = torch.where((slots[b] >= 0).unsqueeze(1), w0[slots[b].clamp(min=0)], torch.zeros(1, D))
            assert torch.equal(out.detach().cpu().view(torch.int32),
                               want.view(F, B, D).transpose(0, 1).contiguous().view(torch.int32))
            out.backward(go.cuda())
            res.append(w.detach().cpu())
        ok = slots[b] >= 0
        gflat = go.transpose(0, 1).reshape(-1, D)
        ref = w0.double().index_add_(0, slots[b][ok], gflat[ok].double(), alpha=-lr)
        cnt = torch.bincount(slots[b][ok], minlength=C).double().unsqueeze(1)
        assert bool(((res[0].double() - ref).abs() <= _sgd_bound(ref, cnt)).all())
        k = keys[b].keys.cpu().numpy().view(np.uint64)
        owned = np.unique((k[((k & pr.FLAG) != 0) & (k != pr.ALL_ONES)] >> np.uint64(32)).astype(np.int64))
        assert owned.size > 500
        assert torch.equal(res[0][owned].view(torch.int32), res[1][owned].view(torch.int32))
        assert not torch.equal(res[0][owned], w0[owned])


def test_flagged_keys_with_more_than_64_segments():
    """(b) 65 segments with disjoint id ranges: the backward checks at most 64 ranges against each other and must fall
    back to atomics for a longer batch; the result is the fp64 one within the same bound"""
    import cachedembedding_amd as ce
    from cachedembedding_amd.functional import presort_window
    S, C, D, lr = 65, 70000, 4, 0.5
    n = S * SEG
    slots, ids, g = _disjoint(1, SEG, S, C, 4)
    offs = torch.arange(n + 1, dtype=torch.int32).cuda()
    keys = presort_window(slots.cuda(), C, offsets=offs, include_last_offset=True, ids=ids.cuda())
    assert _check_src(keys, slots.numpy(), C, n, "src_excl", np.arange(n + 1), True, n, 0, ids.numpy()) > 1000
    r = keys[0].ranges.cpu()
    assert r.shape == (S, 2) and bool((r[:-1, 1] < r[1:, 0]).all())
    w0 = torch.randn(C, D, generator=g)
    go = torch.randn(n, D, generator=g) * 0.1
    w = w0.clone().cuda().requires_grad_(True)
    ce.embedding_bag(slots[0].cuda(), w, offs, mode="sum", include_last_offset=True, sparse=True,
                     fused_sgd=ce.FusedSGD(lr), presorted=keys[0]).backward(go.cuda())
    ok = slots[0] >= 0
    ref = w0.double().index_add_(0, slots[0][ok], go[ok].double(), alpha=-lr)
    cnt = torch.bincount(slots[0][ok], minlength=C).double().unsqueeze(1)
    assert bool(((w.detach().cpu().double() - ref).abs() <= _sgd_bound(ref, cnt)).all())


# ---- lookups that no bag covers -------------------------------------------------------------------------------------------

UNCOVERED = {"first_offset_3": (3, 0, True), "first_offset_3_last0": (3, 0, False), "last_offset_nnz_minus_2": (0, 2, True)}
_cases = {}


def _uncovered_case(layout, D):
    """1000 lookups over 300 rows; the lookups in front of offsets[0] / behind the last bag's end name rows 292.. that
    nothing else looks up.  The fp64 reference comes from lookup_plan alone and is shared by the tests below."""
    if (layout, D) in _cases:
        return _cases[layout, D]
    lo, cut, last = UNCOVERED[layout]
    rng = np.random.default_rng([len(layout), D])
    nnz, Rw = 1000, 300
    lens = rng.integers(0, 5, 2 * nnz)
    lens = lens[:np.searchsorted(np.cumsum(lens), nnz - lo - cut) + 1]
    lens[-1] -= lens.sum() - (nnz - lo - cut)
    off = lo + np.concatenate([[0], np.cumsum(lens)])
    nb = len(lens)
    ids = (rng.random(nnz) ** 2 * (Rw - 8)).astype(np.int64)
    out = np.r_[0:lo, nnz - cut:nnz]
    ids[out] = Rw - 8 + np.arange(out.size)
    offsets = off if last else off[:-1]
    plan = pr.lookup_plan(ids, Rw, offsets, last, nb, 0)
    assert np.array_equal(np.nonzero(plan.bag < 0)[0], out) and (np.diff(off) == 0).sum() > 20
    W0 = rng.standard_normal((Rw, D)).astype(np.float32)
    go = rng.standard_normal((nb, D)).astype(np.float32)
    keep = plan.bag >= 0
    blen = np.diff(off)[plan.bag[keep]]
    ref = {}
    for mode in ("sum", "mean"):
        s = np.where(blen > 1, 1.0 / blen, 1.0) if mode == "mean" else np.ones(blen.size)
        fwd = np.zeros((nb, D))
        np.add.at(fwd, plan.bag[keep], s[:, None] * W0[plan.row[keep]].astype(np.float64))
        grads = s[:, None] * go[plan.out_row[keep]].astype(np.float64)
        G = np.zeros((Rw, D))
        np.add.at(G, plan.row[keep], grads)
        ref[mode] = (fwd, G, grads)
    for a in (W0, go):
        a.setflags(write=False)
    _cases[layout, D] = dict(ids=ids, offsets=offsets, last=last, nb=nb, out=out, alone=ids[out], W0=W0, go=go,
                             rows=plan.row[keep], ref=ref, R=Rw)
    return _cases[layout, D]


def _keys_for(c, presorted):
    from cachedembedding_amd.functional import presort_slots, presort_window
    idx = _dev(c["ids"])
    if presorted == "none":
        return None
    if presorted == "slots":
        return presort_slots(idx, c["R"])
    return presort_window(idx.view(1, -1), c["R"], offsets=_dev(c["offsets"]), include_last_offset=c["last"])[0]


def _run_uncovered(c, mode, presorted, fused):
    """forward + backward of one call; returns (weight tensor afterwards, its .grad); the forward is checked here"""
    import cachedembedding_amd as ce
    w = torch.from_numpy(c["W0"].copy()).cuda().requires_grad_(True)
    out = ce.embedding_bag(_dev(c["ids"]), w, _dev(c["offsets"]), mode=mode, include_last_offset=c["last"],
                           fused_sgd=fused, presorted=_keys_for(c, presorted))
    np.testing.assert_allclose(out.detach().cpu().numpy(), c["ref"][mode][0], rtol=1e-5, atol=1e-6)
    out.backward(torch.from_numpy(c["go"].copy()).cuda())
    torch.cuda.synchronize()
    return w.detach().cpu().numpy(), None if w.grad is None else w.grad.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


FORMS = [("sum", "none"), ("sum", "slots"), ("sum", "src"), ("mean", "none"), ("mean", "slots")]


@pytest.mark.parametrize("mode,presorted", FORMS)
@pytest.mark.parametrize("D", [8, 6])
@pytest.mark.parametrize("layout", list(UNCOVERED))
def test_uncovered_lookups_dense_gradient_and_fused_sgd(layout, D, mode, presorted):
    """a lookup in front of offsets[0], or behind the end of the last bag, took no part in the forward and takes none in
    the backward: its row gets an all-zero gradient / keeps its bits; every other row is the fp64 result without those
    lookups, within the tolerance of test_source_row_keys_backward_matches_tile_backward (1e-5, 1e-5)"""
    import cachedembedding_amd as ce
    c = _uncovered_case(layout, D)
    G = c["ref"][mode][1]
    _, grad = _run_uncovered(c, mode, presorted, None)
    assert not grad[c["alone"]].any(), grad[c["alone"]]
    np.testing.assert_allclose(grad, G, rtol=1e-5, atol=1e-5)
    lr = 0.5
    w, grad = _run_uncovered(c, mode, presorted, ce.FusedSGD(lr))
    assert grad is None
    assert np.array_equal(_bits(w[c["alone"]]), _bits(c["W0"][c["alone"]]))
    np.testing.assert_allclose(w, c["W0"].astype(np.float64) - lr * G, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("accumulator", ["cache", "step"])
@pytest.mark.parametrize("mode,presorted", FORMS)
@pytest.mark.parametrize("D", [8, 6])
@pytest.mark.parametrize("layout", list(UNCOVERED))
def test_uncovered_lookups_rowwise_adagrad(layout, D, mode, presorted, accumulator):
    """the same for the fused row-wise Adagrad with either accumulator, against the fp64 step over the covered lookups
    with the bounds of test_gpu_rowwise_adagrad.py; the rows only uncovered lookups name keep weight and momentum"""
    from cachedembedding_amd.functional import FusedRowwiseAdagrad
    from test_gpu_rowwise_adagrad import _Track
    c = _uncovered_case(layout, D)
    lr = 0.05
    mom = torch.zeros(c["R"], device="cuda")
    w, grad = _run_uncovered(c, mode, presorted, FusedRowwiseAdagrad(lr, momentum=mom, accumulator=accumulator))
    assert grad is None
    track = _Track(c["W0"], c["R"], lr)
    track.step(c["rows"], c["ref"][mode][2])
    M = mom.cpu().numpy()
    assert np.array_equal(_bits(w[c["alone"]]), _bits(c["W0"][c["alone"]])) and not M[c["alone"]].any()
    assert not track.touched[c["alone"]].any() and track.touched.sum() > 100
    track.check(w, M)
    untouched = ~track.touched
    assert np.array_equal(_bits(w[untouched]), _bits(c["W0"][untouched])) and not M[untouched].any()
