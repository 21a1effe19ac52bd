"""LRU eviction (EvictionStrategy.LRU / CE_EVICT_LRU) on the GPU against the reference model of tests/lru_ref.py: after
EVERY call slots, cached_idx_map, inverted_cached_idx and the cache rows are compared exactly, as
tests/test_gpu_cache.py::test_seeded_streams_vs_oracle does it for the other strategies; at the end the hit, miss and
write-back histories, the totals and the flushed host table.  Between calls the touched cache rows are scaled (a
stand-in for a training step), so that write-backs carry fresh payloads."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from lru_ref import LruOracleCachedParamMgr  # noqa: E402
from oracle.cache_oracle import id_freq_map, power_law_ids  # noqa: E402

pytestmark = pytest.mark.gpu


def _ce():
    import cachedembedding_amd as ce
    return ce


def _pair(w, C, freq=None, warm=0.0, failed_call_is_use=True, depth=0, **kw):
    """(manager, model) over copies of the table `w`, preloaded alike"""
    ce = _ce()
    mgr = ce.CachedParamMgr(torch.from_numpy(w.copy()), C, evict_strategy=ce.EvictionStrategy.LRU, **kw)
    assert mgr.freq_cnter is None
    mgr.reorder(freq, warm)
    ora = LruOracleCachedParamMgr(w.copy(), C, failed_call_is_use=failed_call_is_use)
    ora.reorder(freq, warm)
    if depth:
        mgr.set_protect_depth(depth)
        ora.protect_depth = depth
    assert np.array_equal(mgr.idx_map.cpu().numpy().astype(np.int64), ora.idx_map)          # the identity
    _state_equal(mgr, ora)
    return mgr, ora


def _state_equal(mgr, ora):
    assert np.array_equal(mgr.cached_idx_map.cpu().numpy().astype(np.int64), ora.cached_idx_map)
    assert np.array_equal(mgr.inverted_cached_idx.cpu().numpy().astype(np.int64), ora.inverted_cached_idx)
    np.testing.assert_array_equal(mgr.cuda_cached_weight.detach().cpu().numpy(), ora.cuda_cached_weight)


def _after_call(mgr, ora, slots, eslots):
    """slots equal; a step on the touched rows; state equal"""
    slots_np = slots.cpu().numpy()
    assert np.array_equal(slots_np.reshape(-1), np.asarray(eslots).reshape(-1))
    used = np.unique(slots_np[slots_np >= 0])
    ora.cuda_cached_weight[used] *= np.float32(1.25)
    with torch.no_grad():
        mgr.cuda_cached_weight[torch.from_numpy(used).cuda()] *= 1.25
    _state_equal(mgr, ora)


def _call(mgr, ora, ids):
    eslots = ora.prepare_ids(ids)
    slots = mgr.prepare_ids(torch.from_numpy(ids).cuda())
    _after_call(mgr, ora, slots, eslots)


def _finish(mgr, ora, failed_at=()):
    """histories (a failed call leaves a record in the manager's, none in the model's), totals, flushed table"""
    mgr.sync_stats()
    keep = [i for i in range(len(mgr.num_hits_history)) if i not in failed_at]
    assert [mgr.num_hits_history[i] for i in keep] == ora.num_hits_history
    assert [mgr.num_miss_history[i] for i in keep] == ora.num_miss_history
    assert [mgr.num_write_back_history[i] for i in keep] == ora.num_write_back_history
    t = mgr.totals()
    assert t["cache_miss"] == ora.cache_miss and t["total_cache"] == ora.total_cache
    assert t["cpu_to_cuda_numel"] == ora.cpu_to_cuda_numel and t["cuda_to_cpu_numel"] == ora.cuda_to_cpu_numel
    mgr.flush()
    ora.flush()
    np.testing.assert_array_equal(mgr.weight.numpy(), ora.weight)
    assert (mgr.cached_idx_map == -1).all() and (mgr.inverted_cached_idx == -1).all()


def _draw(rng, perm, N, C, n_ids, s):
    ids = perm[power_law_ids(rng, N, n_ids, s)]
    if len(np.unique(ids)) > C:
        ids = ids[:C // 2]
    return ids


def _table(rng, N, D, s):
    w = rng.standard_normal((N, D)).astype(np.float32)
    perm = rng.permutation(N)
    freq = id_freq_map(perm[power_law_ids(rng, N, 200000, s)], N)
    return w, perm, freq


# ------------------------------------------------------------------------------------------------ 1
def test_hand_checked_script():
    """N = 6, C = 3, no preload.  The second [3] evicts row 1, not row 0: of two slots with the same last use the higher
    one goes first."""
    ce = _ce()
    script = [[0, 1, 2], [3], [0, 1], [2], [3], [0], [1]]
    w = torch.arange(24, dtype=torch.float32).view(6, 4)
    bag = ce.CachedEmbeddingBag(6, 4, _weight=w.clone(), mode="sum", cuda_row_num=3, warmup_ratio=0.0,
                                evict_strategy=ce.EvictionStrategy.LRU)
    ora = LruOracleCachedParamMgr(w.numpy().copy(), 3)
    mgr = bag.cache_weight_mgr
    evicted = []
    for ids in script:
        before = mgr.cached_idx_map.cpu().numpy()
        out = bag(torch.tensor(ids, device="cuda"), torch.tensor([0], device="cuda"))
        torch.testing.assert_close(out.cpu(), w[ids].sum(0, keepdim=True), rtol=0, atol=0)
        after = mgr.cached_idx_map.cpu().numpy()
        evicted.append(sorted(set(before[before >= 0].tolist()) - set(after[after >= 0].tolist())))
        ora.prepare_ids(np.array(ids))
        _state_equal(mgr, ora)
    assert bag.num_hits_history == [0, 0, 2, 0, 0, 1, 0] == ora.num_hits_history
    assert evicted == [[], [2], [], [3], [1], [], [2]]


# ------------------------------------------------------------------------------------------------ 2
SHAPES = [(50000, 512, 32, 400, 0.25),
          (3000, 3000, 16, 2500, 0.5),            # the cache is as large as the table
          (70001, 4097, 100, 4096, 1.05)]         # odd sizes, rows that are no whole 16-byte vectors


@pytest.mark.parametrize("preload", [True, False])
@pytest.mark.parametrize("N,C,D,n_ids,s", SHAPES)
def test_seeded_streams(N, C, D, n_ids, s, preload):
    rng = np.random.default_rng(N + C)
    w, perm, freq = _table(rng, N, D, s)
    mgr, ora = _pair(w, C, freq if preload else None, 0.7 if preload else 0.0)
    for _ in range(12):
        _call(mgr, ora, _draw(rng, perm, N, C, n_ids, s))
    _finish(mgr, ora)


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("N,C,n_ids,calls", [(64, 8, 3, 300),            # 3 slot bits + 8 bits of call 255 = 11: one
                                             (20000, 4097, 64, 600)])    # radix digit; 13 + 9 = 22 at call 511: two
def test_key_width_crosses_a_radix_digit_while_the_stream_runs(N, C, n_ids, calls):
    """The key is (last use << slot_bits) | (slot counted down) and the select looks at bits(call number) + slot_bits
    of it, in 11-bit digits: the pass count goes from 1 to 2 at call 256 of the small cache and from 2 to 3 at call 512
    of the large one (no preload: the first prepare_ids is call 1).  Uniform ids keep every call evicting."""
    rng = np.random.default_rng(N + C)
    w = rng.standard_normal((N, 4)).astype(np.float32)
    mgr, ora = _pair(w, C)
    for _ in range(calls):
        _call(mgr, ora, rng.integers(0, N, n_ids))
    assert sum(ora.num_write_back_history[-50:]) > 0
    _finish(mgr, ora)


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("N,C,D,n_ids,s", [(20000, 2000, 8, 300, 1.05),
                                           (20000, 400, 8, 300, 0.25)])    # a cache small enough to evict at every call
def test_protect_depth(depth, N, C, D, n_ids, s):
    rng = np.random.default_rng(N + C + depth)
    w, perm, freq = _table(rng, N, D, s)
    mgr, ora = _pair(w, C, freq, 0.7, depth=depth)
    for _ in range(30):
        _call(mgr, ora, _draw(rng, perm, N, C, n_ids, s))
    _finish(mgr, ora)


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("async_copy,buffer_size", [(False, 0), (True, 0), (True, 3)])
def test_transports(async_copy, buffer_size):
    N, C, D, n_ids, s = 50000, 512, 32, 400, 0.25
    rng = np.random.default_rng(N + C)
    w, perm, freq = _table(rng, N, D, s)
    mgr, ora = _pair(w, C, freq, 0.7, async_copy=async_copy, buffer_size=buffer_size)
    for _ in range(12):
        _call(mgr, ora, _draw(rng, perm, N, C, n_ids, s))
    _finish(mgr, ora)


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("halves", [False, True])
def test_window_entries(halves):
    """a window of 4 batches is ONE call: all its rows share one recency (in one piece, and in the _begin / _finish
    halves with protect_depth 1)"""
    from cachedembedding_amd.functional import presort_len
    N, C, D, P, n, s = 20000, 1500, 8, 4, 256, 0.25          # (~350 unique rows per window: it evicts from the 5th on)
    rng = np.random.default_rng(N + C)
    w, perm, freq = _table(rng, N, D, s)
    mgr, ora = _pair(w, C, freq, 0.7, depth=1 if halves else 0)
    out = torch.empty(P, n, dtype=torch.int64, device="cuda")
    keys = torch.empty(P, presort_len(n), dtype=torch.int64, device="cuda")
    for _ in range(10):
        ids = perm[power_law_ids(rng, N, P * n, s)].reshape(P, n)
        eslots = ora.prepare_ids(ids.reshape(-1))
        t = torch.from_numpy(ids).cuda()
        if halves:
            mgr.prepare_ids_begin(t, out)
            mgr.prepare_ids_finish()
        else:
            mgr.prepare_ids_keys(t, out, keys)
        _after_call(mgr, ora, out, eslots)
    _finish(mgr, ora)


def test_padded_entry():
    """-1 on the padded entry names nothing: no slot, no use"""
    N, C, D, n_ids, s = 20000, 600, 8, 500, 0.25
    rng = np.random.default_rng(N + C)
    w, perm, freq = _table(rng, N, D, s)
    mgr, ora = _pair(w, C, freq, 0.7)
    for it in range(10):
        ids = _draw(rng, perm, N, C, n_ids, s)
        ids = np.where(rng.random(len(ids)) < 0.3, -1, ids)
        if it == 5:
            ids[:] = -1                                     # nothing but padding: still a call
        eslots = ora.prepare_ids_padded(ids)
        slots = mgr.prepare_ids(torch.from_numpy(ids).cuda(), padded=True)
        assert (slots.cpu().numpy()[ids == -1] == -1).all()
        _after_call(mgr, ora, slots, eslots)
    _finish(mgr, ora)


# ------------------------------------------------------------------------------------------------ 7
def test_captured_cache_op():
    """One cache op captured into a hipGraph (zero-copy transport, one stream; the call number is counted on the
    device, the select is sized for the whole 30-bit stamp) and replayed 20 times with changing ids in the static
    buffer, between eager calls before and after.  Captured calls take the bitmap front: the model's failed-call flag
    is off."""
    N, C, D, n_ids, s = 50000, 512, 32, 400, 0.25
    rng = np.random.default_rng(N + C + 7)
    w, perm, freq = _table(rng, N, D, s)
    mgr, ora = _pair(w, C, freq, 0.7, failed_call_is_use=False)
    for _ in range(3):
        _call(mgr, ora, _draw(rng, perm, N, C, n_ids, s))
    static_ids = torch.zeros(n_ids, dtype=torch.int64, device="cuda")
    static_slots = torch.empty(n_ids, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mgr.prepare_ids(static_ids, out=static_slots)
    for _ in range(20):
        ids = perm[power_law_ids(rng, N, n_ids, s)]
        assert len(np.unique(ids)) <= C
        eslots = ora.prepare_ids(ids)
        static_ids.copy_(torch.from_numpy(ids))
        g.replay()
        mgr.graph_replayed(1, n_ids)
        torch.cuda.synchronize()
        _after_call(mgr, ora, static_slots, eslots)
    for _ in range(3):
        _call(mgr, ora, _draw(rng, perm, N, C, n_ids, s))
    _finish(mgr, ora)


# ------------------------------------------------------------------------------------------------ 8
def test_failed_calls_on_the_default_front():
    """A bad-id call and an overflowing call in the middle of a stream: state untouched, and -- the per-lookup front
    keeps the stamps a failed call wrote -- the calls after them equal the model in which a failed call is a use of the
    resident rows it named."""
    N, C, D, n_ids, s = 50000, 512, 32, 400, 0.25
    rng = np.random.default_rng(N + C + 8)
    w, perm, freq = _table(rng, N, D, s)
    mgr, ora = _pair(w, C, freq, 0.7, failed_call_is_use=True)
    failed_at = []
    for c in range(14):
        if c in (5, 9):
            resident = ora.cached_idx_map[ora.cached_idx_map >= 0]
            if c == 5:          # names the 200 resident rows in the highest slots (the next to go), then a bad id
                ids, err = np.concatenate([resident[-200:], [N]]), IndexError
            else:               # more unique rows than slots, 300 of them resident
                absent = perm[ora.inverted_cached_idx[perm] < 0]
                ids, err = np.concatenate([resident[:300], absent[:C + 1 - 300]]), AssertionError
                assert len(np.unique(ids)) == C + 1
            before = (mgr.cached_idx_map.clone(), mgr.inverted_cached_idx.clone(), mgr.cuda_cached_weight.detach().clone())
            with pytest.raises(err):
                ora.prepare_ids(ids)
            with pytest.raises(err):
                mgr.prepare_ids(torch.from_numpy(ids).cuda())
            assert torch.equal(before[0], mgr.cached_idx_map) and torch.equal(before[1], mgr.inverted_cached_idx)
            assert torch.equal(before[2], mgr.cuda_cached_weight.detach())
            failed_at.append(c)
            continue
        _call(mgr, ora, _draw(rng, perm, N, C, n_ids, s))
    _finish(mgr, ora, failed_at)


# ------------------------------------------------------------------------------------------------ 9
def test_module_trains_like_a_plain_embedding_bag():
    """CachedEmbeddingBag(evict_strategy=LRU) with the fused SGD against torch.nn.EmbeddingBag + SGD on the CPU, same
    ids and gradients, host table after flush.  The tolerance is the one
    tests/test_gpu_modules.py::test_flush_save_reload_continue_training_round_trip uses for the same comparison (a
    cached module with fused SGD against a plain EmbeddingBag with SGD) under DATASET and LFU.  It is a tolerance for
    table rows; the pooled outputs on the way are not compared with it: a bag's sum can cancel (0.045 out of rows of
    magnitude 1 here), and a relative bound on such a sum does not follow from one on the rows (measured: rows within
    the tolerance, one output element of 2400 off by 1.5e-6 = 12 ulp of a row element).  The forward itself is
    compared exactly in test_hand_checked_script."""
    ce = _ce()
    N, D, C, lr, steps, n_ids, bags = 2000, 16, 200, 0.1, 20, 300, 150
    g = torch.Generator().manual_seed(9)
    rng = np.random.default_rng(9)
    w0 = torch.randn(N, D, generator=g)
    perm = rng.permutation(N)
    emb = ce.CachedEmbeddingBag(N, D, sparse=True, _weight=w0.clone(), mode="sum", include_last_offset=True,
                                cuda_row_num=C, warmup_ratio=0.7, evict_strategy=ce.EvictionStrategy.LRU)
    emb.set_fused_sgd(lr)
    ref = torch.nn.EmbeddingBag.from_pretrained(w0.clone(), freeze=False, mode="sum", include_last_offset=True)
    opt = torch.optim.SGD(ref.parameters(), lr=lr)
    off = torch.arange(0, n_ids + 1, n_ids // bags)
    for _ in range(steps):
        ids = torch.from_numpy(perm[power_law_ids(rng, N, n_ids, 0.6)])
        assert len(torch.unique(ids)) <= C
        go = torch.randn(bags, D, generator=g)
        out = emb(ids.cuda(), off.cuda())
        out.backward(go.cuda())
        o = ref(ids, off)
        opt.zero_grad()
        o.backward(go)
        opt.step()
    assert sum(emb.cache_weight_mgr.num_write_back_history) > 0
    emb.flush()
    torch.testing.assert_close(emb.weight, ref.weight.detach(), rtol=1e-5, atol=1e-6)
