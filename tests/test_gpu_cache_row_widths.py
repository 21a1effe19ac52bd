"""The cache op's row movers at the widths the in-row layouts produce (tests/cache_row_width_cases.py): 3 * D floats of an
Adam-layout row, 2 * D of partial row-wise Adam, a q8 / q4 row, a 16-bit row, and the scalar width 66.  A row wider than
64 lanes' worth (64 16-byte vectors, or 64 floats of a row that is no multiple of 16 bytes) leaves the movers' register
path for their copy_row loop; these tests run both bodies of every mover on every transport against the CPU oracle.

A row mover copies bits: slots, maps, counters, the whole cache and the write-back history are compared for equality
after every call, the host table row for row after the flush.  No tolerance appears anywhere.  The last section trains
Adam-layout modules through a cache that evicts at every step and compares them, bit for bit, with modules whose cache
holds the whole table."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import cache_row_width_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

ARRANGEMENTS = ["zerocopy", "staged", "worker_kernel", "worker_sdma"]


def _ce():
    import cachedembedding_amd as ce
    return ce


def _strat(ce, s):
    return {"dataset": ce.EvictionStrategy.DATASET, "lfu": ce.EvictionStrategy.LFU, "lru": ce.EvictionStrategy.LRU}[s]


def _rows_equal(got, want, what):
    """bit for bit (-0.0 is not 0.0 here); numpy's own report only once they differ -- it costs twenty times the compare"""
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        np.testing.assert_array_equal(got, want, err_msg=what)
        raise AssertionError(f"{what}: equal as numbers, not as bits")


def _state_equal(mgr, ora, lfu):
    assert np.array_equal(mgr.cached_idx_map.cpu().numpy().astype(np.int64), ora.cached_idx_map)
    assert np.array_equal(mgr.inverted_cached_idx.cpu().numpy().astype(np.int64), ora.inverted_cached_idx)
    if lfu:
        assert np.array_equal(mgr.freq_cnter.cpu().numpy(), ora.freq_cnter)
    _rows_equal(mgr.cuda_cached_weight.detach().cpu().numpy(), ora.cuda_cached_weight, "cuda_cached_weight")


def _pair(stream, transport="zerocopy", admit=None, monkeypatch=None):
    """(manager, oracle) over copies of the stream's table, warmed up alike, on `transport`"""
    ce = _ce()
    if admit is not None:
        monkeypatch.setenv("CE_WORKER_ADMIT", admit)          # read when the manager's swap engine is created
    w = stream.table()
    ora = stream.oracle(w.copy())
    mgr = ce.CachedParamMgr(torch.from_numpy(w.copy()), stream.C, evict_strategy=_strat(ce, stream.strategy),
                            async_copy=transport == "staged")
    assert mgr._lib_dim == stream.width and tuple(mgr.cuda_cached_weight.shape) == (stream.C, stream.width)
    mgr.reorder(None, stream.warm)
    if transport == "worker":
        mgr.set_transport("worker")
    if stream.depth:
        mgr.set_protect_depth(stream.depth)
    _state_equal(mgr, ora, stream.strategy == "lfu")
    return mgr, ora


def _step(mgr, ora, slots, want, c, lfu):
    """the slots agree; a training step on the touched rows (every write-back then carries a payload the host table has
    never held); the state agrees"""
    assert np.array_equal(slots.reshape(-1).cpu().numpy(), want)
    ora.cuda_cached_weight[np.unique(want)] += cases.Stream.bump(c)
    with torch.no_grad():
        mgr.cuda_cached_weight[torch.unique(slots)] += float(cases.Stream.bump(c))
    _state_equal(mgr, ora, lfu)


def _finish(mgr, ora, transport):
    assert mgr.transport_name == transport          # (no fall-back to the zero-copy kernels)
    assert mgr.num_write_back_history == ora.num_write_back_history
    mgr.flush()
    ora.flush()
    _rows_equal(mgr.weight.numpy(), ora.weight, "the host table after the flush")
    assert (mgr.cached_idx_map == -1).all() and (mgr.inverted_cached_idx == -1).all()


# ---- every arrangement, every width ------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", list(cases.WIDTHS))
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
def test_every_arrangement_at_every_width(arrangement, width, monkeypatch):
    """test_every_arrangement_in_two_halves_and_with_the_keys_tail (tests/test_gpu_worker.py) at the widths of the
    in-row layouts: the call in two halves (padded, without and with keys) and the whole call with the keys tail take
    turns on the zero-copy, staged and worker transports (chained and host-gather admission); the strategy changes with
    the width."""
    from cachedembedding_amd.functional import presort_len, presort_window
    s = cases.halves_stream(width)
    transport = arrangement.split("_")[0]
    admit = {"worker_kernel": "kernel", "worker_sdma": "sdma"}.get(arrangement)
    mgr, ora = _pair(s, transport, admit, monkeypatch)
    lfu = s.strategy == "lfu"
    per_call = 100
    klen = presort_len(per_call)
    evicted = 0
    for c, ids in s.calls(ora):
        want = ora.prepare_ids(ids)
        dev = torch.from_numpy(ids).cuda()
        slots = torch.empty(1, per_call, dtype=torch.int64, device="cuda")
        keys = torch.empty(1, klen, dtype=torch.int64, device="cuda")
        form = (c + 3) % 4
        if form == 0:
            mgr.prepare_ids_begin_padded(dev, slots.view(-1))
            mgr.prepare_ids_finish()
        elif form == 1:
            mgr.prepare_ids_begin(dev.view(1, -1), slots)
            mgr.prepare_ids_finish()
        elif form == 2:
            mgr.prepare_ids_begin(dev.view(1, -1), slots, keys)
            mgr.prepare_ids_finish()
        else:
            mgr.prepare_ids_keys(dev.view(1, -1), slots, keys)
        if form >= 2:       # (the order inside a 16384-lookup segment depends on an atomic race in either form)
            ref = presort_window(slots.contiguous(), s.C)
            assert torch.equal(keys.view(1, -1, 16384).sort(dim=2).values, ref.view(1, -1, 16384).sort(dim=2).values)
        evicted += len(ora.traces[-1].evicted_rows)
        _step(mgr, ora, slots, want, c, lfu)
    assert evicted > 2 * s.C, "the stream did not go round the cache twice"
    _finish(mgr, ora, transport)


# ---- re-admission while the write-back is in flight ----------------------------------------------------------------------

@pytest.mark.parametrize("admit", ["kernel", "sdma"])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("width", [66, 260, 384, 3072])
def test_readmission_of_wide_rows_still_in_flight(width, depth, admit, monkeypatch):
    """test_readmission_of_rows_still_in_flight (tests/test_gpu_worker.py) at loop-body widths: every call asks again
    for half of the rows the previous call evicted, whose only up-to-date copy is the previous call's staging block while
    the worker copies it out.  Whether such a row is read from that block or from the host table depends on timing; both
    must give the oracle's bits."""
    s = cases.readmit_stream(width, depth)
    mgr, ora = _pair(s, "worker", admit, monkeypatch)
    lfu = s.strategy == "lfu"
    prev_evicted = np.zeros(0, dtype=np.int64)
    readmitted = 0
    for c, ids in s.calls(ora):
        want = ora.prepare_ids(ids)
        slots = mgr.prepare_ids(torch.from_numpy(ids).cuda())
        readmitted += int(np.isin(ora.traces[-1].miss_rows, prev_evicted).sum())
        prev_evicted = ora.traces[-1].evicted_rows.copy()
        _step(mgr, ora, slots, want, c, lfu)
        if c in (7, 15):
            _rows_equal(mgr.weight.numpy(), ora.weight, f"the host table after call {c}")   # (.weight waits for the worker)
    assert readmitted > 50, "the stream did not exercise the pending-row path"
    _finish(mgr, ora, "worker")
    assert mgr.writeback_stats()["rows"] == sum(ora.num_write_back_history)


# ---- the 16-rows-in-flight vector swap ----------------------------------------------------------------------------------

def test_big_call_takes_the_wide_swap_at_a_wide_row():
    """a call of more than 131072 lookups: the zero-copy swap runs 16 rows in flight per lane group, not the 4 every
    small call gets; 96 vectors per row"""
    s = cases.big_call_stream()
    mgr, ora = _pair(s)
    for c, ids in s.calls(ora):
        assert len(ids) > 131072
        want = ora.prepare_ids(ids)
        slots = mgr.prepare_ids(torch.from_numpy(ids).cuda())
        assert c == 0 or len(ora.traces[-1].evicted_rows) > 0
        _step(mgr, ora, slots, want, c, s.strategy == "lfu")
    _finish(mgr, ora, "zerocopy")


# ---- preload and flush ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("transport", ["zerocopy", "worker"])
@pytest.mark.parametrize("width", [260, 384, 3072, 66])
def test_preload_and_flush_at_wide_rows(width, transport):
    """a 70 % preload (ce_cache_preload), 10 evicting calls, the flush of a full cache"""
    s = cases.warm_stream(width)
    mgr, ora = _pair(s, transport)
    assert int((mgr.cached_idx_map >= 0).sum()) == 140          # the preload placed its rows (compared in _pair)
    for c, ids in s.calls(ora):
        want = ora.prepare_ids(ids)
        slots = mgr.prepare_ids(torch.from_numpy(ids).cuda())
        _step(mgr, ora, slots, want, c, s.strategy == "lfu")
    assert sum(ora.num_write_back_history) > 0
    assert int((mgr.cached_idx_map >= 0).sum()) == s.C          # the flush below moves a full cache
    _finish(mgr, ora, transport)


# ---- transport switches at a wide row -----------------------------------------------------------------------------------

def test_transport_switches_keep_a_wide_table_consistent():
    """zerocopy -> worker -> staged -> worker -> zerocopy in the middle of a stream, 384 floats per row"""
    ce = _ce()
    from oracle.cache_oracle import DATASET, OracleCachedParamMgr
    rng = np.random.default_rng(5)
    N, C, D = 5000, 400, 384
    w = rng.standard_normal((N, D)).astype(np.float32)
    ora = OracleCachedParamMgr(w.copy(), C, DATASET)
    ora.reorder(None, 0.7)
    mgr = ce.CachedParamMgr(torch.from_numpy(w.copy()), C)
    mgr.reorder(None, 0.7)
    order = ["zerocopy", "worker", "staged", "worker", "zerocopy"]
    for c in range(20):
        mgr.set_transport(order[(c // 4) % len(order)])
        assert mgr.transport_name == order[(c // 4) % len(order)]
        ids = rng.integers(0, N, size=250)
        eslots = ora.prepare_ids(ids)
        slots = mgr.prepare_ids(torch.from_numpy(ids).cuda())
        assert np.array_equal(slots.cpu().numpy(), eslots)
        ora.cuda_cached_weight[np.unique(eslots)] *= np.float32(1.5)
        with torch.no_grad():
            mgr.cuda_cached_weight[torch.unique(slots)] *= 1.5
        _state_equal(mgr, ora, False)
    _rows_equal(mgr.weight.numpy(), ora.weight, "the host table before the flush")
    mgr.flush()
    ora.flush()
    _rows_equal(mgr.weight.numpy(), ora.weight, "the host table after the flush")


# ---- the layouts themselves through an evicting cache ------------------------------------------------------------------

_WHOLE = {}


def _train(layout, D, strategy, cuda_row_num, transport=None):
    """8 steps of fused Adam, one id per bag, distinct ids within a step; the state after the flush, and every output"""
    ce = _ce()
    emb = ce.CachedEmbeddingBag(cases.LAYOUT_N, D, mode="sum", include_last_offset=True, cuda_row_num=cuda_row_num,
                                evict_strategy=_strat(ce, strategy), fused_optimizer=layout, init_seed=1000 + D)
    mgr = emb.cache_weight_mgr
    assert mgr._lib_dim == cases.layout_width(layout, D) == mgr.cuda_cached_weight.shape[1]
    if transport is not None:
        mgr.set_transport(transport)
        assert mgr.transport_name == transport
    emb.set_fused_adam(0.05, (0.9, 0.999), 1e-8)
    rng = np.random.default_rng([D, 6])
    off = torch.arange(cases.LAYOUT_B + 1, device="cuda")
    outs = []
    for ids in cases.layout_steps(D):
        go = rng.standard_normal((cases.LAYOUT_B, D)).astype(np.float32)
        out = emb(torch.from_numpy(ids).cuda(), off)
        outs.append(out.detach().cpu().clone())
        out.backward(torch.from_numpy(go).cuda())
    writes = list(emb.num_write_back_history)
    emb.flush()
    torch.cuda.synchronize()
    return dict(weight=emb.weight.clone(), exp_avg=emb.exp_avg.clone(), exp_avg_sq=emb.exp_avg_sq.detach().cpu().clone(),
                step=int(emb.adam_step.item()), outs=outs, writes=writes)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("transport", ["zerocopy", "worker"])
@pytest.mark.parametrize("layout,D,strategy", cases.LAYOUT_CASES)
def test_layout_state_travels_intact_through_an_evicting_cache(layout, D, strategy, transport):
    """Adam (rows w | m | v) at D = 128 and 1024, partial row-wise Adam (rows w | m) at D = 128 and 256: a module whose
    56-row cache evicts at every step against one whose cache holds all 400 rows, from one init_seed on the same steps.
    With distinct ids a row's folded gradient is a single term added to a zero accumulator, so its update is the same
    bits whatever slot it sits in: weights, both moments, the step count and every forward output must be EQUAL.  From
    the third step on at least a third of a step's rows had been evicted since an earlier step named them (counted on
    the oracle from the ids alone), so the moments compared here left for the host table and came back."""
    steps = cases.layout_steps(D)
    back = cases.revisits_of_evicted_rows(steps, strategy)
    assert all(len(np.unique(ids)) == len(ids) for ids in steps)
    assert all(3 * n >= cases.LAYOUT_B for n in back[2:]), back
    if (layout, D) not in _WHOLE:
        _WHOLE[layout, D] = _train(layout, D, strategy, cases.LAYOUT_N)
    whole = _WHOLE[layout, D]
    assert sum(whole["writes"]) == 0
    small = _train(layout, D, strategy, cases.LAYOUT_C, transport)
    assert all(n > 0 for n in small["writes"][1:]), small["writes"]              # evicts at every step after the first
    assert small["step"] == whole["step"] == cases.LAYOUT_STEPS
    for k, (a, b) in enumerate(zip(small["outs"], whole["outs"])):
        assert torch.equal(_bits(a), _bits(b)), f"forward output of step {k}"
    for name in ("weight", "exp_avg", "exp_avg_sq"):
        assert small[name].shape == whole[name].shape
        assert torch.equal(_bits(small[name]), _bits(whole[name])), name
    assert whole["exp_avg"].any() and whole["exp_avg_sq"].any()
    assert tuple(whole["exp_avg_sq"].shape) == ((cases.LAYOUT_N,) if layout == "partial_rowwise_adam" else (cases.LAYOUT_N, D))
