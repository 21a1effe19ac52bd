"""Worker transport (CE_TRANSPORT_WORKER: evictions packed in HBM, copied out with pinned hipMemcpyAsync on private
streams and scattered into the host table by a thread inside libce_hip; admissions by a small kernel on a private
stream launched by a second library thread -- or, CE_WORKER_ADMIT=sdma, gathered by host threads and copied in --
while the cache-op stream parks until they have arrived) against the CPU oracle.  Same bar as the other transports: slots, maps, counters, histories and the
cache payloads bit-exact after every call, the host table bit-exact once the write-backs have landed -- including
rows that are re-admitted in the very call after the one that evicted them (their payload must come from the
staging buffer, the host row is stale at that moment)."""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"


def _ce():
    import cachedembedding_amd as ce
    return ce


def _strat(ce, s):
    return ce.EvictionStrategy.LFU if s == "lfu" else ce.EvictionStrategy.DATASET


def _state_equal(mgr, ora, lfu):
    assert np.array_equal(mgr.cached_idx_map.cpu().numpy().astype(np.int64), ora.cached_idx_map)
    assert np.array_equal(mgr.inverted_cached_idx.cpu().numpy().astype(np.int64), ora.inverted_cached_idx)
    if lfu:
        assert np.array_equal(mgr.freq_cnter.cpu().numpy(), ora.freq_cnter)
    np.testing.assert_array_equal(mgr.cuda_cached_weight.detach().cpu().numpy(), ora.cuda_cached_weight)


@pytest.mark.parametrize("admit", ["kernel", "kernel_deferred", "sdma"])
@pytest.mark.parametrize("name,strategy", [("cache_dataset_freq", "dataset"), ("cache_dataset_nofreq", "dataset"),
                                           ("cache_lfu_freq", "lfu"), ("cache_lfu_nofreq", "lfu")])
def test_golden_streams_worker(name, strategy, admit, monkeypatch):
    """kernel: the chained admission (fused front / select kernels, admission + unpack on the admission stream);
    kernel_deferred: the same with ce_cache_set_deferred_rows -- the call's stream does not wait for its rows, the test
    does (wait_rows) before it touches the cache; sdma: host gather + staged copies behind a parked stream."""
    ce = _ce()
    deferred = admit == "kernel_deferred"
    if deferred:
        admit = "kernel"
    monkeypatch.setenv("CE_WORKER_ADMIT", admit)      # read when the manager's swap engine is created
    z = np.load(GOLD / f"{name}.npz")
    N, C, D, n_ids, calls, warm = (int(v) for v in z["meta"])
    freq = z["freq"] if z["freq"].size else None
    mgr = ce.CachedParamMgr(torch.from_numpy(z["weight"].copy()), C, evict_strategy=_strat(ce, strategy))
    mgr.reorder(freq, warm / 1000.0)
    mgr.set_transport("worker")
    if deferred:
        mgr.set_deferred_rows(True)
    for c in range(calls):
        slots = mgr.prepare_ids(torch.from_numpy(z["ids"][c]).cuda())
        if deferred:
            mgr.wait_rows()
        assert np.array_equal(slots.cpu().numpy(), z["slots"][c])
        assert np.array_equal(mgr.cached_idx_map.cpu().numpy().astype(np.int64), z["cached_idx_map"][c])
        if strategy == "lfu":
            assert np.array_equal(mgr.freq_cnter.cpu().numpy(), z["freq_cnter"][c])
        with torch.no_grad():
            mgr.cuda_cached_weight[torch.unique(slots)] += 0.5
    assert mgr.num_hits_history == z["hits"].tolist()
    assert mgr.num_miss_history == z["misses"].tolist()
    mgr.flush()
    np.testing.assert_array_equal(mgr.weight.numpy(), z["weight_after_flush"])
    assert mgr.writeback_stats()["jobs"] == calls


@pytest.mark.parametrize("admit", ["kernel", pytest.param("kernel_slow_writeback", marks=pytest.mark.test_hooks), "sdma"])
@pytest.mark.parametrize("strategy", ["dataset", "lfu"])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("N,C,D,per_call", [(6000, 700, 128, 300), (20000, 1500, 32, 500), (3001, 257, 20, 100)])
def test_readmission_of_rows_still_in_flight(strategy, depth, N, C, D, per_call, admit, monkeypatch):
    """Every call asks for half of the rows the previous call evicted (plus fresh ones): their only up-to-date copy is
    the previous call's staging buffer while the worker is still copying it out.  Cache payloads are compared after
    every call, the host table at the end and at two intermediate writeback_wait() points.
    kernel_slow_writeback: every write-back job starts 2 ms late (test hook), so the kernel admission of the next call
    runs before it has landed and must take those rows out of the staging buffer (it only waits for the job before)."""
    slow = admit == "kernel_slow_writeback"
    monkeypatch.setenv("CE_WORKER_ADMIT", "kernel" if slow else admit)
    if slow:
        monkeypatch.setenv("CE_WORKER_OUT_DELAY_US", "2000")
    ce = _ce()
    from oracle.cache_oracle import DATASET, LFU, OracleCachedParamMgr
    rng = np.random.default_rng(N * 7 + C + depth)
    w = rng.standard_normal((N, D)).astype(np.float32)
    ora = OracleCachedParamMgr(w.copy(), C, LFU if strategy == "lfu" else DATASET)
    ora.protect_depth = depth
    ora.reorder(None, 1.0)
    mgr = ce.CachedParamMgr(torch.from_numpy(w.copy()), C, evict_strategy=_strat(ce, strategy))
    mgr.reorder(None, 1.0)
    mgr.set_transport("worker")
    mgr.set_protect_depth(depth)
    lfu = strategy == "lfu"
    prev_evicted = np.zeros(0, dtype=np.int64)
    readmitted = 0
    if depth:
        per_call //= 2                # unique(call c U call c-1) must fit the cache when the previous call is protected
    for c in range(24):
        fresh = rng.integers(0, N, size=per_call)
        again = prev_evicted[rng.permutation(len(prev_evicted))[: len(prev_evicted) // 2]]
        ids = np.concatenate([fresh, again, again[: len(again) // 3]])       # some of them more than once
        rng.shuffle(ids)
        eslots = ora.prepare_ids(ids)
        slots = mgr.prepare_ids(torch.from_numpy(ids).cuda())
        assert np.array_equal(slots.cpu().numpy(), eslots)
        readmitted += int(np.isin(ora.traces[-1].miss_rows, prev_evicted).sum())
        prev_evicted = ora.traces[-1].evicted_rows.copy()                    # no frequency map: row == id
        # a training step on the touched rows: every write-back carries a payload the host table has never seen
        ora.cuda_cached_weight[np.unique(eslots)] += np.float32(0.25 * (c + 1))
        with torch.no_grad():
            mgr.cuda_cached_weight[torch.unique(slots)] += 0.25 * (c + 1)
        _state_equal(mgr, ora, lfu)
        if c in (7, 15):
            np.testing.assert_array_equal(mgr.weight.numpy(), ora.weight)   # .weight waits for the worker
    assert readmitted > 50, "the stream did not exercise the pending-row path"
    assert mgr.num_write_back_history == ora.num_write_back_history
    mgr.flush()
    ora.flush()
    np.testing.assert_array_equal(mgr.weight.numpy(), ora.weight)
    st = mgr.writeback_stats()
    assert st["rows"] == sum(ora.num_write_back_history)
    if slow:
        assert st["in_jobs_before_writeback_landed"] >= 10, st


@pytest.mark.parametrize("strategy", ["dataset", "lfu"])
@pytest.mark.parametrize("N,C,D,per_call", [(3001, 257, 20, 100), (6000, 700, 128, 300)])       # scalar rows, vector rows
@pytest.mark.parametrize("arrangement", ["zerocopy", "staged", "worker_kernel", "worker_sdma"])
def test_every_arrangement_in_two_halves_and_with_the_keys_tail(arrangement, N, C, D, per_call, strategy, monkeypatch):
    """The forms of a cache op that the streams above do not reach on every arrangement: the call in two halves
    (ce_cache_prepare_ids_begin_padded / _begin without and with keys, then _finish) and the whole call with the keys
    tail (ce_cache_prepare_ids_keys), taking turns call by call, on the zero-copy, staged and worker transports (chained
    and host-gather admission).  13 calls fill the cache (3) and go round it twice more, so both the warm-up and the
    steady form of every arrangement run.  Slots, maps, counters and cache payloads against the oracle after every
    call, the window's keys against a presort of the slots, the host table row for row after the flush."""
    ce = _ce()
    from cachedembedding_amd.functional import presort_len, presort_window
    from oracle.cache_oracle import DATASET, LFU, OracleCachedParamMgr
    if arrangement.startswith("worker"):
        monkeypatch.setenv("CE_WORKER_ADMIT", "sdma" if arrangement == "worker_sdma" else "kernel")
    lfu = strategy == "lfu"
    rng = np.random.default_rng(N + 31 * C)
    w = rng.standard_normal((N, D)).astype(np.float32)
    ora = OracleCachedParamMgr(w.copy(), C, LFU if lfu else DATASET)
    ora.reorder(None, 0.0)
    mgr = ce.CachedParamMgr(torch.from_numpy(w.copy()), C, evict_strategy=_strat(ce, strategy),
                            async_copy=arrangement == "staged")
    mgr.reorder(None, 0.0)
    if arrangement.startswith("worker"):
        mgr.set_transport("worker")
    klen = presort_len(per_call)
    evicted = 0
    for c in range(13):
        ids = rng.integers(0, N, size=per_call)
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
        assert np.array_equal(slots.view(-1).cpu().numpy(), want)
        if form >= 2:       # (the order inside a 16384-lookup segment depends on an atomic race in either form)
            ref = presort_window(slots.contiguous(), C)
            assert torch.equal(keys.view(1, -1, 16384).sort(dim=2).values, ref.view(1, -1, 16384).sort(dim=2).values)
        evicted += len(ora.traces[-1].evicted_rows)
        # a training step on the touched rows: every write-back carries a payload the host table has never seen
        ora.cuda_cached_weight[np.unique(want)] += np.float32(0.25 * (c + 1))
        with torch.no_grad():
            mgr.cuda_cached_weight[torch.unique(slots)] += 0.25 * (c + 1)
        _state_equal(mgr, ora, lfu)
    assert evicted > 2 * C, "the stream did not go round the cache twice"
    assert mgr.transport_name == arrangement.split("_")[0]          # (no fall-back to the zero-copy kernels)
    assert mgr.num_write_back_history == ora.num_write_back_history
    mgr.flush()
    ora.flush()
    np.testing.assert_array_equal(mgr.weight.numpy(), ora.weight)


def test_transport_switches_keep_the_table_consistent():
    """zerocopy -> worker -> staged -> worker -> zerocopy in the middle of a stream"""
    ce = _ce()
    from oracle.cache_oracle import DATASET, OracleCachedParamMgr
    rng = np.random.default_rng(5)
    N, C, D = 5000, 400, 64
    w = rng.standard_normal((N, D)).astype(np.float32)
    ora = OracleCachedParamMgr(w.copy(), C, DATASET)
    ora.reorder(None, 0.7)
    mgr = ce.CachedParamMgr(torch.from_numpy(w.copy()), C)
    mgr.reorder(None, 0.7)
    order = ["zerocopy", "worker", "staged", "worker", "zerocopy"]
    for c in range(20):
        mgr.set_transport(order[(c // 4) % len(order)])
        ids = rng.integers(0, N, size=250)
        eslots = ora.prepare_ids(ids)
        slots = mgr.prepare_ids(torch.from_numpy(ids).cuda())
        assert np.array_equal(slots.cpu().numpy(), eslots)
        ora.cuda_cached_weight[np.unique(eslots)] *= np.float32(1.5)
        with torch.no_grad():
            mgr.cuda_cached_weight[torch.unique(slots)] *= 1.5
        _state_equal(mgr, ora, False)
    np.testing.assert_array_equal(mgr.weight.numpy(), ora.weight)
    mgr.flush()
    ora.flush()
    np.testing.assert_array_equal(mgr.weight.numpy(), ora.weight)


def test_more_victims_than_the_staging_buffer_holds():
    """stage_rows is min(C, 262144): with a bigger cache the overflow takes the direct zero-copy path even under the
    worker transport; here the whole cache turns over in one call at D = 4 (C = 300k slots)."""
    ce = _ce()
    from oracle.cache_oracle import DATASET, OracleCachedParamMgr
    rng = np.random.default_rng(11)
    N, C, D = 900_000, 300_000, 4
    w = rng.standard_normal((N, D)).astype(np.float32)
    ora = OracleCachedParamMgr(w.copy(), C, DATASET)
    ora.reorder(None, 1.0)
    mgr = ce.CachedParamMgr(torch.from_numpy(w.copy()), C)
    mgr.reorder(None, 1.0)
    mgr.set_transport("worker")
    for c in range(3):
        ids = np.arange(C) + C * ((c + 1) % 3)            # a disjoint block of C rows: evicts everything
        eslots = ora.prepare_ids(ids)
        slots = mgr.prepare_ids(torch.from_numpy(ids).cuda())
        assert np.array_equal(slots.cpu().numpy(), eslots)
        ora.cuda_cached_weight += np.float32(1.0)
        with torch.no_grad():
            mgr.cuda_cached_weight += 1.0
    assert ora.num_write_back_history[-1] == C
    np.testing.assert_array_equal(mgr.weight.numpy(), ora.weight)


@pytest.mark.test_hooks
def test_overflow_tail_readmits_rows_of_a_slow_previous_writeback(monkeypatch):
    """a call that misses more rows than the staging buffer holds reads the rows past it zero-copy
    out of the host table.  With the relaxed write-back order the previous call's write-back may still be on its way
    then -- so rows that call evicted THROUGH ITS STAGED PART and that land in this call's overflow tail must not be
    read before it has arrived.  Call 2's miss list is [300k, 550k) + [600k, 650k): positions >= 262144 are rows
    [612144, 650k), which call 1 evicted among its first 262144 (staged) victims; every write-back starts 30 ms late."""
    monkeypatch.setenv("CE_WORKER_ADMIT", "kernel")
    monkeypatch.setenv("CE_WORKER_OUT_DELAY_US", "30000")
    ce = _ce()
    from oracle.cache_oracle import DATASET, OracleCachedParamMgr
    rng = np.random.default_rng(12)
    N, C, D = 900_000, 300_000, 4
    w = rng.standard_normal((N, D)).astype(np.float32)
    ora = OracleCachedParamMgr(w.copy(), C, DATASET)
    ora.reorder(None, 1.0)
    mgr = ce.CachedParamMgr(torch.from_numpy(w.copy()), C)
    mgr.reorder(None, 1.0)
    mgr.set_transport("worker")
    calls = [np.arange(600_000, 900_000), np.arange(0, 300_000),
             np.concatenate([np.arange(300_000, 550_000), np.arange(600_000, 650_000)])]
    for c, ids in enumerate(calls):
        eslots = ora.prepare_ids(ids)
        slots = mgr.prepare_ids(torch.from_numpy(ids).cuda())
        assert np.array_equal(slots.cpu().numpy(), eslots)
        if c == 2:
            tail = ora.traces[-1].miss_rows[262144:]
            assert len(tail) and np.isin(tail, calls[0][:262144]).all()       # the case this test is about
        np.testing.assert_array_equal(mgr.cuda_cached_weight.detach().cpu().numpy(), ora.cuda_cached_weight)
        ora.cuda_cached_weight += np.float32(c + 1.0)
        with torch.no_grad():
            mgr.cuda_cached_weight += c + 1.0
    mgr.flush()
    ora.flush()
    np.testing.assert_array_equal(mgr.weight.numpy(), ora.weight)


def test_overlapped_window_raises_on_overflow():
    """strict=False pipelines must not train on -1 slots silently: the failed call is reported one window late"""
    ce = _ce()
    from cachedembedding_amd.pipeline import PrefetchWindow
    N, D, C = 4000, 16, 300
    emb = ce.CachedEmbeddingBag(N, D, sparse=True, mode="sum", include_last_offset=True, cuda_row_num=C,
                                warmup_ratio=0.7)
    win = PrefetchWindow(emb, 2, overlap=True, transport="worker")
    g = torch.Generator().manual_seed(0)
    ok = [torch.randint(0, N, (64,), generator=g).cuda() for _ in range(2)]
    too_many = [torch.arange(0, 400).cuda(), torch.arange(400, 800).cuda()]      # 800 unique rows > 300 slots
    win.submit(ok)
    win.collect()
    win.submit(too_many)
    with pytest.raises(AssertionError, match="increase cuda_row_num"):
        # the check is non-blocking: the failed call is reported by the first collect() that finds its record --
        # this one if the GPU was quick, the next one at the latest (the record is complete after the sync)
        slots = win.collect()
        torch.cuda.synchronize()
        assert int(slots[0].min()) == -1
        win.submit(ok)
        win.collect()


def test_phase_timers_and_history_window():
    ce = _ce()
    N, D, C = 3000, 32, 200
    mgr = ce.CachedParamMgr(torch.randn(N, D), C)
    mgr.reorder(None, 0.5)
    mgr.set_profiling(True)
    g = torch.Generator().manual_seed(1)
    for _ in range(20):
        mgr.prepare_ids(torch.randint(0, N, (150,), generator=g).cuda())
    t = mgr.phase_times()
    assert t["calls"] == 20
    names = [k for k in t if k != "calls"]
    assert len(names) == 6 and all(t[k] >= 0.0 for k in names) and sum(t[k] for k in names) > 0.0
    assert len(mgr.num_hits_history) == 20
    mgr.set_profiling(False)


@pytest.mark.timeout(300)
def test_worker_transport_with_more_streams_than_hardware_queues():
    """HIP multiplexes streams onto a few hardware queues (4 unless GPU_MAX_HW_QUEUES says otherwise).  The cache-op
    stream parks in hipStreamWaitValue64 while the admission worker copies rows in: nothing that releases it may sit
    in a hardware queue behind the parked wait.  Many live streams force queue sharing; the calls go round them."""
    ce = _ce()
    from oracle.cache_oracle import DATASET, OracleCachedParamMgr
    extra = [torch.cuda.Stream() for _ in range(24)]
    x = torch.ones(1 << 20, device="cuda")
    for st in extra:
        with torch.cuda.stream(st):
            x.add_(1.0)
    torch.cuda.synchronize()
    rng = np.random.default_rng(77)
    N, C, D = 30000, 2000, 64
    w = rng.standard_normal((N, D)).astype(np.float32)
    ora = OracleCachedParamMgr(w.copy(), C, DATASET)
    ora.reorder(None, 0.7)
    mgrs = []
    for k in range(3):                       # several managers alive at once: 3 x (1 admission + 2 write-back streams)
        m = ce.CachedParamMgr(torch.from_numpy(w.copy()), C)
        m.reorder(None, 0.7)
        m.set_transport("worker")
        mgrs.append(m)
    oras = [ora] + [None, None]
    oras[1] = OracleCachedParamMgr(w.copy(), C, DATASET); oras[1].reorder(None, 0.7)
    oras[2] = OracleCachedParamMgr(w.copy(), C, DATASET); oras[2].reorder(None, 0.7)
    for c in range(30):
        st = extra[(5 * c) % len(extra)]
        ids = rng.integers(0, N, size=900)
        with torch.cuda.stream(st):
            for m, o in zip(mgrs, oras):
                slots = m.prepare_ids(torch.from_numpy(ids).cuda())
                assert np.array_equal(slots.cpu().numpy(), o.prepare_ids(ids))
        # busy neighbours on other streams while the next call runs
        for s2 in extra[c % 7::7]:
            with torch.cuda.stream(s2):
                x.mul_(1.0)
        torch.cuda.synchronize()
    for m, o in zip(mgrs, oras):
        np.testing.assert_array_equal(m.weight.numpy(), o.weight)


@pytest.mark.parametrize("strategy", ["dataset", "lfu"])
def test_worker_transport_empty_and_ragged_calls(strategy):
    """calls of very different sizes, including empty ones and calls without any miss, back to back"""
    ce = _ce()
    from oracle.cache_oracle import DATASET, LFU, OracleCachedParamMgr
    rng = np.random.default_rng(9)
    N, C, D = 8000, 900, 32
    w = rng.standard_normal((N, D)).astype(np.float32)
    ora = OracleCachedParamMgr(w.copy(), C, LFU if strategy == "lfu" else DATASET)
    ora.reorder(None, 0.5)
    mgr = ce.CachedParamMgr(torch.from_numpy(w.copy()), C, evict_strategy=_strat(ce, strategy))
    mgr.reorder(None, 0.5)
    mgr.set_transport("worker")
    sizes = [0, 1, 700, 0, 0, 5, 850, 3, 0, 600, 600, 1, 0]
    for c, n in enumerate(sizes):
        ids = rng.integers(0, N, size=n)
        if c == 7:
            ids = np.asarray(ora.cached_idx_map[ora.cached_idx_map >= 0][:3])      # hits only: nothing moves
        eslots = ora.prepare_ids(ids)
        slots = mgr.prepare_ids(torch.from_numpy(ids).cuda())
        assert np.array_equal(slots.cpu().numpy(), eslots)
        if len(eslots):
            ora.cuda_cached_weight[np.unique(eslots)] += np.float32(1.0)
            with torch.no_grad():
                mgr.cuda_cached_weight[torch.unique(slots)] += 1.0
        _state_equal(mgr, ora, strategy == "lfu")
    assert mgr.num_hits_history == ora.num_hits_history and mgr.num_miss_history == ora.num_miss_history
    np.testing.assert_array_equal(mgr.weight.numpy(), ora.weight)
    mgr.flush()
    ora.flush()
    np.testing.assert_array_equal(mgr.weight.numpy(), ora.weight)


@pytest.mark.test_hooks
@pytest.mark.parametrize("strict", [True, False])
def test_a_failed_admission_releases_the_stream_and_admits_nothing(strict, monkeypatch):
    """Host-gather admission (CE_WORKER_ADMIT=sdma: the one form of the worker transport that still has a library
    thread and a parked stream between a call's front and its rows).  The admission worker reports a failed HIP call
    for job 3 (test hook CE_WORKER_FAIL_IN_JOB): the parked cache-op stream must be released all the same (no hang), the
    call's record must say CE_ERR_HIP, every slot of the call is -1, NONE of the rows it missed may be resident
    afterwards (their payload never arrived: a later flush would write garbage home), and the engine stays failed: the
    next call raises instead of training on a table that has lost rows."""
    ce = _ce()
    from cachedembedding_amd import _lib
    from oracle.cache_oracle import DATASET, OracleCachedParamMgr
    monkeypatch.setenv("CE_WORKER_ADMIT", "sdma")
    monkeypatch.setenv("CE_WORKER_FAIL_IN_JOB", "3")
    rng = np.random.default_rng(17)
    N, C, D = 6000, 500, 64
    w = rng.standard_normal((N, D)).astype(np.float32)
    ora = OracleCachedParamMgr(w.copy(), C, DATASET)
    ora.reorder(None, 0.5)
    mgr = ce.CachedParamMgr(torch.from_numpy(w.copy()), C)
    mgr.reorder(None, 0.5)
    mgr.set_transport("worker")
    mgr.strict = strict
    ids = [rng.integers(0, N, size=300) for _ in range(5)]
    for c in range(2):
        eslots = ora.prepare_ids(ids[c])
        slots = mgr.prepare_ids(torch.from_numpy(ids[c]).cuda())
        assert np.array_equal(slots.cpu().numpy(), eslots)
    _state_equal(mgr, ora, False)
    resident_before = ora.cached_idx_map.copy()
    ora.prepare_ids(ids[2])                                       # what the call WOULD have done
    missed, evicted = ora.traces[-1].miss_rows, ora.traces[-1].evicted_rows
    assert len(missed) > 50 and len(evicted) > 50
    if strict:
        with pytest.raises(_lib.CeError) as ei:
            mgr.prepare_ids(torch.from_numpy(ids[2]).cuda())
        assert ei.value.code == _lib.CE_ERR_HIP
    else:
        slots = mgr.prepare_ids(torch.from_numpy(ids[2]).cuda())
        torch.cuda.synchronize()                                  # returns: the stream was released
        assert (slots.cpu().numpy() == -1).all()
        with pytest.raises(_lib.CeError) as ei:
            mgr.raise_on_failed_calls()
        assert ei.value.code == _lib.CE_ERR_HIP
    torch.cuda.synchronize()
    inv = mgr.inverted_cached_idx.cpu().numpy()
    cmap = mgr.cached_idx_map.cpu().numpy().astype(np.int64)
    assert (inv[missed] == -1).all(), "a row whose payload never arrived is marked resident"
    assert (inv[evicted] == -1).all()                             # the victims did leave
    assert not np.isin(cmap[cmap >= 0], missed).any()
    kept = np.setdiff1d(resident_before[resident_before >= 0], evicted)
    assert np.array_equal(np.sort(cmap[cmap >= 0]), np.sort(kept)), "rows the call did not touch stay where they were"
    with pytest.raises(_lib.CeError, match="injected"):           # the engine stays failed
        mgr.prepare_ids(torch.from_numpy(ids[3]).cuda())


def test_hook_tests_on_the_test_hooks_build():
    """The tests marked `test_hooks` need a write-back that starts late or an admission job that fails; the product
    library has no such switches (tests/test_abi.py), so they run here: one child pytest process bound
    to libce_hip_testhooks.so (the same objects with ce_cache.hip recompiled under -DCE_TEST_HOOKS, built by
    __graft_entry__.build()).  Every one of them must pass there, none may be skipped."""
    import os
    import re
    import subprocess
    import sys
    from conftest import HOOKS_LIB, ROOT, hooks_build_loaded
    if hooks_build_loaded():
        pytest.skip("this IS the child process")
    if not HOOKS_LIB.exists():                  # (normally built by __graft_entry__.build() and shipped with the tree)
        from cachedembedding_amd import build as _b
        _b.build_test_hooks()
    assert HOOKS_LIB.exists(), f"{HOOKS_LIB} is missing: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, CE_LIBRARY=str(HOOKS_LIB))
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_worker.py"), "-q", "-x",
                        "-m", "gpu and test_hooks", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True,
                       timeout=1200, cwd=str(ROOT))
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == 15 and "skipped" not in r.stdout.splitlines()[-1], tail
