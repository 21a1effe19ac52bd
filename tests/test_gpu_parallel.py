"""GPU tests of the sharded paths.  Only one GPU is available to the tests, so world_size 2 runs as two
processes sharing cuda:0 over gloo (the exchange stages through host memory; on a real node the same
code runs over RCCL) -- what is exercised here is HipShardOps (ce_bucketize_rows, owner cache op,
gather/pool/grad kernels) plus the exchange bookkeeping, checked against plain torch on the full table."""
import os
import socket
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _entry(fn, rank, world, port, q, args, backend="gloo"):
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    try:
        if backend == "nccl":
            # one rank per GPU over RCCL / xGMI: the way bench.py --gpus N runs
            torch.cuda.set_device(rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
        else:
            torch.cuda.set_device(0)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        fn(rank, world, *args)
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:
        import traceback
        q.put((rank, "fail", traceback.format_exc()))


def _spawn(fn, world, *args, backend="gloo"):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_entry, args=(fn, r, world, port, q, args, backend)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    res = []
    while not q.empty():
        res.append(q.get())
    assert len(res) == world, f"only {len(res)} of {world} ranks reported"
    for r in res:
        assert r[1] == "ok", r


def _rowwise(rank, world, strategy, with_freq, overlap=False):
    import cachedembedding_amd as ce
    from cachedembedding_amd.parallel import RowwiseShardedEmbeddingBag, ShardedWindowPipeline
    torch.manual_seed(0)
    N, D, F, B_loc, P, lr = 5003, 64, 4, 32, 3, 0.25
    w_full = torch.randn(N, D)
    freq = torch.randint(0, 50, (N,)) if with_freq else None
    strat = ce.EvictionStrategy.LFU if strategy == "lfu" else ce.EvictionStrategy.DATASET
    if with_freq and strategy == "dataset":
        order = torch.argsort(freq, descending=True, stable=True)
        id2row = torch.empty(N, dtype=torch.long)
        id2row[order] = torch.arange(N)
    else:
        id2row = torch.arange(N)
    # global table indexed by ROW; shard r holds rows r, r+W, ...
    shard = w_full[rank::world].contiguous()
    emb = RowwiseShardedEmbeddingBag(N, D, mode="sum", include_last_offset=True, ids_freq_mapping=freq,
                                     warmup_ratio=0.7, evict_strategy=strat, _weight_shard=shard,
                                     cuda_row_num=(1000 if overlap else 600) * world)
    emb.set_fused_sgd(lr)
    g = torch.Generator().manual_seed(100 + rank)
    offsets = torch.arange(F * B_loc + 1, dtype=torch.int32, device="cuda")
    ref_w = w_full.clone()
    nwin = 4 if overlap else 2
    all_ids = [[torch.randint(0, N, (F * B_loc,), generator=g) for _ in range(P)] for _ in range(nwin)]
    if overlap:     # static bag layout known at plan time: the gradient fold streams over source-row keys
        emb.ops.set_bag_layout(offsets, True, F)
    pipe = ShardedWindowPipeline(emb, overlap=overlap)
    pipe.submit([i.cuda() for i in all_ids[0]])
    for window in range(nwin):
        ids_list = all_ids[window]
        if window + 1 < nwin:
            pipe.submit([i.cuda() for i in all_ids[window + 1]])
        plans = pipe.collect()
        for ids, plan in zip(ids_list, plans):
            go = torch.randn(B_loc, F, D, generator=g)
            if overlap:     # the straight-line step bench.py uses (no autograd engine)
                out = emb.forward_backward(plan, offsets, go.cuda(), hook_features=F)
            else:
                out = emb(plan, offsets, hook_features=F)
                out.backward(go.cuda())
            exp = ref_w[id2row[ids]].view(F, B_loc, D).transpose(0, 1)
            torch.testing.assert_close(out.cpu(), exp, rtol=1e-5, atol=1e-6)
            pipe.pump()                         # next window's plan advances one phase between steps
            packs = [None] * world
            dist.all_gather_object(packs, (ids, go))
            for pids, pgo in packs:
                ref_w.index_add_(0, id2row[pids], pgo.transpose(0, 1).reshape(-1, D), alpha=-lr)
    assert emb.cache_weight_mgr.sync_stats().status == 0
    emb.flush()
    torch.testing.assert_close(emb.weight, ref_w[rank::world], rtol=1e-4, atol=1e-5)


def _rowwise_graphed(rank, world, strategy, with_freq, capacity, overlap, sizes=(5003, 64, 4, 32, 3, 1000),
                     force_graph=False, stream="random", expect_split=None, flip=False):
    # stream: how consecutive batches relate -- "random" draws; "same": every batch of a window looks up the SAME rows
    # (every row late and urgent: what the split must not overtake); "disjoint": consecutive batches share no row (all
    # early / deferred: everything may travel ahead)
    """parallel.GraphedShardedWindow (fixed-capacity exchange, the window's steps replayed as one hipGraph at world 1,
    launched one by one over gloo) against plain torch on the full table: pooled output of every step, table after
    flush.  capacity below the bucket sizes forces every window through the variable-size fallback."""
    import cachedembedding_amd as ce
    from cachedembedding_amd.parallel import GraphedShardedWindow, RowwiseShardedEmbeddingBag
    torch.manual_seed(0)
    (N, D, F, B_loc, P, C_rank), lr = sizes, 0.25
    w_full = torch.randn(N, D)
    freq = torch.randint(0, 50, (N,)) if with_freq else None
    strat = ce.EvictionStrategy.LFU if strategy == "lfu" else ce.EvictionStrategy.DATASET
    if with_freq and strategy == "dataset":
        order = torch.argsort(freq, descending=True, stable=True)
        id2row = torch.empty(N, dtype=torch.long)
        id2row[order] = torch.arange(N)
    else:
        id2row = torch.arange(N)
    shard = w_full[rank::world].contiguous()
    emb = RowwiseShardedEmbeddingBag(N, D, mode="sum", include_last_offset=True, ids_freq_mapping=freq,
                                     warmup_ratio=0.7, evict_strategy=strat, _weight_shard=shard,
                                     cuda_row_num=C_rank * world)
    emb.set_fused_sgd(lr)
    g = torch.Generator().manual_seed(100 + rank)
    offsets = torch.arange(F * B_loc + 1, dtype=torch.int32, device="cuda")
    emb.ops.set_bag_layout(offsets, True, F)
    nwin = 4
    if N > 100000:       # bench-shaped: skewed ids, ~10 % distinct rows per batch
        all_ids = [[(torch.rand(F * B_loc, generator=g) ** 5 * N).long().clamp_(0, N - 1) for _ in range(P)]
                   for _ in range(nwin + 1)]
    elif stream == "same":
        gs = torch.Generator().manual_seed(7)              # (the same rows on EVERY rank, too)
        all_ids = [[torch.randint(0, N, (F * B_loc,), generator=gs)] * P for _ in range(nwin + 1)]
    elif stream == "alternating":
        # even windows look up 50 rows (every bucket fits the capacity), odd windows ~250 distinct rows per batch (every
        # bucket overflows it): with `flip` the arrangement changes between a window's submit() and its run()
        all_ids = [[torch.randint(0, 50 if w_ % 2 == 0 else N, (F * B_loc,), generator=g) for _ in range(P)]
                   for w_ in range(nwin + 1)]
    elif stream == "disjoint":
        # batch b of a window draws from the rows congruent to b modulo P + 1 (and the first batch of the next window
        # from another class than the last batch of this one): on every rank, so no row is touched in two consecutive steps
        k = P + 1
        all_ids = [[torch.randint(0, N // k, (F * B_loc,), generator=g) * k + (b + w_) % k for b in range(P)]
                   for w_ in range(nwin + 1)]
    else:
        all_ids = [[torch.randint(0, N, (F * B_loc,), generator=g) for _ in range(P)] for _ in range(nwin + 1)]
    go = torch.randn(P, B_loc, F, D, generator=g)               # one static upstream gradient per batch of a window
    big = N > 100000
    if big:
        # bench shape: held to the per-element bound of tests/test_gpu_bag.py::test_full_size_step_vs_torch_cpu
        # (oracle/closed_form.py's: cold rows 1e-5 relative with no floor, hot rows + 3e-4 lr grad_rms sqrt(lookups); reference in fp64)
        go *= 0.01
        ref64 = w_full.double()
        abs64 = torch.zeros(N, D, dtype=torch.float64)           # sum |lr g| per row and element (the cold rows' scale)
        cnt = torch.zeros(N, dtype=torch.float64)
    go_d = go.cuda()
    outs = torch.zeros(P, B_loc, F, D, device="cuda")

    def dense_fn(out, i):
        outs[i].copy_(out)
        return go_d[i]

    ref_w = w_full.clone()
    # window 0 doubles as the warm-up (it trains once eagerly inside the constructor): account for it
    hook_ran = []

    def before_capture(w):
        # the work a caller times on candidate gradient buffers: the table update at lr = 0 must leave the table as it is
        before = w._table.clone()
        w.enqueue_update_lr0(torch.randn(B_loc, F, D, device="cuda"))
        torch.cuda.synchronize()
        assert torch.equal(before, w._table)
        hook_ran.append(w.out_lottery)

    # (the pooled output of every step in ONE static buffer picked among three candidates; before_capture as above)
    gw = GraphedShardedWindow(emb, P, F * B_loc, offsets, dense_fn, capacity=capacity, hook_features=F,
                              overlap=overlap, warmup_ids=[i.cuda() for i in all_ids[0]],
                              use_graph=True if force_graph else None, static_out_candidates=3,
                              before_capture=before_capture) if capacity >= 64 else \
        GraphedShardedWindow(emb, P, F * B_loc, offsets, dense_fn, capacity=capacity, hook_features=F, overlap=overlap)
    if capacity >= 64:
        assert len(hook_ran) == 1 and hook_ran[0] is not None and len(hook_ran[0]["us"]) == 3
        assert gw._out_static is not None and tuple(gw._out_static.shape) == (B_loc, F, D)
    if force_graph and rank == 0:
        print("window steps with RCCL all-to-alls inside:", "captured as hipGraphs" if gw._graphs is not None
              else "capture refused -> launched one by one", flush=True)

    def reference_window(ids_list):
        exp = []
        for i, ids in enumerate(ids_list):
            src = ref64 if big else ref_w
            exp.append(src[id2row[ids]].view(F, B_loc, D).transpose(0, 1).clone())
            packs = [None] * world
            dist.all_gather_object(packs, ids)
            packs_go = [None] * world
            dist.all_gather_object(packs_go, go[i])
            for pids, pgo in zip(packs, packs_go):
                ref_w.index_add_(0, id2row[pids], pgo.transpose(0, 1).reshape(-1, D), alpha=-lr)
                if big:
                    ref64.index_add_(0, id2row[pids], pgo.transpose(0, 1).reshape(-1, D).double(), alpha=-lr)
                    abs64.index_add_(0, id2row[pids], pgo.transpose(0, 1).reshape(-1, D).double().abs(), alpha=lr)
                    cnt.add_(torch.bincount(id2row[pids], minlength=N))
        return exp

    def bound(ref, rows_cnt, abs_sum):
        # oracle/closed_form.py's bound (round 5): <= 4 lookups 1e-5 of max(|ref|, sum |lr g|), no absolute floor;
        # more: 1e-5 |ref| + 3e-4 lr grad_rms sqrt(lookups)
        from oracle.closed_form import elementwise_bound
        return elementwise_bound(ref.reshape(-1, D), rows_cnt.reshape(-1), abs_sum.reshape(-1, D), lr, 0.01).view(ref.shape)

    if capacity >= 64:
        reference_window(all_ids[0])                 # the eager warm-up pass of the constructor
    first = 1
    if overlap:
        gw.submit([i.cuda() for i in all_ids[first]], first % 2)
    for w in range(first, nwin + 1):
        if not overlap:             # reference semantics: a window's cache op runs when the one before has trained
            gw.submit([i.cuda() for i in all_ids[w]], w % 2)
        elif w + 1 <= nwin:
            gw.submit([i.cuda() for i in all_ids[w + 1]], (w + 1) % 2)
            if flip:       # a plan submitted under one arrangement, trained under the other
                gw.set_arrangement("overlap" if gw.arrangement == "interleaved" else "interleaved")
        gw.run(w % 2)
        torch.cuda.synchronize()
        exp = reference_window(all_ids[w])
        for i in range(P):
            if not big:
                torch.testing.assert_close(outs[i].cpu(), exp[i], rtol=1e-5, atol=1e-5)
                continue
            # a pooled row IS the table row at that step (one id per bag): the row's bound, with the lookups it has
            # summed by the end of this window (a hot row collects thousands of fp32 atomic updates per window)
            rws = id2row[all_ids[w][i]]
            c = cnt[rws].view(F, B_loc).transpose(0, 1)
            a = abs64[rws].view(F, B_loc, D).transpose(0, 1)
            assert bool(((outs[i].cpu().double() - exp[i]).abs() <= bound(exp[i], c, a)).all())
    if expect_split is not None:
        assert gw._split == (expect_split and world > 1)
    if gw._split and stream in ("same", "disjoint") and capacity >= 64:
        # the classification of the last planned window, as the owner made it (bit 0 late, bit 1 urgent)
        fl = gw._flags_o[nwin % 2].cpu()
        valid = gw._serve[nwin % 2].cpu() >= 0
        if stream == "same":
            assert bool((fl[:, 1:][valid[:, 1:]] & 1).bool().all()) and bool((fl[valid] & 2).bool().all())
        else:
            assert not bool((fl[valid] & 1).bool().any()) and not bool((fl[:, :-1][valid[:, :-1]] & 2).bool().any())
    if stream == "alternating":
        assert gw.fallback_windows == nwin // 2, gw.fallback_windows      # windows 1 and 3 of 1..4
    elif capacity < 64:
        assert gw.fallback_windows == nwin
    else:
        assert gw.fallback_windows == 0
        if world == 1:
            assert gw._graphs is not None, "the window's steps were not captured"
    assert emb.cache_weight_mgr.sync_stats().status == 0
    emb.flush()
    if not big:
        torch.testing.assert_close(emb.weight, ref_w[rank::world], rtol=1e-4, atol=1e-5)
    else:
        mine, c, a = ref64[rank::world], cnt[rank::world], abs64[rank::world]
        err = (emb.weight.double() - mine).abs()
        bd = bound(mine, c, a)
        assert bool((err <= bd).all()), float((err / bd.clamp(min=1e-300)).max())
        assert bool(((ref_w[rank::world].double() - mine).abs() <= bd).all())      # torch fp32: same bound
        assert float(cnt.max()) > 1e5, "the case must have rows that sum very many gradients"


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("strategy,with_freq", [("dataset", True), ("lfu", False)])
@pytest.mark.parametrize("capacity,overlap", [(256, True), (256, False), (8, True)])
def test_rowwise_graphed_fixed_capacity_window(world, strategy, with_freq, capacity, overlap):
    _spawn(_rowwise_graphed, world, strategy, with_freq, capacity, overlap)


@pytest.mark.parametrize("world", [1, 2])
def test_arrangement_flips_between_submit_and_run_of_an_overflowing_window(world):
    """run() must wait for the overflow flag of a plan that ran on the training stream (submitted under
    'interleaved') even when the arrangement has changed to 'overlap' by the time the window trains -- otherwise it reads
    the flag of the window before (here: "fits" for a window that overflows, i.e. rows pooled as zeros and their
    gradients dropped).  Every second window overflows its buckets; the arrangement flips after every submit()."""
    _spawn(_rowwise_graphed, world, "dataset", True, 64, True, (5003, 64, 4, 64, 3, 1000), False, "alternating", None, True)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", ["split", "all_late", "off", "stream_same", "stream_disjoint"])
def test_rowwise_graphed_window_early_late_split(world, mode, monkeypatch):
    """The early / late split of the row exchanges: rows nobody touched in the step before travel while
    that step computes, the gradients of rows nobody needs in the step after return behind it.  Same per-step pooled
    outputs and the same table as plain torch on the full table with the split as classified ("split"), with every row
    forced late + urgent ("all_late": the synchronous exchange in split form), switched off ("off": round 4's step),
    and on id streams that make every row late ("stream_same") or every row early ("stream_disjoint")."""
    if mode == "all_late":
        monkeypatch.setenv("CE_SPLIT_FORCE", "late")
    if mode == "off":
        monkeypatch.setenv("CE_SHARDED_SPLIT", "0")
    stream = {"stream_same": "same", "stream_disjoint": "disjoint"}.get(mode, "random")
    _spawn(_rowwise_graphed, world, "dataset", True, 512, True, (5003, 64, 4, 32, 4, 1000), False, stream, mode != "off")


@pytest.mark.parametrize("world", [1, 2])
def test_rowwise_graphed_window_at_the_benchmarked_batch_shape(world):
    """the same check with the bench's batch shape: 26 features x 16384 samples per rank, D = 128, skewed ids, two
    batches per window (window dedupe: one launch per pass for both), buckets of up to 262144 rows, against torch's
    index_add_ on the full 2 M-row table"""
    _spawn(_rowwise_graphed, world, "dataset", True, 262144, True, (2_000_003, 128, 26, 16384, 2, 1_200_000 // world))


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("strategy,with_freq", [("dataset", True), ("lfu", False), ("lfu", True)])
def test_rowwise_sharded_vs_full_table(world, strategy, with_freq):
    _spawn(_rowwise, world, strategy, with_freq)


@pytest.mark.parametrize("world", [1, 2])
def test_rowwise_sharded_overlapped_window_pipeline(world):
    """window plans built one window ahead on a side stream (protect_depth 1) train identically"""
    _spawn(_rowwise, world, "dataset", True, True)


def _column(rank, world):
    import cachedembedding_amd as ce
    from cachedembedding_amd.parallel import ParallelCachedEmbeddingBag
    torch.manual_seed(0)
    N, D, F, Bg = 2000, 96, 3, 8
    w = torch.randn(N, D)
    emb = ParallelCachedEmbeddingBag(N, D, sparse=True, _weight=w.clone(), mode="sum", include_last_offset=True,
                                     cache_ratio=0.2, warmup_ratio=0.7)
    ids = torch.randint(0, N, (F * Bg,))                 # GLOBAL batch, identical on every rank
    off = torch.arange(F * Bg + 1, dtype=torch.int32)
    out = emb(ids.cuda(), off.cuda(), shape_hook=lambda x: x.view(F, Bg, -1).transpose(0, 1))
    exp = w[ids].view(F, Bg, D).transpose(0, 1)
    exp = torch.tensor_split(exp, world, dim=0)[rank]    # [B_glob/W, F, D]
    torch.testing.assert_close(out.cpu(), exp, rtol=1e-5, atol=1e-6)
    out.sum().backward()
    gw = emb.cache_weight_mgr.cuda_cached_weight.grad
    assert gw is not None and gw.is_sparse


@pytest.mark.parametrize("world", [1, 2])
def test_column_parallel_matches_reference_contract(world):
    _spawn(_column, world)


def test_bucketize_rows_stable_and_counts():
    import cachedembedding_amd as ce
    from cachedembedding_amd._lib import check, lib, ptr, stream_ptr
    torch.manual_seed(1)
    for n, W, N in [(1, 2, 10), (4097, 8, 100000), (50000, 3, 977), (8192, 64, 10**6)]:
        ids = torch.randint(0, N, (n,), device="cuda")
        idx_map = torch.randperm(N, device="cuda").int()
        rows = torch.empty(n, dtype=torch.int64, device="cuda")
        perm = torch.empty(n, dtype=torch.int64, device="cuda")
        counts = torch.empty(W, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.ce_bucketize_workspace(n, W), dtype=torch.uint8, device="cuda")
        check(lib.ce_bucketize_rows(ptr(ids), n, ptr(idx_map), W, ptr(rows), ptr(perm), ptr(counts), ptr(ws),
                                    ws.numel(), stream_ptr()))
        r = idx_map[ids].long()
        owner = r % W
        order = torch.argsort(owner, stable=True)
        assert torch.equal(counts, torch.bincount(owner, minlength=W))
        assert torch.equal(rows, (r // W)[order])
        exp_perm = torch.empty_like(order)
        exp_perm[order] = torch.arange(n, device="cuda")
        assert torch.equal(perm, exp_perm)


def test_dedupe_bucket_rows_properties():
    """ce_dedupe_bucket_rows: the unique rows of the batch, grouped by owner; pos maps every lookup to its row
    (the order inside a bucket is not specified, so the check is on the properties the exchange relies on)."""
    from cachedembedding_amd._lib import check, lib, ptr, stream_ptr
    torch.manual_seed(2)
    for n, W, N, skew in [(1, 2, 10, False), (4097, 8, 100000, True), (50000, 3, 977, False),
                          (8192, 64, 10**6, True), (425984, 8, 3_000_000, True), (1000, 1, 5000, False),
                          (255, 5, 300, False), (257, 7, 64, True), (1023, 2, 2000, False), (1025, 16, 40, True),
                          (70000, 8, 1, False), (3000, 4, 5000, None)]:
        if skew is None:   # one row carries every lookup
            ids = torch.full((n,), 1234, device="cuda", dtype=torch.long)
        elif skew:   # long-tail ids: many duplicates inside a wave
            ids = (torch.rand(n, device="cuda").pow(6) * N).long().clamp_(0, N - 1)
        else:
            ids = torch.randint(0, N, (n,), device="cuda")
        if n > 10:
            ids[3] = -1          # out-of-range ids are skipped: pos = -1
            ids[7] = N
        idx_map = torch.randperm(N, device="cuda").int()
        stamp = torch.randint(0, 2**31 - 1, (N,), dtype=torch.int32, device="cuda")   # garbage is fine
        slot = torch.empty(N, dtype=torch.int32, device="cuda")
        scratch = torch.empty((W + 1) * n, dtype=torch.int32, device="cuda")
        for _rep in (1, 2, 3):   # second call reuses the scratch arrays; third: ONE scratch array (slot_of_row = NULL)
            if _rep == 3:
                slot = None
            rows = torch.full((n,), -7, dtype=torch.int64, device="cuda")
            pos = torch.empty(n, dtype=torch.int64, device="cuda")
            counts = torch.empty(W, dtype=torch.int64, device="cuda")
            check(lib.ce_dedupe_bucket_rows(ptr(ids), n, ptr(idx_map), N, W, ptr(stamp), ptr(slot),
                                            ptr(scratch), ptr(rows), ptr(pos), ptr(counts), stream_ptr()))
            ok = (ids >= 0) & (ids < N)
            r = idx_map[ids[ok]].long()
            uniq = torch.unique(r)
            assert torch.equal(counts, torch.bincount(uniq % W, minlength=W))
            n_u = int(counts.sum())
            assert n_u == uniq.numel()
            assert bool((pos[~ok] == -1).all())
            # bucket w holds exactly the local rows of owner w, each once
            off = 0
            for w, c in enumerate(counts.tolist()):
                seg = rows[off:off + c]
                assert torch.equal(torch.sort(seg).values, torch.sort(uniq[uniq % W == w] // W).values)
                off += c
            # every lookup points at its own row: global row = local * W + owner(position)
            owner_of_pos = torch.repeat_interleave(torch.arange(W, device="cuda"), counts)
            p = pos[ok]
            assert bool(((p >= 0) & (p < n_u)).all())
            assert torch.equal(rows[p] * W + owner_of_pos[p], r)


@pytest.mark.parametrize("P", [1, 3, 8])
def test_dedupe_bucket_rows_padded_window_properties(P):
    """ce_dedupe_bucket_rows_padded (P = 1 per call) and its window form (the P batches in one launch per pass, one
    stamp array per batch): bucket w of batch b holds exactly the rows owner w has in that batch, each once, padded with
    -1 to the capacity; every lookup's place points at its own row; a bucket beyond the capacity raises the flag."""
    from cachedembedding_amd._lib import check, lib, ptr, stream_ptr
    torch.manual_seed(P)
    for n, W, N, cap in [(4097, 4, 100000, 2048), (50000, 3, 977, 512), (425984, 8, 3_000_000, 16384), (300, 1, 64, 64),
                         (1000, 2, 5000, 100)]:
        ids = (torch.rand(P, n, device="cuda").pow(4) * N).long().clamp_(0, N - 1)
        ids[0, 3] = -1
        ids[P - 1, 7] = N
        idx_map = torch.randperm(N, device="cuda").int()
        stamp = torch.randint(0, 2**31 - 1, (P * N,), dtype=torch.int32, device="cuda")
        slot = torch.empty(P * N, dtype=torch.int32, device="cuda")
        scratch = torch.empty(P * (W + 1) * n, dtype=torch.int32, device="cuda")
        rows = torch.full((P, W * cap), -7, dtype=torch.int64, device="cuda")
        pos = torch.full((P, n), -7, dtype=torch.int64, device="cuda")
        counts = torch.full((P, W), -7, dtype=torch.int64, device="cuda")
        ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
        for _rep in (1, 2, 3):   # third: ONE scratch array per batch (slot_of_row = NULL), what the pipelines pass
            if _rep == 3:
                slot = None
            ovf.zero_()
            if P == 1:
                check(lib.ce_dedupe_bucket_rows_padded(ptr(ids), n, ptr(idx_map), N, W, cap, ptr(stamp), ptr(slot),
                                                       ptr(scratch), ptr(rows), ptr(pos), ptr(counts), ptr(ovf),
                                                       stream_ptr()))
            else:
                check(lib.ce_dedupe_bucket_rows_padded_window(ptr(ids), n, P, ptr(idx_map), N, W, cap, ptr(stamp),
                                                              ptr(slot), ptr(scratch), ptr(rows), ptr(pos), ptr(counts),
                                                              ptr(ovf), stream_ptr()))
            over = False
            for b in range(P):
                ok = (ids[b] >= 0) & (ids[b] < N)
                r = idx_map[ids[b][ok]].long()
                uniq = torch.unique(r)
                exp_counts = torch.bincount(uniq % W, minlength=W)
                assert torch.equal(counts[b], exp_counts)
                over = over or bool((exp_counts > cap).any())
                assert bool((pos[b][~ok] == -1).all())
                for w in range(W):
                    seg = rows[b, w * cap:(w + 1) * cap]
                    c = min(int(exp_counts[w]), cap)
                    assert bool((seg[c:] == -1).all())
                    mine = uniq[uniq % W == w] // W
                    if c == mine.numel():
                        assert torch.equal(torch.sort(seg[:c]).values, torch.sort(mine).values)
                    else:       # overflowing bucket: a subset of the owner's rows, each once
                        assert torch.unique(seg[:c]).numel() == c and bool(torch.isin(seg[:c], mine).all())
                p = pos[b][ok]
                placed = p >= 0
                assert bool((p[placed] < W * cap).all())
                assert torch.equal(rows[b][p[placed]] * W + p[placed] // cap, r[placed])
                if not bool((exp_counts > cap).any()):
                    assert bool(placed.all())
            assert bool(ovf.item()) == over


def test_rows_axpy_matches_index_add():
    from cachedembedding_amd._lib import check, lib, ptr, stream_ptr
    torch.manual_seed(3)
    for R, D, n in [(1000, 128, 5000), (64, 32, 1), (5000, 64, 4097), (300, 100, 999), (300, 7, 50), (200, 256, 333),
                    (100, 512, 77)]:
        w = torch.randn(R, D, device="cuda")
        idx = torch.randint(0, R, (n,), device="cuda")
        if n > 4:
            idx[2] = -1
            idx[4] = R
        src = torch.randn(n, D, device="cuda")
        ok = (idx >= 0) & (idx < R)
        exp = w.clone().index_add_(0, idx[ok], src[ok], alpha=-0.5)
        check(lib.ce_rows_axpy(ptr(w), R, D, ptr(idx), n, ptr(src), -0.5, stream_ptr()))
        torch.testing.assert_close(w, exp, rtol=1e-5, atol=1e-5)   # fp32 sums, atomic order differs


def test_exchange_local_index_matches_numpy():
    """ce_exchange_local_index: places of a rank's own bucket -> the cache slot its owner side resolved, every other
    place -> a row of the receive buffer behind the cache, no place -> -1."""
    import numpy as np
    from cachedembedding_amd._lib import check, lib, ptr, stream_ptr
    rng = np.random.default_rng(11)
    for P, n, W, cap, rank, C in [(3, 1000, 4, 64, 1, 5000), (1, 17, 1, 32, 0, 100), (8, 4099, 2, 512, 1, 1 << 20),
                                  (2, 300, 8, 16, 7, 77)]:
        pos = rng.integers(-1, W * cap, size=(P, n)).astype(np.int64)
        slots = rng.integers(-1, C, size=(P, W * cap)).astype(np.int64)
        lo, hi = rank * cap, (rank + 1) * cap
        exp = np.where(pos < 0, -1, np.where((pos >= lo) & (pos < hi),
                                             np.take_along_axis(slots, np.clip(pos, 0, W * cap - 1), axis=1), C + pos))
        d_pos, d_slots = torch.from_numpy(pos).cuda(), torch.from_numpy(slots).cuda()
        out = torch.full((P, n), -7, dtype=torch.int64, device="cuda")
        check(lib.ce_exchange_local_index(ptr(d_pos), n, P, ptr(d_slots), W * cap, lo, hi, C, ptr(out), stream_ptr()))
        assert np.array_equal(out.cpu().numpy(), exp)
    # bad ranges are refused
    assert lib.ce_exchange_local_index(ptr(d_pos), n, P, ptr(d_slots), W * cap, 0, W * cap + 1, C, ptr(out),
                                       stream_ptr()) != 0


def test_reserve_tail_moves_the_cache_and_keeps_its_rows():
    """CachedParamMgr.reserve_tail: the cache moves into an allocation with extra rows behind it; resident rows,
    the Parameter object and later cache ops (admission, eviction, flush) are unaffected."""
    import cachedembedding_amd as ce
    torch.manual_seed(2)
    N, D, C = 5000, 32, 400
    w0 = torch.randn(N, D)
    emb = ce.CachedEmbeddingBag(N, D, _weight=w0.clone(), mode="sum", include_last_offset=True, cuda_row_num=C)
    mgr = emb.cache_weight_mgr
    ids = torch.randint(0, N, (300,), device="cuda")
    slots = mgr.prepare_ids(ids)
    param = mgr.cuda_cached_weight
    before = param.data[slots].clone()
    tail = mgr.reserve_tail(128)
    assert mgr.cuda_cached_weight is param and tail.shape == (128, D)
    assert tail.data_ptr() == param.data_ptr() + C * D * 4                  # right behind the cache
    assert torch.equal(param.data[slots], before) and torch.equal(before.cpu(), w0[ids.cpu()])
    assert mgr.reserve_tail(64).data_ptr() == tail.data_ptr()                # a smaller request reuses it
    tail.fill_(123.0)
    with torch.no_grad():
        param.data[slots] += 1.0                                             # "training" on the moved cache
    ids2 = torch.randint(0, N, (350,), device="cuda")                       # forces evictions of updated rows
    slots2 = mgr.prepare_ids(ids2)
    torch.testing.assert_close(param.data[slots2].cpu(),
                               w0[ids2.cpu()] + torch.isin(ids2, ids).cpu().float().unsqueeze(1), rtol=0, atol=0)
    emb.flush()
    exp = w0.clone()
    exp[ids.cpu().unique()] += 1.0
    torch.testing.assert_close(emb.weight, exp, rtol=0, atol=0)
    assert bool((tail == 123.0).all())                                       # no cache op touches the tail


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: one rank per GPU over RCCL")
@pytest.mark.parametrize("overlap", [False, True])
def test_rowwise_sharded_over_rccl(overlap):
    """the row-wise exchange with the `nccl` (= RCCL) backend, one rank per GPU: all_to_all_single with zero-length
    splits, the side streams of the window pipeline against RCCL's own stream, the worker transport beside the
    collectives.  Same oracle as the single-GPU runs: plain torch on the full table.  Skipped on one-GPU boxes."""
    world = min(torch.cuda.device_count(), 4)
    _spawn(_rowwise, world, "dataset", True, overlap, backend="nccl")
    _spawn(_rowwise, 2, "lfu", False, overlap, backend="nccl")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: one rank per GPU over RCCL")
def test_rowwise_graphed_window_captures_rccl_collectives_or_falls_back():
    """GraphedShardedWindow(use_graph=True) at world 2 over RCCL: a window's steps hold two all_to_all_single calls
    each; whether this stack can capture them into a hipGraph has never been run here.  Either outcome must train
    identically to plain torch on the full table: the captured graphs, or -- if the capture is refused -- the clean
    fallback to launching the same fixed-capacity steps one by one (a warning, no half-captured state)."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _spawn(_rowwise_graphed, 2, "dataset", True, 256, True, (5003, 64, 4, 32, 3, 1000), True, backend="nccl")


@pytest.mark.parametrize("ranks,extra", [(2, ["--verify_sharded"]), (3, ["--use_lfu"])])
def test_bench_multi_rank_path_with_ranks_sharing_the_gpu(ranks, extra):
    """`bench.py --gpus N` is launched by the driver as `torch.distributed.run --nproc-per-node N`; no multi-GPU box is
    available to the tests, so the same command runs with N ranks SHARING cuda:0 over gloo (--share_gpu) on a
    scaled-down table: window sizing (prefetch_num is lowered until the shard cache holds it -- the probing calls
    overflow on purpose), capacity choice, the fixed-capacity plan, the steps and the timed region all execute, and
    rank 0 prints ONE JSON line with the whole-job rate."""
    import json
    import subprocess
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), str(ROOT / "bench.py"), "--gpus", str(ranks), "--share_gpu",
           "--table_scale", "0.02", "--batch_size", "4096", "--steps", "16", "--warmup", "8", "--no_cpu_baseline",
           "--min_time", "0.05", "--full"] + extra
    r = subprocess.run(cmd, cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == ranks and out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["global_batch"] == 4096 * ranks
    if "--verify_sharded" in extra:
        v = out["verified"]
        assert v["pass"] and v["all_ranks"]["bound_violations"] == 0 and v["all_ranks"]["untouched_mismatch"] == 0
        assert v["all_ranks"]["rows"] > 100_000


@pytest.mark.parametrize("extra", [[], ["--interleaved"], ["--use_lfu", "--prefetch_num", "1"], ["--force_sharded"]])
def test_bench_one_gpu_line_carries_roofline_box_and_a_passing_verification(extra):
    """the driver's command on a scaled-down table: ONE JSON line with `roofline`, `cpu_baseline`-free here, the same-run
    `box` probe and `verified.pass` -- the closed-form check of the table the run leaves behind -- for the default
    pipeline, the one-stream form, LFU at prefetch_num 1 (cache op two windows ahead) and the row-wise path at W = 1."""
    import json
    import subprocess
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    cmd = [sys.executable, str(ROOT / "bench.py"), "--table_scale", "0.1", "--cache_ratio", "0.03", "--prefetch_num", "4",
           "--steps", "20", "--warmup", "5", "--no_cpu_baseline", "--min_time", "0.05", "--full"] + extra
    r = subprocess.run(cmd, cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["value"] > 0 and out["n_gpus"] == 1 and out["unit"] == "lookups/s"
    v = out["verified"]
    assert v["pass"] and v["bound_violations"] == 0 and v["untouched_mismatch"] == 0 and v["rows"] > 100_000, v
    if "--force_sharded" not in extra:
        # (the check ran on ids that bench.py had given back behind the steps and drew again afterwards -- or on resident
        # ones where a re-draw could not be confirmed; the line says which)
        assert out["config"]["id_windows"].startswith(("given back", "resident"))
        assert out["roofline"]["bound"] == "hbm" and 0 < out["roofline"]["frac"] < 1.2
        assert out["box"]["before"]["read_GBps"] > 1000 and out["it_per_s_scope"].startswith("embedding operator only")


def test_bench_plain_line_times_exactly_the_steps_and_dumps_the_last_step(tmp_path):
    """a plain run (no --full) on a scaled-down table: ONE JSON line with the headline alone -- `steps` timed steps,
    ms_per_step consistent with value -- and --dump-outputs writes the last timed step's forward output and updated
    rows as float32 files; the same command twice gives the same forward output (same inputs, same rows)"""
    import json
    import subprocess
    import numpy as np
    outs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--table_scale", "0.1", "--cache_ratio", "0.03",
               "--prefetch_num", "4", "--steps", "10", "--warmup", "5", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 10 and out["unit"] == "lookups/s" and out["higher_is_better"] is True
        assert out["dtype"] == "f32" and out["ms_per_step"] > 0
        lookups = out["config"]["batch_size"] * out["config"]["features"] * out["config"]["pooling"]
        assert abs(out["value"] * out["ms_per_step"] * 1e-3 / lookups - 1) < 1e-6
        for moved in ("roofline", "verified", "cpu_baseline", "box", "reference_window_semantics", "repeated_region"):
            assert moved not in out, moved
        fwd, upd = np.load(d / "forward_output.npy"), np.load(d / "updated_rows.npy")
        assert fwd.dtype == np.float32 and upd.dtype == np.float32
        assert fwd.shape[1:] == (26, 128) and upd.shape[:2] == fwd.shape[:2] and upd.shape[-1] == 128
        assert fwd.nbytes + upd.nbytes <= 64 << 20 and np.isfinite(fwd).all() and np.abs(fwd).max() > 0
        outs.append((fwd, upd))
    # (the rows that sum thousands of gradients per step by atomics differ in the last bits from run to run: held to
    # 1e-3 of the largest magnitude; other inputs would differ by the magnitude itself)
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-3 * float(np.abs(a).max()))


@pytest.mark.parametrize("W,P,cap,n_rows,fill", [(2, 4, 64, 500, 0.8), (3, 8, 1100, 9000, 0.9), (8, 8, 2500, 40000, 0.95),
                                                 (4, 1, 300, 1000, 0.5), (2, 5, 1024, 300, 1.0)])
def test_split_classify_and_places_against_a_plain_restatement(W, P, cap, n_rows, fill):
    """ce_split_classify / ce_split_places (the early / late split of the row-wise exchange) against loops in numpy:
    a row is LATE when any peer asks for it in the batch before, URGENT when any peer asks for it in the batch after
    (the last batch: always); places = rank inside the chunk's class, early rows that do not fit spill behind the late
    ones; the scratch mask is all zero again afterwards."""
    import numpy as np
    from cachedembedding_amd._lib import check, lib, ptr, stream_ptr
    rng = np.random.default_rng(W * 1000 + P * 10 + cap)
    serve = np.full((W, P, cap), -1, dtype=np.int64)
    for w in range(W):
        for b in range(P):
            k = int(cap * fill * rng.uniform(0.7, 1.0))
            serve[w, b, :k] = rng.choice(n_rows, size=min(k, n_rows), replace=False)[:k] if k <= n_rows else \
                rng.integers(0, n_rows, size=k)
    dev = "cuda"
    sv = torch.from_numpy(serve).to(dev)
    mask = torch.zeros(n_rows, dtype=torch.int64, device=dev)
    flags = torch.full((W, P, cap), 77, dtype=torch.uint8, device=dev)
    check(lib.ce_split_classify(ptr(sv), W, P, cap, n_rows, None, 0, ptr(mask), ptr(flags), stream_ptr()))
    assert int(mask.abs().sum()) == 0
    got = flags.cpu().numpy()
    sets = [set(serve[:, b, :][serve[:, b, :] >= 0].tolist()) for b in range(P)]
    exp = np.zeros_like(got)
    for w in range(W):
        for b in range(P):
            for j in range(cap):
                r = serve[w, b, j]
                if r < 0:
                    continue
                late = b > 0 and r in sets[b - 1]
                urgent = b == P - 1 or r in sets[b + 1]
                exp[w, b, j] = (1 if late else 0) | (2 if urgent else 0)
    assert np.array_equal(got, exp)
    # ---- places, batch-major, with capacities small enough to make some early / deferred rows spill
    ids = np.ascontiguousarray(serve.transpose(1, 0, 2))
    fl = np.ascontiguousarray(exp.transpose(1, 0, 2))
    valid = ids >= 0
    n_l = (valid & ((fl & 1) > 0)).sum(-1)
    n_e = valid.sum(-1) - n_l
    n_u = (valid & ((fl & 2) > 0)).sum(-1)
    n_d = valid.sum(-1) - n_u
    ce_ = max(1, int(n_e.max() * 0.8))
    cl = int(n_l.max() + max(0, n_e.max() - ce_)) + 1
    cd = max(1, int(n_d[:-1].max() * 0.8)) if P > 1 else 1
    caps = np.array([[ce_, cl, cd, cap]] * P, dtype=np.int32)
    skip = 1 % W
    pf = torch.empty(P, W * cap, dtype=torch.int32, device=dev)
    pb = torch.empty_like(pf)
    counts = torch.zeros(P, W, 4, dtype=torch.int32, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    ids_d, fl_d, caps_d = torch.from_numpy(ids).to(dev), torch.from_numpy(fl).to(dev), torch.from_numpy(caps).to(dev)
    check(lib.ce_split_places(ptr(ids_d), ptr(fl_d), P, W, cap, skip, ptr(caps_d), ptr(pf), ptr(pb), ptr(counts), ptr(ovf),
                              stream_ptr()))
    assert int(ovf) == 0
    c = counts.cpu().numpy()
    assert np.array_equal(c[..., 0], n_e) and np.array_equal(c[..., 1], n_l)
    assert np.array_equal(c[..., 2], n_d) and np.array_equal(c[..., 3], n_u)
    pf, pb = pf.cpu().numpy().reshape(P, W, cap), pb.cpu().numpy().reshape(P, W, cap)
    for b in range(P):
        for w in range(W):
            re = rl = rd = ru = 0
            for j in range(cap):
                if ids[b, w, j] < 0 or w == skip:
                    assert pf[b, w, j] == -1 and pb[b, w, j] == -1
                    continue
                if fl[b, w, j] & 1:
                    want = W * ce_ + w * cl + rl
                    rl += 1
                else:
                    want = w * ce_ + re if re < ce_ else W * ce_ + w * cl + n_l[b, w] + (re - ce_)
                    re += 1
                assert pf[b, w, j] == want, (b, w, j)
                cdb, cub = caps[b, 2], caps[b, 3]
                if fl[b, w, j] & 2:
                    want = W * cdb + w * cub + ru
                    ru += 1
                else:
                    want = w * cdb + rd if rd < cdb else W * cdb + w * cub + n_u[b, w] + (rd - cdb)
                    rd += 1
                assert pb[b, w, j] == want, (b, w, j)
    # a late region that is too small is reported, not silently truncated
    caps2 = caps.copy()
    caps2[:, 1] = max(1, int(n_l.max()) - 1)
    ovf.zero_()
    if n_l.max() > 1:
        caps2_d = torch.from_numpy(caps2).to(dev)
        pf2 = torch.empty(P, W * cap, dtype=torch.int32, device=dev)
        pb2 = torch.empty_like(pf2)
        check(lib.ce_split_places(ptr(ids_d), ptr(fl_d), P, W, cap, -1, ptr(caps2_d), ptr(pf2), ptr(pb2), None, ptr(ovf),
                                  stream_ptr()))
        assert int(ovf) == 1
