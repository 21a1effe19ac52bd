"""The calls behind tests/golden/cache_refusals.json: what the handle-based entries of ce_cache.hip refuse, with which
code and message, and in which order.  Shared by the recorder (tests/golden/record_cache_refusals.py) and the two
replays (tests/test_cache_refusals_cpu.py, tests/test_gpu_cache_refusals.py), so all walk the same calls in the same
order.

create_cases(): ce_cache_create refuses everything down to the workspace alignment before its first HIP call, so its bad
configurations run where no GPU is visible, on made-up addresses: every bad value alone and every two of them together
(of two bad values the entry names the one it checks first: the pairs pin the order).  A configuration that passes
every check reaches the first HIP call, which fails there (CE_ERR_HIP).

handle_cases(): every other entry, on one tiny cache of real arrays (N = 64, C = 8, D = 4, max_ids_per_call = 16).  Every
refusing call returns before any launch.  The refusals of a pending call need a call that is pending: one good
ce_cache_prepare_ids_begin_padded of four ids, finished at the end."""
import ctypes
import itertools

CE_ERR_HIP = 2
N, C, D, MAX_IDS = 64, 8, 4, 16
CE_EVICT_DATASET, CE_EVICT_LFU = 0, 1


def _p(i):
    return 0x7f0000000000 + 0x100000 * i            # non-null, 256-byte aligned


# ---------------------------------------------------------------------------------------------- ce_cache_create
_GOOD_CFG = dict(num_embeddings=N, cuda_row_num=C, embedding_dim=D, evict_strategy=CE_EVICT_LFU, transport=0,
                 protect_depth=0, max_ids_per_call=MAX_IDS, host_weight=_p(0), host_weight_dev=_p(1),
                 cache_weight=_p(2), idx_map=None, inverted_cached_idx=_p(3), cached_idx_map=_p(4), freq_cnter=_p(5),
                 workspace=_p(6), workspace_bytes=None)         # None: what ce_cache_workspace_bytes asks for

# (label, argument or field, bad value); "cfg" / "out": the argument itself is NULL
CREATE_SINGLES = [
    ("cfg=null", "cfg", None), ("out=null", "out", None),
    ("num_embeddings=0", "num_embeddings", 0), ("num_embeddings=2^31-1", "num_embeddings", 2 ** 31 - 1),
    ("cuda_row_num=0", "cuda_row_num", 0), ("cuda_row_num=N+1", "cuda_row_num", N + 1),
    ("embedding_dim=0", "embedding_dim", 0),
    ("evict_strategy=7", "evict_strategy", 7),
    ("cache_weight=null", "cache_weight", None), ("inverted_cached_idx=null", "inverted_cached_idx", None),
    ("cached_idx_map=null", "cached_idx_map", None), ("workspace=null", "workspace", None),
    ("host_weight=null", "host_weight", None), ("host_weight_dev=null", "host_weight_dev", None),
    ("inverted_cached_idx+4", "inverted_cached_idx", _p(3) + 4),
    ("freq_cnter=null", "freq_cnter", None),                    # LFU without its counters
    ("workspace_bytes=16", "workspace_bytes", 16),
    ("workspace+128", "workspace", _p(6) + 128),
]


def create_cases():
    """[(label, {argument or field: bad value})]: the good configuration, every bad value alone, every two together"""
    out = [("good", {})]
    out += [(label, {what: bad}) for label, what, bad in CREATE_SINGLES]
    for (la, wa, ba), (lb, wb, bb) in itertools.combinations(CREATE_SINGLES, 2):
        if wa != wb:
            out.append((f"{la},{lb}", {wa: ba, wb: bb}))
    return out


def run_create(_lib):
    """[(label, return value, message)]; the message is None where the refusal is the first HIP call's"""
    lib, rows = _lib.lib, []
    for label, bad in create_cases():
        cfg = _lib.CeCacheConfig()
        fields = dict(_GOOD_CFG)
        fields.update({k: v for k, v in bad.items() if k not in ("cfg", "out")})
        if fields["workspace_bytes"] is None:
            fields["workspace_bytes"] = int(lib.ce_cache_workspace_bytes(N, C, MAX_IDS, D))
        for k, v in fields.items():
            setattr(cfg, k, v)
        h = ctypes.c_void_p()
        rc = lib.ce_cache_create(None if "cfg" in bad else ctypes.byref(cfg), None, None if "out" in bad else ctypes.byref(h))
        assert rc != 0, f"{label}: made-up addresses must not get as far as a cache"
        rows.append((label, int(rc), None if rc == CE_ERR_HIP else _lib.last_error()))
    return rows


# ---------------------------------------------------------------------------------------------- the other entries
STRATEGIES = ["dataset", "lfu"]


class TinyCache:
    """one cache of real arrays, made through ce_cache_create directly (the manager fixes max_ids_per_call at 2^31 - 2)"""

    def __init__(self, _lib, strategy):
        import torch
        from cachedembedding_amd.cache_mgr import HostTable
        lib = _lib.lib
        dev = torch.device("cuda", torch.cuda.current_device())
        self.table = HostTable.allocate(N, D)
        self.table.tensor.zero_()
        self.cache = torch.zeros(C, D, device=dev)
        self.inverted = torch.empty(N, dtype=torch.int32, device=dev)
        self.cached_idx_map = torch.empty(C, dtype=torch.int32, device=dev)
        self.freq = torch.empty(C, dtype=torch.int64, device=dev) if strategy == "lfu" else None
        ws_bytes = int(lib.ce_cache_workspace_bytes(N, C, MAX_IDS, D))
        self.ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=dev)
        cfg = _lib.CeCacheConfig()
        cfg.num_embeddings, cfg.cuda_row_num, cfg.embedding_dim = N, C, D
        cfg.evict_strategy = CE_EVICT_LFU if strategy == "lfu" else CE_EVICT_DATASET
        cfg.transport, cfg.protect_depth, cfg.max_ids_per_call = 0, 0, MAX_IDS
        cfg.host_weight, cfg.host_weight_dev = self.table.host_ptr, self.table.dev_ptr
        cfg.cache_weight = self.cache.data_ptr()
        cfg.idx_map = None
        cfg.inverted_cached_idx = self.inverted.data_ptr()
        cfg.cached_idx_map = self.cached_idx_map.data_ptr()
        cfg.freq_cnter = self.freq.data_ptr() if self.freq is not None else None
        cfg.workspace = (self.ws.data_ptr() + 255) & ~255
        cfg.workspace_bytes = ws_bytes
        self.handle = ctypes.c_void_p()
        _lib.check(lib.ce_cache_create(ctypes.byref(cfg), _lib.stream_ptr(), ctypes.byref(self.handle)))
        self.ids = torch.arange(MAX_IDS + 1, dtype=torch.int64, device=dev)
        self.slots = torch.empty(MAX_IDS + 1, dtype=torch.int64, device=dev)
        self.keys = torch.empty(16384, dtype=torch.int64, device=dev)
        self.rows = torch.arange(C + 1, dtype=torch.int32, device=dev)
        self.other_stream = torch.cuda.Stream(device=dev)

    def destroy(self, _lib):
        _lib.lib.ce_cache_destroy(self.handle)


def handle_cases(t, lib, stream):
    """[(label, thunk)] in the order they must run; every thunk returns the entry's return value.  `good` thunks are
    the two calls that are meant to pass (the pending call and its finish)."""
    h, ids, slots, keys, rows = t.handle, t.ids.data_ptr(), t.slots.data_ptr(), t.keys.data_ptr(), t.rows.data_ptr()
    other = t.other_stream.cuda_stream
    assert other != stream
    ms, calls, i64 = (ctypes.c_double * 8)(), ctypes.c_int64(), ctypes.c_int64()
    sec, cnt = (ctypes.c_double * 6)(), (ctypes.c_int64 * 4)()

    def window(fn, hh, nb, nnz, i=ids, s=slots, k=keys):            # the layout of one id per bag, no source keys
        return lambda: fn(hh, i, nb, nnz, s, 0, None, 0, 0, nnz, 0, 0, k, stream)

    out = []
    flat = [("ce_cache_prepare_ids", lib.ce_cache_prepare_ids), ("ce_cache_prepare_ids_padded", lib.ce_cache_prepare_ids_padded),
            ("ce_cache_prepare_ids_begin_padded", lib.ce_cache_prepare_ids_begin_padded)]
    wins = [("ce_cache_prepare_ids_keys", lib.ce_cache_prepare_ids_keys), ("ce_cache_prepare_ids_begin", lib.ce_cache_prepare_ids_begin)]
    for name, fn in flat:
        out += [(f"{name}: null handle", lambda fn=fn: fn(None, ids, 4, slots, stream)),
                (f"{name}: n=-1", lambda fn=fn: fn(h, ids, -1, slots, stream)),
                (f"{name}: n=17", lambda fn=fn: fn(h, ids, MAX_IDS + 1, slots, stream)),
                (f"{name}: null ids, n=4", lambda fn=fn: fn(h, None, 4, slots, stream)),
                (f"{name}: null slots, n=4", lambda fn=fn: fn(h, ids, 4, None, stream)),
                (f"{name}: null handle, n=17", lambda fn=fn: fn(None, ids, MAX_IDS + 1, slots, stream)),
                (f"{name}: n=17, null ids", lambda fn=fn: fn(h, None, MAX_IDS + 1, slots, stream))]
    for name, fn in wins:
        out += [(f"{name}: null handle", window(fn, None, 1, 4)),
                (f"{name}: n_batches=0", window(fn, h, 0, 4)),
                (f"{name}: nnz_per_batch=0", window(fn, h, 1, 0)),
                (f"{name}: n_batches=-1", window(fn, h, -1, 4)),
                (f"{name}: n=17", window(fn, h, 1, MAX_IDS + 1)),
                (f"{name}: n=17x1, null keys_out", window(fn, h, MAX_IDS + 1, 1, k=None)),
                (f"{name}: null ids, n=4", window(fn, h, 1, 4, i=None)),
                (f"{name}: null handle, n_batches=0", window(fn, None, 0, 4)),
                (f"{name}: n_batches=0, null keys_out", window(fn, h, 0, 4, k=None))]
    out += [("ce_cache_prepare_ids_keys: null keys_out", window(lib.ce_cache_prepare_ids_keys, h, 1, 4, k=None)),
            ("ce_cache_prepare_ids_keys: null handle, null keys_out", window(lib.ce_cache_prepare_ids_keys, None, 1, 4, k=None))]
    out += [("ce_cache_prepare_ids_finish: null handle", lambda: lib.ce_cache_prepare_ids_finish(None, stream)),
            ("ce_cache_prepare_ids_finish: nothing begun", lambda: lib.ce_cache_prepare_ids_finish(h, stream)),
            ("ce_cache_prepare_ids_finish: nothing begun, another stream", lambda: lib.ce_cache_prepare_ids_finish(h, other))]
    out += [("ce_cache_preload: null handle", lambda: lib.ce_cache_preload(None, rows, None, 4, stream)),
            ("ce_cache_preload: n=-1", lambda: lib.ce_cache_preload(h, rows, None, -1, stream)),
            ("ce_cache_preload: n=C+1", lambda: lib.ce_cache_preload(h, rows, None, C + 1, stream)),
            ("ce_cache_flush: null handle", lambda: lib.ce_cache_flush(None, stream)),
            ("ce_cache_set_transport: null handle", lambda: lib.ce_cache_set_transport(None, 0)),
            ("ce_cache_set_transport: 7", lambda: lib.ce_cache_set_transport(h, 7)),
            ("ce_cache_set_transport: -1", lambda: lib.ce_cache_set_transport(h, -1)),
            ("ce_cache_set_protect_depth: null handle", lambda: lib.ce_cache_set_protect_depth(None, 1)),
            ("ce_cache_set_protect_depth: -1", lambda: lib.ce_cache_set_protect_depth(h, -1)),
            ("ce_cache_set_protect_depth: 1024", lambda: lib.ce_cache_set_protect_depth(h, 1024)),
            ("ce_cache_set_buffer_rows: null handle", lambda: lib.ce_cache_set_buffer_rows(None, 4)),
            ("ce_cache_set_buffer_rows: -1", lambda: lib.ce_cache_set_buffer_rows(h, -1)),
            ("ce_cache_set_freq_bound: null handle", lambda: lib.ce_cache_set_freq_bound(None, 4)),
            ("ce_cache_set_freq_bound: -1", lambda: lib.ce_cache_set_freq_bound(h, -1)),
            ("ce_cache_set_deferred_rows: null handle", lambda: lib.ce_cache_set_deferred_rows(None, 1)),
            ("ce_cache_set_cache_weight: null handle", lambda: lib.ce_cache_set_cache_weight(None, t.cache.data_ptr())),
            ("ce_cache_set_cache_weight: null pointer", lambda: lib.ce_cache_set_cache_weight(h, None)),
            ("ce_cache_set_cache_weight: +4", lambda: lib.ce_cache_set_cache_weight(h, t.cache.data_ptr() + 4)),
            ("ce_cache_graph_replayed: null handle", lambda: lib.ce_cache_graph_replayed(None, 1, 4, stream)),
            ("ce_cache_graph_replayed: n_calls=-1", lambda: lib.ce_cache_graph_replayed(h, -1, 4, stream)),
            ("ce_cache_graph_replayed: ids_per_call=-1", lambda: lib.ce_cache_graph_replayed(h, 1, -1, stream)),
            ("ce_cache_graph_replayed: n_calls=257", lambda: lib.ce_cache_graph_replayed(h, 257, 4, stream)),    # kRing / 4 + 1
            ("ce_cache_lookup_slots: null handle", lambda: lib.ce_cache_lookup_slots(None, ids, 4, slots, stream)),
            ("ce_cache_lookup_slots: null ids, n=4", lambda: lib.ce_cache_lookup_slots(h, None, 4, slots, stream)),
            ("ce_cache_lookup_slots: null slots, n=4", lambda: lib.ce_cache_lookup_slots(h, ids, 4, None, stream)),
            ("ce_cache_lookup_slots: n=-1", lambda: lib.ce_cache_lookup_slots(h, ids, -1, slots, stream)),
            ("ce_cache_phase_times: null handle", lambda: lib.ce_cache_phase_times(None, ms, 8, ctypes.byref(calls), 0)),
            ("ce_cache_phase_times: null ms_out", lambda: lib.ce_cache_phase_times(h, None, 8, ctypes.byref(calls), 0)),
            ("ce_cache_phase_times: cap=5", lambda: lib.ce_cache_phase_times(h, ms, 5, ctypes.byref(calls), 0)),
            ("ce_cache_swap_stats: null handle", lambda: lib.ce_cache_swap_stats(None, sec, cnt)),
            ("ce_cache_swap_stats: null seconds", lambda: lib.ce_cache_swap_stats(h, None, cnt)),
            ("ce_cache_swap_stats: null counts", lambda: lib.ce_cache_swap_stats(h, sec, None)),
            ("ce_cache_free_rows: null handle", lambda: lib.ce_cache_free_rows(None, ctypes.byref(i64))),
            ("ce_cache_free_rows: null out", lambda: lib.ce_cache_free_rows(h, None))]
    # ---- one call begun and not finished: what refuses meanwhile
    out += [("good: ce_cache_prepare_ids_begin_padded of 4 ids", lambda: lib.ce_cache_prepare_ids_begin_padded(h, ids, 4, slots, stream))]
    for name, fn in flat:
        out += [(f"{name}: a call is pending", lambda fn=fn: fn(h, ids, 4, slots, stream)),
                (f"{name}: a call is pending, n=17", lambda fn=fn: fn(h, ids, MAX_IDS + 1, slots, stream))]
    for name, fn in wins:
        out += [(f"{name}: a call is pending", window(fn, h, 1, 4)),
                (f"{name}: a call is pending, n_batches=0", window(fn, h, 0, 4))]
    out += [("ce_cache_preload: a call is pending", lambda: lib.ce_cache_preload(h, rows, None, 4, stream)),
            ("ce_cache_preload: a call is pending, n=C+1", lambda: lib.ce_cache_preload(h, rows, None, C + 1, stream)),
            ("ce_cache_flush: a call is pending", lambda: lib.ce_cache_flush(h, stream)),
            ("ce_cache_set_transport: a call is pending", lambda: lib.ce_cache_set_transport(h, 1)),
            ("ce_cache_set_transport: a call is pending, 7", lambda: lib.ce_cache_set_transport(h, 7)),
            ("ce_cache_set_deferred_rows: a call is pending", lambda: lib.ce_cache_set_deferred_rows(h, 1)),
            ("ce_cache_prepare_ids_finish: another stream", lambda: lib.ce_cache_prepare_ids_finish(h, other)),
            ("good: ce_cache_prepare_ids_finish", lambda: lib.ce_cache_prepare_ids_finish(h, stream)),
            ("ce_cache_prepare_ids_finish: finished already", lambda: lib.ce_cache_prepare_ids_finish(h, stream))]
    return out


def run_handle(_lib, strategy):
    """[(label, return value, message)] on a fresh tiny cache; the message is None where nothing was refused"""
    import torch
    t = TinyCache(_lib, strategy)
    try:
        rows = []
        for label, thunk in handle_cases(t, _lib.lib, _lib.stream_ptr()):
            rc = int(thunk())
            assert (rc == 0) == label.startswith("good"), (label, rc, _lib.last_error())
            rows.append((label, rc, _lib.last_error() if rc else None))
        torch.cuda.synchronize()
        assert t.slots[:4].tolist() == [0, 1, 2, 3]       # the one good call ran: four rows into an empty cache
    finally:
        t.destroy(_lib)
    return rows
