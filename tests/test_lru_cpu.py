"""LRU eviction without a GPU: the reference model of tests/lru_ref.py against a hand-checked script, against an
independent OrderedDict LRU, and against the strategy's invariants on seeded streams; and what ce_cache_create answers
to the new strategy code on made-up addresses (as tests/cache_refusal_cases.py does it)."""
import ctypes
import re
import sys
from collections import OrderedDict
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import cache_refusal_cases as cc  # noqa: E402
from lru_ref import LruOracleCachedParamMgr  # noqa: E402
from oracle.cache_oracle import id_freq_map, power_law_ids  # noqa: E402

SCRIPT = [[0, 1, 2], [3], [0, 1], [2], [3], [0], [1]]
SCRIPT_HITS = [0, 0, 2, 0, 0, 1, 0]
SCRIPT_EVICTED = [[], [2], [], [3], [1], [], [2]]       # the second [3] evicts row 1, not row 0: the tie rule


def test_hand_checked_script():
    m = LruOracleCachedParamMgr(np.arange(24, dtype=np.float32).reshape(6, 4), 3)
    for ids in SCRIPT:
        m.prepare_ids(np.array(ids))
    assert m.num_hits_history == SCRIPT_HITS
    assert [t.evicted_rows.tolist() for t in m.traces] == SCRIPT_EVICTED


@pytest.mark.parametrize("N,C,calls,seed", [(40, 7, 400, 0), (300, 32, 1500, 1)])
def test_single_id_calls_equal_an_ordered_dict_lru(N, C, calls, seed):
    """one id per call: no two slots share a last use, so the tie rule never applies and the evictions are those of a
    textbook LRU"""
    rng = np.random.default_rng(seed)
    m = LruOracleCachedParamMgr(rng.standard_normal((N, 2)).astype(np.float32), C)
    lru = OrderedDict()
    for i in power_law_ids(rng, N, calls, 0.6):
        i = int(i)
        evicted = []
        if i in lru:
            lru.move_to_end(i)
        else:
            if len(lru) == C:
                evicted = [lru.popitem(last=False)[0]]
            lru[i] = True
        m.prepare_ids(np.array([i]))
        assert m.traces[-1].evicted_rows.tolist() == evicted
        assert set(m.cached_idx_map[m.cached_idx_map >= 0].tolist()) == set(lru)


@pytest.mark.parametrize("N,C,n_ids,s,depth,warm", [(2000, 100, 60, 0.25, 0, True), (2000, 100, 30, 0.6, 2, True),
                                                   (500, 64, 40, 1.05, 1, False)])
def test_victim_invariants_on_seeded_streams(N, C, n_ids, s, depth, warm):
    rng = np.random.default_rng(N + C + depth)
    perm = rng.permutation(N)
    m = LruOracleCachedParamMgr(rng.standard_normal((N, 2)).astype(np.float32), C)
    m.protect_depth = depth
    m.reorder(id_freq_map(perm[power_law_ids(rng, N, 20000, s)], N) if warm else None, 0.7)
    evictions = 0
    for _ in range(60):
        ids = perm[power_law_ids(rng, N, n_ids, s)]
        before_map, before_use = m.cached_idx_map.copy(), m.last_use.copy()
        protected = np.unique(np.concatenate([ids] + m._protect_history[-depth:] if depth else [ids]))
        eligible = (before_map >= 0) & ~np.isin(before_map, protected)
        m.prepare_ids(ids)
        vic = m.traces[-1].evicted_slots
        evictions += len(vic)
        assert eligible[vic].all(), "a victim was empty or protected"
        rest = eligible.copy()
        rest[vic] = False
        if len(vic) and rest.any():
            assert before_use[rest].min() >= before_use[vic].max(), "an eligible slot older than a victim was kept"
            # ... and among equal last uses the higher slot went first
            edge = before_use[vic].max()
            kept_at_edge = np.nonzero(rest & (before_use == edge))[0]
            gone_at_edge = vic[before_use[vic] == edge]
            if len(kept_at_edge):
                assert kept_at_edge.max() < gone_at_edge.min()
    assert evictions > 0


def test_failed_call_flag():
    """a failed call changes nothing; whether it is a use of the resident rows it named is the flag"""
    for flag, evicted in ((True, 1), (False, 0)):
        m = LruOracleCachedParamMgr(np.zeros((6, 2), dtype=np.float32), 2, failed_call_is_use=flag)
        m.prepare_ids(np.array([0]))
        m.prepare_ids(np.array([1]))
        with pytest.raises(IndexError):
            m.prepare_ids(np.array([0, 6]))           # names row 0, then fails
        with pytest.raises(AssertionError):
            m.prepare_ids(np.array([2, 3, 4]))        # more unique rows than slots: names nothing resident
        assert m.cached_idx_map.tolist() == [0, 1]
        m.prepare_ids(np.array([5]))
        assert m.traces[-1].evicted_rows.tolist() == [evicted]


# ------------------------------------------------------------------------------------------------ ABI
def _create(_lib, **fields):
    lib = _lib.lib
    cfg = _lib.CeCacheConfig()
    f = dict(cc._GOOD_CFG)
    f.update(fields)
    if f["workspace_bytes"] is None:
        f["workspace_bytes"] = int(lib.ce_cache_workspace_bytes(cc.N, cc.C, cc.MAX_IDS, cc.D))
    for k, v in f.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    rc = lib.ce_cache_create(ctypes.byref(cfg), None, ctypes.byref(h))
    return int(rc), _lib.last_error()


def test_create_accepts_the_lru_code_and_still_refuses_the_others():
    if torch.cuda.is_available():
        pytest.skip("passes made-up addresses: only for machines without a GPU")
    from cachedembedding_amd import _lib
    # LRU without counters passes every check and reaches the first HIP call, which fails where there is no GPU
    assert _create(_lib, evict_strategy=_lib.CE_EVICT_LRU, freq_cnter=None)[0] == _lib.CE_ERR_HIP
    assert _create(_lib, evict_strategy=_lib.CE_EVICT_LRU)[0] == _lib.CE_ERR_HIP
    for code in (3, 7, -1):
        assert _create(_lib, evict_strategy=code) == (_lib.CE_ERR_INVALID, "unknown eviction strategy")
    assert _create(_lib, evict_strategy=_lib.CE_EVICT_LFU, freq_cnter=None) == (_lib.CE_ERR_INVALID, "LFU needs freq_cnter")
    # the order of the checks is unchanged: the strategy is looked at before the arrays, the counters after them
    assert _create(_lib, evict_strategy=3, cache_weight=None)[1] == "unknown eviction strategy"
    assert _create(_lib, evict_strategy=_lib.CE_EVICT_LRU, cache_weight=None)[1] == "null device array"
    assert _create(_lib, evict_strategy=_lib.CE_EVICT_LRU, freq_cnter=None, host_weight=None)[1] == "null host table"


def test_strategy_codes_agree_with_the_header():
    """The library's code for LRU is 2 in the header and in the mirror.  The Python enum keeps upstream's VALUES for its
    first two members (LFU = 1, DATASET = 2: not the library's codes), so LRU cannot have the value 2 there without
    becoming an alias of DATASET; what has to hold is that it is a member of its own and that the manager hands the
    library the header's code for it."""
    from cachedembedding_amd import _lib
    from cachedembedding_amd.cache_mgr import EVICT_CODES, EvictionStrategy
    header = (HERE.parent / "include" / "ce_api.h").read_text()
    codes = {n: int(v) for n, v in re.findall(r"#define (CE_EVICT_[A-Z]+) (\d+)", header)}
    assert codes == {"CE_EVICT_DATASET": 0, "CE_EVICT_LFU": 1, "CE_EVICT_LRU": 2}
    assert _lib.CE_EVICT_LRU == codes["CE_EVICT_LRU"] == 2
    assert len({EvictionStrategy.DATASET, EvictionStrategy.LFU, EvictionStrategy.LRU}) == 3
    assert EvictionStrategy.LRU is not EvictionStrategy.DATASET and EvictionStrategy(2) is EvictionStrategy.DATASET
    assert EVICT_CODES == {EvictionStrategy.DATASET: 0, EvictionStrategy.LFU: 1, EvictionStrategy.LRU: 2}


def test_fused_sparse_modules_refuses_two_strategies():
    from cachedembedding_amd.cache_mgr import EvictionStrategy
    from cachedembedding_amd.modules import FusedSparseModules
    with pytest.raises(ValueError, match="not both"):
        FusedSparseModules([10, 20], 8, use_cache=True, use_lfu_eviction=True, evict_strategy=EvictionStrategy.LRU)
