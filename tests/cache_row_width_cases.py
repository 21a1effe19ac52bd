"""Shared inputs of the row-width tests of the cache op (test infrastructure): the widths under test, the lane-group
rule that decides which body of a row mover runs at a width, which table layout produces each width, and the seeded id
streams.  tests/test_cache_row_widths_cpu.py checks the inputs against the oracle alone; tests/test_gpu_cache_row_widths.py
runs them through the library.  Both draw the same streams: the ids come from a generator seeded by (stream, width)
that the table's values never touch.

A width is the row length in fp32 elements that the cache op is driven with (CeCacheConfig.embedding_dim): 3 * D for an
Adam-layout table, 2 * D for partial row-wise Adam, (16 + D) / 4 for q8, (16 + D / 2) / 4 for q4, D / 2 for a 16-bit
table."""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

from lru_ref import LruOracleCachedParamMgr  # noqa: E402
from oracle.cache_oracle import DATASET, LFU, OracleCachedParamMgr  # noqa: E402

# width -> the layouts that produce it (at the D producing_dim() derives); 66 is produced by none: it is the scalar row
# (66 % 4 != 0) just past the 64-lane group
WIDTHS = {
    24: ("adam",),
    132: ("q4",),
    256: ("partial_rowwise_adam",),
    260: ("q8",),
    384: ("adam",),
    512: ("partial_rowwise_adam", "w16"),
    3072: ("adam",),
    66: (),
}

STRATEGIES = ("dataset", "lfu", "lru")


def strategy_of(width):
    """DATASET / LFU / LRU in turn over WIDTHS: the strategy picks victims, it moves no rows"""
    return STRATEGIES[list(WIDTHS).index(width) % 3]


def row_shape(width):
    """(vec, rowlen, G, body) as ce_cache_create derives them for 16-byte aligned tables: rows of whole 16-byte vectors
    when width % 4 == 0, of floats otherwise; a group of G = min(64, next power of two >= rowlen) lanes per row; the
    movers take their register path when one pass of the group covers the row, their copy_row loop otherwise"""
    vec = width % 4 == 0
    rowlen = width // 4 if vec else width
    g = 1
    while g < rowlen and g < 64:
        g <<= 1
    return vec, rowlen, g, "register" if rowlen <= g else "loop"


def passes(width):
    """passes of the lane group over a row, and the live lanes of the last one"""
    _, rowlen, g, _ = row_shape(width)
    n = -(-rowlen // g)
    return n, rowlen - (n - 1) * g


def layout_width(layout, dim):
    """fp32 elements per row of `layout` at embedding_dim `dim` by the layout's own rule, or None where the layout
    refuses the dim"""
    from cachedembedding_amd import _lib
    try:
        if layout in ("adam", "partial_rowwise_adam"):
            _lib.check_adam_dim(dim)
            return _lib.LAYOUT_SPAN[layout] * dim
        if layout == "w16":
            _lib.check_w16_dim(dim)
            return dim // 2
    except NotImplementedError:
        return None
    if layout in ("q8", "q4"):
        nbytes = (_lib.lib.ce_q8_row_bytes if layout == "q8" else _lib.lib.ce_q4_row_bytes)(dim)
        return nbytes // 4 if nbytes and nbytes % 4 == 0 else None
    raise ValueError(layout)


def producing_dim(layout, width):
    """the one embedding_dim at which `layout` has rows of `width` fp32 elements"""
    dims = [d for d in range(1, 1025) if layout_width(layout, d) == width]
    assert len(dims) == 1, (layout, width, dims)
    return dims[0]


def make_oracle(strategy, weight, C):
    if strategy == "lru":
        return LruOracleCachedParamMgr(weight, C)
    return OracleCachedParamMgr(weight, C, LFU if strategy == "lfu" else DATASET)


_TABLES = {}


class Stream:
    """A seeded stream of cache-op calls at one width.  table() is the host table; calls(ora) yields (c, ids) and
    expects the caller to have run ora.prepare_ids(ids) before it asks for the next call (readmit_stream reads the
    oracle's last trace).  bump() is the training step stand-in between calls."""

    def __init__(self, name, width, N, C, n_calls, warm, draw, depth=0, strategy=None):
        self.name, self.width, self.N, self.C, self.n_calls, self.warm = name, width, N, C, n_calls, warm
        self.depth = depth
        self.strategy = strategy or strategy_of(width)
        self._draw = draw
        self._tag = {"halves": 1, "readmit": 2, "big_call": 3, "warm": 4}[name]

    def table(self, width=None):
        """standard-normal fp32 [N, width], drawn once per (stream, width) and handed out read-only: callers copy"""
        key = (self._tag, self.width, self.N, self.width if width is None else width)
        if key not in _TABLES:
            rng = np.random.default_rng([self.width, self._tag, 0])
            _TABLES[key] = rng.standard_normal(key[2:], dtype=np.float32)
            _TABLES[key].setflags(write=False)
        return _TABLES[key]

    def oracle(self, weight):
        ora = make_oracle(self.strategy, weight, self.C)
        ora.protect_depth = self.depth
        ora.reorder(None, self.warm)
        return ora

    def calls(self, ora):
        rng = np.random.default_rng([self.width, self._tag, 1, self.depth])
        for c in range(self.n_calls):
            yield c, self._draw(rng, c, ora)

    @staticmethod
    def bump(c):
        """what every row of call c's slots gains on both sides: a payload the host table has never held"""
        return np.float32(0.25 * (c + 1))


def halves_stream(width):
    """13 calls of 100 ids over N = 3001, C = 257, cold cache: 3 calls fill it, 10 go round it twice more"""
    N = 3001
    return Stream("halves", width, N, 257, 13, 0.0, lambda rng, c, ora: rng.integers(0, N, size=100))


def readmit_stream(width, depth):
    """24 calls over N = 6000, C = 700, full cache: 300 fresh ids (150 when the previous call is protected: both calls'
    rows must fit) plus half of the rows the previous call evicted, a third of those twice.  At width 3072 the table
    has 2000 rows: what a case costs there is copying and comparing the host table (74 MB at N = 6000, several times
    over), and the rows outside the cache's reach add nothing to what the movers are asked to do."""
    N, per_call = (6000 if width <= 512 else 2000), 300 // (2 if depth else 1)

    def draw(rng, c, ora):
        prev = ora.traces[-1].evicted_rows if ora.traces else np.zeros(0, dtype=np.int64)      # no frequency map: row == id
        fresh = rng.integers(0, N, size=per_call)
        again = prev[rng.permutation(len(prev))[: len(prev) // 2]]
        ids = np.concatenate([fresh, again, again[: len(again) // 3]])
        rng.shuffle(ids)
        return ids

    return Stream("readmit", width, N, 700, 24, 1.0, draw, depth=depth)


BIG_CALL_LOOKUPS = 140_000          # > 131072: the zero-copy swap of a vector row takes its 16-rows-in-flight form


def big_call_stream():
    """width 384: 4 calls of 140 000 lookups over at most 200 distinct rows each, N = 3001, C = 257"""
    N = 3001

    def draw(rng, c, ora):
        rows = rng.choice(N, 200, replace=False)
        return rows[rng.integers(0, 200, size=BIG_CALL_LOOKUPS)]

    return Stream("big_call", 384, N, 257, 4, 0.0, draw)


def warm_stream(width):
    """10 calls of 150 ids over N = 3000, C = 200 after a 70 % preload"""
    N = 3000
    return Stream("warm", width, N, 200, 10, 0.7, lambda rng, c, ora: rng.integers(0, N, size=150))


# ---- the layouts through an evicting cache ------------------------------------------------------------------------------

LAYOUT_N, LAYOUT_B, LAYOUT_C, LAYOUT_STEPS = 400, 48, 56, 8
# (layout, D, strategy): the widths 384, 3072, 256 and 512
LAYOUT_CASES = [("adam", 128, "dataset"), ("adam", 1024, "lfu"),
                ("partial_rowwise_adam", 128, "lfu"), ("partial_rowwise_adam", 256, "dataset")]


def layout_steps(seed):
    """8 steps of 48 DISTINCT ids over N = 400: from the third step on, half of a step's ids are ids of the step before
    the last -- which a 56-row cache had to evict to make room for the last step's -- and the rest are new to both
    neighbours"""
    rng = np.random.default_rng([seed, 5])
    steps = []
    for k in range(LAYOUT_STEPS):
        old = rng.choice(steps[k - 2], LAYOUT_B // 2, replace=False) if k >= 2 else np.zeros(0, dtype=np.int64)
        taken = np.concatenate([old] + steps[max(0, k - 2):k])
        pool = np.setdiff1d(np.arange(LAYOUT_N), taken)
        ids = np.concatenate([old, rng.choice(pool, LAYOUT_B - len(old), replace=False)]).astype(np.int64)
        steps.append(ids[rng.permutation(LAYOUT_B)])
    return steps


def revisits_of_evicted_rows(steps, strategy, C=LAYOUT_C, warm=0.7):
    """per step: how many of its rows an earlier step had named AND the cache has evicted since (they miss now although
    an earlier call had made them resident) -- from the ids alone, on the oracle over a table of one column"""
    ora = make_oracle(strategy, np.zeros((LAYOUT_N, 1), np.float32), C)
    ora.reorder(None, warm)
    seen = np.zeros(LAYOUT_N, bool)
    out = []
    for ids in steps:
        ora.prepare_ids(ids)
        out.append(int(seen[ora.traces[-1].miss_rows].sum()))
        seen[ids] = True
    return out
