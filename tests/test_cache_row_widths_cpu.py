"""The inputs of tests/test_gpu_cache_row_widths.py without a GPU (tests/cache_row_width_cases.py): the widths sit on
the side of the 64-lane boundary the GPU tests rely on, every width a layout is said to produce is what that layout's
row-bytes rule gives, and every stream meets -- on the oracle alone -- the conditions the GPU tests assert about it.
These are conditions of the inputs: a failure here is mended in the seed or the stream, not in the bar."""
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import cache_row_width_cases as cases  # noqa: E402

# width: (vec, rowlen, G, body), typed in: the restated rule must put every width where the GPU tests expect it
SHAPES = {
    24: (True, 6, 8, "register"),          # 2 of 8 lanes masked
    132: (True, 33, 64, "register"),       # 31 of 64 lanes masked
    256: (True, 64, 64, "register"),       # exactly full
    260: (True, 65, 64, "loop"),           # second pass with one live lane
    384: (True, 96, 64, "loop"),           # 1.5 passes
    512: (True, 128, 64, "loop"),          # 2 full passes
    3072: (True, 768, 64, "loop"),         # 12 passes
    66: (False, 66, 64, "loop"),           # scalar, second pass with two live lanes
}
# (layout, D) the issue's table names for each width
PRODUCERS = {24: [("adam", 8)], 132: [("q4", 1024)], 256: [("partial_rowwise_adam", 128)], 260: [("q8", 1024)],
             384: [("adam", 128)], 512: [("partial_rowwise_adam", 256), ("w16", 1024)], 3072: [("adam", 1024)], 66: []}


def test_the_table_holds_every_width_on_its_side_of_the_boundary():
    assert set(cases.WIDTHS) == set(SHAPES)
    for width, want in SHAPES.items():
        assert cases.row_shape(width) == want, width


def test_each_side_of_the_boundary_is_present_for_each_row_type():
    shapes = {w: cases.row_shape(w) for w in cases.WIDTHS}
    passes = {w: cases.passes(w) for w in cases.WIDTHS}
    vec = [w for w, s in shapes.items() if s[0]]
    scalar = [w for w, s in shapes.items() if not s[0]]
    assert any(shapes[w][1] == 64 and shapes[w][3] == "register" for w in vec)               # rowlen == G
    assert any(shapes[w][1] == 65 and passes[w] == (2, 1) for w in vec)                       # one lane past it
    assert any(shapes[w][3] == "loop" and 1 < passes[w][1] < 64 for w in vec)                 # a partial last pass
    assert any(shapes[w][3] == "loop" and passes[w][0] > 2 for w in vec)                      # more than 2 passes
    assert any(shapes[w][3] == "loop" and passes[w] == (2, 64) for w in vec)                  # whole passes only
    assert any(shapes[w][3] == "register" and shapes[w][1] < shapes[w][2] for w in vec)       # a masked register path
    assert any(shapes[w][3] == "register" and shapes[w][2] == 64 and shapes[w][1] < 64 for w in vec)
    assert any(shapes[w][3] == "loop" for w in scalar) and all(shapes[w][1] > 64 for w in scalar)
    # the rule itself at the boundary, both row types
    assert cases.row_shape(64)[1:] == (16, 16, "register") and cases.row_shape(63)[1:] == (63, 64, "register")
    assert cases.row_shape(65)[1:] == (65, 64, "loop") and cases.row_shape(1)[1:] == (1, 1, "register")


def test_every_claimed_width_is_what_the_layouts_rule_gives():
    from cachedembedding_amd import _lib
    for width, layouts in cases.WIDTHS.items():
        got = [(layout, cases.producing_dim(layout, width)) for layout in layouts]
        assert got == PRODUCERS[width], width
    # the rules, spelled out once against the library and the layouts' spans
    assert _lib.lib.ce_q8_row_bytes(1024) == 4 * 260 and _lib.lib.ce_q4_row_bytes(1024) == 4 * 132
    assert _lib.LAYOUT_SPAN["adam"] * 128 == 384 and _lib.LAYOUT_SPAN["adam"] * 1024 == 3072
    assert _lib.LAYOUT_SPAN["partial_rowwise_adam"] * 128 == 256 and _lib.LAYOUT_SPAN["partial_rowwise_adam"] * 256 == 512
    assert cases.layout_width("q8", 1040) is None and cases.layout_width("adam", 1028) is None
    for layout, D, _ in cases.LAYOUT_CASES:
        assert cases.layout_width(layout, D) in cases.WIDTHS


def test_the_strategies_take_turns_over_the_widths():
    got = {w: cases.strategy_of(w) for w in cases.WIDTHS}
    assert set(got.values()) == set(cases.STRATEGIES)
    assert {got[w] for w in (66, 260, 384, 3072)} == {"dataset", "lfu"}      # what the re-admission test crosses


def _run(stream):
    """the stream on the oracle over a one-column table: (traces, lookups per call)"""
    ora = stream.oracle(np.zeros((stream.N, 1), np.float32))
    lens = []
    for c, ids in stream.calls(ora):
        assert len(np.unique(ids)) <= stream.C, (stream.name, stream.width, c)       # no call exceeds the capacity
        ora.prepare_ids(ids)
        lens.append(len(ids))
    assert len(ora.traces) == stream.n_calls
    return ora, lens


@pytest.mark.parametrize("width", list(cases.WIDTHS))
def test_halves_stream_goes_round_the_cache_twice(width):
    s = cases.halves_stream(width)
    assert (s.N, s.C, s.n_calls) == (3001, 257, 13)
    ora, lens = _run(s)
    assert lens == [100] * 13
    assert sum(len(t.evicted_rows) for t in ora.traces) > 2 * s.C


@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("width", [66, 260, 384, 3072])
def test_readmit_stream_asks_again_for_rows_just_evicted(width, depth):
    s = cases.readmit_stream(width, depth)
    assert (s.N, s.C, s.n_calls) == (6000 if width <= 512 else 2000, 700, 24) and s.strategy in ("dataset", "lfu")
    ora = s.oracle(np.zeros((s.N, 1), np.float32))
    readmitted, prev = 0, np.zeros(0, dtype=np.int64)
    for c, ids in s.calls(ora):
        assert len(np.unique(ids)) <= s.C
        ora.prepare_ids(ids)
        readmitted += int(np.isin(ora.traces[-1].miss_rows, prev).sum())
        prev = ora.traces[-1].evicted_rows.copy()
    assert readmitted > 50


def test_big_call_stream_is_above_the_swaps_threshold_and_evicts():
    s = cases.big_call_stream()
    assert s.width == 384 and s.C == 257 and cases.row_shape(s.width)[0]
    ora, lens = _run(s)
    assert len(lens) == 4 and all(n > 131072 for n in lens)
    assert all(len(t.unique_rows) <= 200 for t in ora.traces)
    assert all(len(t.evicted_rows) > 0 for t in ora.traces[1:])


@pytest.mark.parametrize("width", [260, 384, 3072, 66])
def test_warm_stream_evicts(width):
    s = cases.warm_stream(width)
    assert (s.N, s.C, s.n_calls, s.warm) == (3000, 200, 10, 0.7)
    ora, lens = _run(s)
    assert lens == [150] * 10
    assert sum(len(t.evicted_rows) for t in ora.traces) > 0


def test_streams_are_the_same_at_every_draw():
    """the CPU test and the GPU tests draw identical streams; the table's values do not move the ids"""
    a, b = cases.readmit_stream(260, 1), cases.readmit_stream(260, 1)
    oa = a.oracle(np.zeros((a.N, 1), np.float32))
    ob = b.oracle(b.table(width=2).copy())
    for (_, x), (_, y) in zip(a.calls(oa), b.calls(ob)):
        assert np.array_equal(x, y)
        oa.prepare_ids(x)
        ob.prepare_ids(y)
    t = cases.halves_stream(24).table()
    assert t.dtype == np.float32 and t.shape == (3001, 24) and not t.flags.writeable
    assert float(np.abs(t).max()) > 3.0 and abs(float(t.mean())) < 0.05 and 0.9 < float(t.std()) < 1.1


@pytest.mark.parametrize("layout,D,strategy", cases.LAYOUT_CASES)
def test_layout_steps_revisit_rows_evicted_earlier(layout, D, strategy):
    """distinct ids within a step, and from the third step on at least a third of a step's rows had been named before and
    evicted since.  (The first two steps cannot hold such a row: the first eviction happens while the second step's
    rows are admitted, and a step's own rows are protected from it.)"""
    steps = cases.layout_steps(D)
    assert len(steps) == cases.LAYOUT_STEPS == 8 and cases.LAYOUT_C < 2 * cases.LAYOUT_B
    for ids in steps:
        assert len(ids) == cases.LAYOUT_B == len(np.unique(ids)) and ids.min() >= 0 and ids.max() < cases.LAYOUT_N
    back = cases.revisits_of_evicted_rows(steps, strategy)
    assert back[:2] == [0, 0] and all(3 * n >= cases.LAYOUT_B for n in back[2:]), back
