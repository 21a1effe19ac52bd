"""A plain numpy model of the window presort's key contract (k_bag_presort_seg; include/ce_api.h).

Two statements, independent of every kernel:

  lookup_plan   which cache row, which bag and which row of grad_out / of the output lookup j of one batch stands for;
  check_keys    what a key array written for that batch must look like, segment by segment.

Numpy only (argsort, bincount, searchsorted, unique); nothing here imports torch or the library.

Key forms (a key is a uint64: high word = row, low word below):
  "lookup"    row << 32 | lookup-in-segment; an ignored lookup (slot outside [0, num_rows)) is all ones
  "src"       row << 32 | out_row;           an ignored lookup is 0xffffffff << 32 | out_row
  "src_excl"  "src" plus bit 31 of the low word on the heads of owner-exclusive runs
In the two source-row forms a lookup that no bag covers is all ones, like the padding behind the batch: it has no
output row.  The "lookup" form knows no bags, so coverage does not show in it.
"""
from typing import NamedTuple, Optional

import numpy as np

SEG = 16384                      # positions per segment
BLOCK = 16                       # a flagged run lies inside one block of this many positions
FLAG = np.uint64(0x80000000)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
ROW_IGNORED = np.uint64(0xFFFFFFFF)
FORMS = ("lookup", "src", "src_excl")
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


class Plan(NamedTuple):
    """per lookup of one batch; -1 = ignored (row) / uncovered (bag, out_row)"""
    row: np.ndarray
    bag: np.ndarray
    out_row: np.ndarray
    num_rows: int


def lookup_plan(slots, num_rows: int, offsets, include_last_offset: bool, num_bags: int, hook_features: int) -> Plan:
    """Which gradient row does lookup j read, and which cache row does it add to?

    row      slots[j], or -1 when it lies outside [0, num_rows);
    bag      the b with offsets[b] <= j < end(b), end(b) = offsets[b + 1], or the number of lookups for the last bag
             without include_last_offset; -1 when there is none (j < offsets[0], or j >= end(last bag)).
             offsets=None: one id per bag, bag = j;
    out_row  the bag, or b * F + f for bag g = f * B + b (B = num_bags / F) under hook_features = F; -1 when uncovered."""
    slots = np.asarray(slots, np.int64).reshape(-1)
    n = slots.size
    row = np.where((slots >= 0) & (slots < num_rows), slots, -1)
    j = np.arange(n, dtype=np.int64)
    if offsets is None:
        assert num_bags == n, "offsets=None states one id per bag"
        bag = j.copy()
    else:
        off = np.asarray(offsets, np.int64).reshape(-1)
        assert off.size == num_bags + (1 if include_last_offset else 0)
        starts = off[:num_bags]
        ends = off[1:num_bags + 1] if include_last_offset else np.concatenate([off[1:num_bags], [n]])
        assert (np.diff(starts) >= 0).all() and (ends >= starts).all(), "offsets must not decrease"
        b = np.searchsorted(starts, j, side="right") - 1            # last b with offsets[b] <= j
        bc = np.clip(b, 0, num_bags - 1)
        bag = np.where((b >= 0) & (j < ends[bc]), bc, -1)
    if hook_features:
        assert num_bags % hook_features == 0
        B = num_bags // hook_features
        out_row = np.where(bag >= 0, (bag % B) * hook_features + bag // B, -1)
    else:
        out_row = bag.copy()
    return Plan(row, bag, out_row, int(num_rows))


def presort_len(n: int) -> int:
    return -(-int(n) // SEG) * SEG


def model_keys(plan: Plan, n: int, form: str) -> np.ndarray:
    """the key of every lookup, in lookup order (no flags)"""
    assert form in FORMS and plan.row.size == n
    live = plan.row >= 0
    hi = np.where(live, plan.row, 0xFFFFFFFF).astype(np.uint64) << np.uint64(32)
    if form == "lookup":
        low = (np.arange(n, dtype=np.int64) % SEG).astype(np.uint64)
        return np.where(live, hi | low, ALL_ONES)
    covered = plan.out_row >= 0
    low = np.where(covered, plan.out_row, 0).astype(np.uint64)
    return np.where(covered, hi | low, ALL_ONES)


def _runs(rows: np.ndarray):
    """maximal stretches of equal rows: (first position, last position, row) of each"""
    if rows.size == 0:
        z = np.zeros(0, np.int64)
        return z, z, rows[:0]
    first = np.nonzero(np.concatenate([[True], rows[1:] != rows[:-1]]))[0]
    last = np.concatenate([first[1:], [rows.size]]) - 1
    return first, last, rows[first]


def _expected_flags(rows: np.ndarray, buckets: int, excl_run: int) -> np.ndarray:
    """positions (in a segment's live prefix) that carry the owner-exclusive flag: the head of every run that lies
    inside one 16-position block and whose bucket holds at most excl_run keys"""
    first, last, rrow = _runs(rows)
    per_bucket = np.bincount((rows & np.uint64(buckets - 1)).astype(np.int64), minlength=buckets)
    small = per_bucket[(rrow & np.uint64(buckets - 1)).astype(np.int64)] <= excl_run
    return first[small & (first // BLOCK == last // BLOCK)]


def build_keys(plan: Plan, n: int, form: str, *, buckets: int = 8192, excl_run: int = 32, rng=None) -> np.ndarray:
    """A key array that keeps the contract, built from the model alone: the live keys of a segment grouped by bucket
    (row & (buckets - 1)), inside a bucket in any order -- or, for "src_excl" and a bucket of at most excl_run keys,
    by row with any order inside a run -- then the ignored keys, then all ones."""
    per = model_keys(plan, n, form)
    rng = rng or np.random.default_rng(0)
    out = np.full(presort_len(n), ALL_ONES, np.uint64)
    for s0 in range(0, n, SEG):
        k = rng.permutation(per[s0:min(n, s0 + SEG)])
        live = (k >> np.uint64(32)) < np.uint64(plan.num_rows)
        lk = k[live]
        r = lk >> np.uint64(32)
        b = (r & np.uint64(buckets - 1)).astype(np.int64)
        if form == "src_excl":
            small = np.bincount(b, minlength=buckets)[b] <= excl_run
            lk = lk[np.lexsort((np.where(small, r, 0), b))]
            lk[_expected_flags(lk >> np.uint64(32), buckets, excl_run)] |= FLAG
        else:
            lk = lk[np.argsort(b, kind="stable")]
        rest = np.sort(k[~live])                                    # ignored keys in front of the all-ones ones
        out[s0:s0 + lk.size] = lk
        out[s0 + lk.size:s0 + k.size] = rest
    return out


def run_of(keys: np.ndarray, num_rows: int, seg: int, row: int):
    """(first position, last position, flagged) of the stretch of `row` in segment `seg`, positions counted inside the
    segment; the row must form ONE stretch there"""
    k = np.asarray(keys).view(np.uint64)[seg * SEG:(seg + 1) * SEG]
    at = np.nonzero((k >> np.uint64(32)) == np.uint64(row))[0]
    assert at.size and at[-1] - at[0] + 1 == at.size, f"row {row} is not one stretch of segment {seg}"
    return int(at[0]), int(at[-1]), bool(k[at[0]] & FLAG)


def _need(cond, seg, what, detail=None):
    if not cond:
        raise AssertionError(f"segment {seg}: {what}" + ("" if detail is None else f" ({detail})"))


def check_keys(keys, plan: Plan, n: int, form: str, *, ids=None, ranges=None, buckets: int = 8192,
               excl_run: int = 32) -> dict:
    """Assert that `keys` (the presort_len(n) keys of ONE batch, any integer dtype of 8 bytes) keep the contract for the
    batch `plan` describes; see the module docstring and include/ce_api.h.  buckets / excl_run are the documented
    constants of the grouping (CE_SEG_BUCKETS, "<= 32 keys"); the flag-safety checks do not use them.
    ids (the n ids the slots were computed from) with ranges ([segments, 2]): ranges[s] is exactly [min, max] of the
    ids of segment s, ignored lookups included; ranges without ids: every range says "everything".
    Returns counts: {"flags": flagged keys, "live": keys with a row < num_rows, "segments": ...}."""
    assert form in FORMS
    k_all = np.ascontiguousarray(keys).reshape(-1).view(np.uint64)
    assert k_all.size == presort_len(n), f"{k_all.size} keys for {n} lookups"
    want_all = model_keys(plan, n, form)
    R = np.uint64(plan.num_rows)
    mask = np.uint64(buckets - 1)
    n_flags = n_live = 0
    for seg, s0 in enumerate(range(0, k_all.size, SEG)):
        k = k_all[s0:s0 + SEG]
        n_here = min(SEG, n - s0)
        hi = k >> np.uint64(32)
        flagged = ((k & FLAG) != 0) & (k != ALL_ONES)
        # ---- the multiset, flags cleared; what lies beyond the batch is all ones
        want = np.concatenate([want_all[s0:s0 + n_here], np.full(SEG - n_here, ALL_ONES, np.uint64)])
        got = np.sort(np.where(flagged, k & ~FLAG, k))
        want.sort()
        bad = np.nonzero(got != want)[0]
        _need(bad.size == 0, seg, "the keys are not the model's",
              None if bad.size == 0 else f"{bad.size} differ, first: got {int(got[bad[0]]):#x} want {int(want[bad[0]]):#x}")
        # ---- live keys first
        live = hi < R
        nl = int(live.sum())
        _need(live[:nl].all(), seg, "a key with a row >= num_rows stands in front of a live key")
        _need(not flagged[nl:].any(), seg, "a flag on a key whose row is >= num_rows",
              np.nonzero(flagged[nl:])[0][:4] + nl)
        if form == "lookup":
            _need((k[nl:] == ALL_ONES).all(), seg, "an ignored lookup must be all ones in the lookup form")
        rows = hi[:nl]
        # ---- grouping
        bkt = (rows & mask).astype(np.int64)
        _need((np.diff(bkt) >= 0).all(), seg, "buckets (row & (buckets - 1)) are not in non-decreasing order")
        if form == "src_excl":
            small = np.bincount(bkt, minlength=buckets)[bkt] <= excl_run
            inside = small[1:] & (bkt[1:] == bkt[:-1])
            _need((rows[1:][inside] >= rows[:-1][inside]).all(), seg,
                  f"the rows of a bucket of <= {excl_run} keys are not in non-decreasing order")
        # ---- flag safety: nothing here uses `buckets`
        first, last, rrow = _runs(rows)
        fl = np.nonzero(flagged[:nl])[0]
        head = np.zeros(nl, bool)
        head[first] = True
        _need(head[fl].all(), seg, "a flagged key does not head its run", fl[~head[fl]][:4])
        urow, ucnt = np.unique(rows, return_counts=True)
        complete = (last - first + 1) == ucnt[np.searchsorted(urow, rrow)]
        fr = np.searchsorted(first, fl)                             # the run every flagged head starts
        _need(complete[fr].all(), seg, "a flagged run does not hold every key of its row in the segment",
              fl[~complete[fr]][:4])
        one_block = first // BLOCK == last // BLOCK
        _need(one_block[fr].all(), seg, "a flagged run crosses a 16-position block", fl[~one_block[fr]][:4])
        # ---- flag liveness: the exact set
        expect = _expected_flags(rows, buckets, excl_run) if form == "src_excl" else np.zeros(0, np.int64)
        _need(np.array_equal(fl, expect), seg, "the flagged positions are not the expected ones",
              (np.setdiff1d(expect, fl)[:4], np.setdiff1d(fl, expect)[:4]))
        n_flags += fl.size
        n_live += nl
        # ---- the id range
        if ranges is not None:
            r = np.asarray(ranges).reshape(-1, 2)[seg]
            if ids is None:
                exp = (I64_MIN, I64_MAX)
            else:
                seg_ids = np.asarray(ids, np.int64).reshape(-1)[s0:s0 + n_here]
                exp = (int(seg_ids.min()), int(seg_ids.max()))
            _need((int(r[0]), int(r[1])) == exp, seg, "the id range is not [min, max] of the segment's ids", (r, exp))
    return {"flags": int(n_flags), "live": int(n_live), "segments": k_all.size // SEG}
