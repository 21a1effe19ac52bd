"""The numpy model of the presort key contract (tests/presort_ref.py) checked against itself: a key array built from the
model passes check_keys, and every single mutation a subtly wrong kernel could make is caught.  No GPU, no library."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from presort_ref import (ALL_ONES, FLAG, SEG, build_keys, check_keys, lookup_plan, model_keys, presort_len,  # noqa: E402
                         run_of)

R = 70000
N = SEG + 1000


def _slots():
    """Two segments, the second partial.  Segment 0: bucket 0 holds row 0 ten times and row 8192 seven times (17 keys:
    positions 0..9 and 10..16 of the segment); bucket 1 holds rows 1, 8193, 16385 eleven times each (33 keys: not
    sorted, no flags); bucket 2 rows 2 and 8194 sixteen times each (32 keys: sorted); three ignored slots; every other
    lookup a row of its own.  Segment 1: skewed rows."""
    rng = np.random.default_rng(5)
    head = np.concatenate([np.repeat([0, 8192], [10, 7]), np.repeat([1, 8193, 16385], 11), np.repeat([2, 8194], 16),
                           [-1, R, R + 3]])
    cand = np.arange(100, R)
    rest = rng.permutation(cand[(cand & 8191) > 2])[:SEG - head.size]         # distinct rows, none in buckets 0..2
    seg0 = rng.permutation(np.concatenate([head, rest]))
    seg1 = (rng.random(1000) ** 3 * R).astype(np.int64)
    return np.concatenate([seg0, seg1]).astype(np.int64)


@pytest.fixture(scope="module")
def case():
    slots = _slots()
    plan = lookup_plan(slots, R, None, True, N, 0)
    ids = slots + 7
    keys = build_keys(plan, N, "src_excl", rng=np.random.default_rng(1))
    ranges = np.array([[ids[:SEG].min(), ids[:SEG].max()], [ids[SEG:].min(), ids[SEG:].max()]], np.int64)
    keys.setflags(write=False)
    return slots, plan, ids, keys, ranges


def _check(case, keys, ranges=None):
    _, plan, ids, _, rg = case
    return check_keys(keys, plan, N, "src_excl", ids=ids, ranges=rg if ranges is None else ranges)


def test_a_key_array_built_from_the_model_passes(case):
    slots, plan, ids, keys, ranges = case
    assert keys.size == presort_len(N) == 2 * SEG
    st = _check(case, keys)
    assert st["segments"] == 2 and st["live"] == N - 3
    # segment 0: 16384 - 3 - 82 rows of their own, the run of row 0, and whatever bucket 2 gives; > 16000 anyway
    assert st["flags"] > 16000
    assert run_of(keys, R, 0, 0) == (0, 9, True)
    assert run_of(keys, R, 0, 8192) == (10, 16, False)              # crosses 15 | 16
    assert run_of(keys, R, 0, 2) == (50, 65, False) and run_of(keys, R, 0, 8194) == (66, 81, False)
    assert not (keys[17:50] & FLAG).any()                           # the bucket of 33
    # the same batch in the two forms without flags, and as int64 (what a torch tensor holds)
    for form in ("lookup", "src"):
        k = build_keys(plan, N, form, rng=np.random.default_rng(2))
        assert check_keys(k.view(np.int64), plan, N, form)["flags"] == 0
    # the forms are not interchangeable
    with pytest.raises(AssertionError):
        check_keys(keys, plan, N, "src")
    with pytest.raises(AssertionError):
        check_keys(build_keys(plan, N, "src"), plan, N, "src_excl")
    with pytest.raises(AssertionError):
        check_keys(build_keys(plan, N, "lookup"), plan, N, "src")


def _mut_low_word(k, case):
    k[300] ^= np.uint64(1)


def _mut_row_half(k, case):
    assert k[300] >> np.uint64(32) != k[301] >> np.uint64(32)
    k[300] = (k[301] >> np.uint64(32) << np.uint64(32)) | (k[300] & np.uint64(0xFFFFFFFF))


def _mut_swap_buckets(k, case):
    a, b = 200, 9000
    assert (k[a] >> np.uint64(32)) & np.uint64(8191) != (k[b] >> np.uint64(32)) & np.uint64(8191)
    k[a], k[b] = k[b], k[a]


def _mut_duplicate(k, case):
    k[301] = k[300]


def _mut_clear_flag(k, case):
    assert k[0] & FLAG
    k[0] &= ~FLAG


def _mut_flag_straddle(k, case):
    assert run_of(k, R, 0, 8192) == (10, 16, False)
    k[10] |= FLAG


def _mut_flag_second(k, case):
    k[1] |= FLAG


def _mut_flag_hot_bucket(k, case):
    rows = k[17:50] >> np.uint64(32)
    first = np.nonzero(np.concatenate([[True], rows[1:] != rows[:-1]]))[0]
    assert first.size > 3, "the bucket of 33 keys must hold its rows in several stretches each"
    k[17 + first[1]] |= FLAG


def _mut_flag_ignored(k, case):
    p = SEG - 3
    assert k[p] >> np.uint64(32) == np.uint64(0xFFFFFFFF) and k[p] != ALL_ONES and k[p - 1] >> np.uint64(32) < np.uint64(R)
    k[p] |= FLAG


def _mut_padding(k, case):
    assert k[-1] == ALL_ONES
    k[-1] = k[SEG] & ~FLAG


MUTATIONS = {
    "low_word_off_by_one": (_mut_low_word, "not the model's"),
    "row_half_of_the_neighbour": (_mut_row_half, "not the model's"),
    "two_buckets_swapped": (_mut_swap_buckets, "buckets"),
    "key_duplicated_over_another": (_mut_duplicate, "not the model's"),
    "flag_cleared_on_an_eligible_run": (_mut_clear_flag, "not the expected ones"),
    "flag_on_a_run_across_15_16": (_mut_flag_straddle, "crosses a 16-position block"),
    "flag_on_the_second_key_of_a_run": (_mut_flag_second, "does not head its run"),
    "flag_on_a_split_row_in_a_bucket_of_33": (_mut_flag_hot_bucket, "does not hold every key of its row"),
    "flag_on_an_ignored_key": (_mut_flag_ignored, "row is >= num_rows"),
    "live_key_in_the_padding_tail": (_mut_padding, "not the model's"),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_a_single_mutation_fails(case, name):
    mutate, message = MUTATIONS[name]
    k = case[3].copy()
    mutate(k, case)
    assert (k != case[3]).sum() in (1, 2)
    with pytest.raises(AssertionError, match=message):
        _check(case, k)


def test_ranges_max_one_too_small_fails(case):
    ranges = case[4].copy()
    ranges[1, 1] -= 1
    with pytest.raises(AssertionError, match="id range"):
        _check(case, case[3], ranges)
    # and without ids a range must say "everything"
    with pytest.raises(AssertionError, match="id range"):
        check_keys(case[3], case[1], N, "src_excl", ranges=case[4])
    everything = np.array([[np.iinfo(np.int64).min, np.iinfo(np.int64).max]] * 2)
    check_keys(case[3], case[1], N, "src_excl", ranges=everything)


def test_unsorted_small_bucket_fails(case):
    """rows of bucket 0 (17 keys) out of order: flags, multiset and buckets still right"""
    k = case[3].copy()
    k[:17] = np.concatenate([k[10:17], k[:10]])
    k[0] |= FLAG                                                    # the flags follow the runs: row 8192 at 0..6 is in one
    k[7] &= ~FLAG                                                   # block now, row 0 at 7..16 crosses 15 | 16
    with pytest.raises(AssertionError, match="rows of a bucket"):
        _check(case, k)


# ---- lookup_plan by hand ------------------------------------------------------------------------------------------------

def _plan(slots, R_, offsets, last, nb, F=0):
    p = lookup_plan(np.array(slots), R_, None if offsets is None else np.array(offsets), last, nb, F)
    return p.row.tolist(), p.bag.tolist(), p.out_row.tolist()


def test_plan_rows():
    assert _plan([0, 4, -1, 5, 8, 2 ** 40], 5, None, True, 6)[0] == [0, 4, -1, -1, -1, -1]


def test_plan_empty_bags_in_front_between_and_behind():
    # bags: [], [], [0, 1], [], [2], [3, 4, 5], [], []
    off = [0, 0, 0, 2, 2, 3, 6, 6, 6]
    row, bag, out = _plan([1] * 6, 3, off, True, 8)
    assert bag == [2, 2, 4, 5, 5, 5] and out == bag


def test_plan_without_include_last_offset():
    # the last bag ends with the lookups; an empty last bag (offsets[-1] == n) covers nothing
    assert _plan([1] * 6, 3, [0, 2, 2, 5], False, 4)[1] == [0, 0, 2, 2, 2, 3]
    assert _plan([1] * 6, 3, [0, 2, 6], False, 3)[1] == [0, 0, 1, 1, 1, 1]


def test_plan_hook_features():
    # F = 2 features, B = 3 samples, bag g = f * B + b -> out_row b * F + f
    row, bag, out = _plan([0] * 6, 1, None, True, 6, 2)
    assert bag == [0, 1, 2, 3, 4, 5] and out == [0, 2, 4, 1, 3, 5]
    # ragged: bags of 2, 0, 1, 1, 3, 0 lookups
    row, bag, out = _plan([0] * 7, 1, [0, 2, 2, 3, 4, 7, 7], True, 6, 2)
    assert bag == [0, 0, 2, 3, 4, 4, 4] and out == [0, 0, 4, 1, 3, 3, 3]


def test_plan_first_offset_3():
    row, bag, out = _plan([1] * 8, 3, [3, 5, 8], True, 2)
    assert bag == [-1, -1, -1, 0, 0, 1, 1, 1] and out == bag
    assert _plan([1] * 8, 3, [3, 5], False, 2)[1] == [-1, -1, -1, 0, 0, 1, 1, 1]
    # with the hook fold the uncovered lookups stay -1
    assert _plan([1] * 8, 3, [3, 5, 8], True, 2, 2)[2] == [-1, -1, -1, 0, 0, 1, 1, 1]


def test_plan_last_offset_nnz_minus_2():
    n = 9
    row, bag, out = _plan([1] * n, 3, [0, 4, n - 2], True, 2)
    assert bag == [0, 0, 0, 0, 1, 1, 1, -1, -1]
    # ... also behind a trailing empty bag
    assert _plan([1] * n, 3, [0, 4, n - 2, n - 2], True, 3)[1] == [0, 0, 0, 0, 1, 1, 1, -1, -1]


def test_uncovered_lookups_in_the_key_forms():
    """source-row forms: all ones, like padding; the lookup form knows no bags"""
    plan = lookup_plan(np.array([4, 5, -1, 6, 7, 8, 9]), 100, np.array([2, 3, 5]), True, 2, 0)
    assert plan.bag.tolist() == [-1, -1, 0, 1, 1, -1, -1]
    src = model_keys(plan, 7, "src")
    assert (src[[0, 1, 5, 6]] == ALL_ONES).all()
    assert src[2] == np.uint64(0xFFFFFFFF << 32 | 0) and src[3] == np.uint64(6 << 32 | 1) and src[4] == np.uint64(7 << 32 | 1)
    lk = model_keys(plan, 7, "lookup")
    assert lk.tolist() == [4 << 32 | 0, 5 << 32 | 1, int(ALL_ONES), 6 << 32 | 3, 7 << 32 | 4, 8 << 32 | 5, 9 << 32 | 6]
    for form in ("lookup", "src", "src_excl"):
        check_keys(build_keys(plan, 7, form), plan, 7, form)
