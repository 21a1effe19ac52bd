"""CPU test of which C entry the backward of embedding_bag calls and what it hands it: every case of
tests/golden/update_dispatch.json (recorded by tests/golden/record_update_dispatch.py from the commit the file names,
before the backward planned its call in one function) is replayed through `_BagFn.backward` of this checkout with the
library replaced by a stand-in -- no GPU, no kernel -- and must give the same entry, the same argument list position by
position and the same allocated workspaces."""
import json
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE), str(HERE / "golden")]
import update_dispatch_cases as dc  # noqa: E402

FIXTURE = json.loads((HERE / "golden" / "update_dispatch.json").read_text())
RECORDS = dc.unpack(FIXTURE["entries"])


def test_fixture_is_whole():
    from record_update_dispatch import ENTRIES, MAX_BYTES
    assert len(RECORDS) == FIXTURE["cases"] and len({r[0] for r in RECORDS}) == len(RECORDS)
    assert set(FIXTURE["entries"]) == set(ENTRIES) and len(ENTRIES) == 37
    assert FIXTURE["shape"] == dict(rows=dc.ROWS, dim=dc.DIM, bags=dc.BAGS, nnz=dc.NNZ)
    assert (HERE / "golden" / "update_dispatch.json").stat().st_size < MAX_BYTES
    assert {r[0].optimizer for r in RECORDS} == set(FIXTURE["recorded_from"])


@pytest.mark.parametrize("entry", sorted(FIXTURE["entries"]))
def test_backward_calls_the_recorded_entry_with_the_recorded_arguments(entry):
    from cachedembedding_amd import functional as F
    wrong = []
    with dc.patched(F) as rec:
        for case, want_entry, want_args, want_allocated in RECORDS:
            if want_entry != entry:
                continue
            got = dc.run(case, F, rec)
            if got != (want_entry, want_args, want_allocated):
                wrong.append((case, (want_entry, want_args, want_allocated), got))
    for case, want, got in wrong[:5]:
        print(case)
        print("  recorded:", *want)
        print("  got:     ", *(got or ("refused before the forward",)))
        if got and len(got[1]) == len(want[1]):
            print("  differing positions:", [i for i, (g, w) in enumerate(zip(got[1], want[1])) if g != w])
    assert not wrong, f"{len(wrong)} of the cases of {entry} differ (the first five are printed)"


def test_every_admitted_case_is_in_the_fixture():
    """the generator has not drifted from the fixture: what base_cases() yields and the checks admit is recorded"""
    from cachedembedding_amd import functional as F
    recorded = {r[0] for r in RECORDS}
    with dc.patched(F):
        admitted = {c for c in dc.base_cases() if dc.build(c, F) is not None}
    assert admitted == {c for c in recorded if not c.variant}
