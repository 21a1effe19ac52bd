"""What the handle-based entries of ce_cache.hip refuse, with which code and message: the calls of
tests/cache_refusal_cases.py (a null handle, n = -1 and n = 17 on a cache of max_ids_per_call = 16, null ids, a window
shape with a 0, null keys_out, _finish with nothing begun or on another stream, every entry that refuses while a call
is pending, an unknown transport, bad depths / bounds / counts, a misaligned cache_weight, too many replayed calls) on
one tiny cache per eviction strategy, answered as in tests/golden/cache_refusals.json (recorded from the library of the
commit named there).  Every refusing call returns before any launch; the one call that is begun and finished admits
four rows."""
import json
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import cache_refusal_cases as cc  # noqa: E402


@pytest.mark.parametrize("strategy", cc.STRATEGIES)
def test_handle_entries_answer_as_recorded(strategy):
    from cachedembedding_amd import _lib
    golden = json.loads((HERE / "golden" / "cache_refusals.json").read_text())
    g = golden["handle"][strategy]
    want = [tuple(golden["answers"][i]) for i in g["rows"]]
    got = cc.run_handle(_lib, strategy)
    assert [label for label, _, _ in got] == g["labels"], "the fixture was recorded for another case list"
    bad = [(label, (rc, msg), w) for (label, rc, msg), w in zip(got, want) if (rc, msg) != w]
    assert not bad, f"{len(bad)} of {len(got)} cases answered differently (case, got, recorded): {bad[:5]}"
    refused = {label.split(":")[0] for label, rc, _ in got if rc}
    assert len(refused) == 19, sorted(refused)            # every entry the fixture is about refused something
