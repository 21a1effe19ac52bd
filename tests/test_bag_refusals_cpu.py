"""What the C entries of ce_bag.hip refuse, with which code and message, and in which ORDER: every case of
tests/bag_refusal_cases.py -- one good call per entry, every argument in turn set to its bad values, every two arguments
together -- is replayed on the built library and must be answered as in tests/golden/bag_refusals.json, recorded by
tests/golden/record_bag_refusals.py from the library of the commit named in the fixture.  The pairs are what pin the
order: of two bad arguments the entry names the one it checks first.  A call that passes every check reaches its first
launch, which fails here (CE_ERR_HIP; only the code is compared, the text carries a line number).  The addresses are
made up, which is why this runs only where nothing could be launched."""
import json
import sys
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import bag_refusal_cases as bc  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return json.loads((HERE / "golden" / "bag_refusals.json").read_text())


def test_the_fixture_covers_every_entry_ce_bag_defines(golden):
    assert sorted(golden["entries"]) == sorted(bc.ENTRIES) and len(bc.ENTRIES) == 24
    for entry, g in golden["entries"].items():
        assert g["singles"] == [label for label, _, _ in bc.singles(entry)], \
            f"{entry}: the fixture was recorded for another case list"
        assert len(g["rows"]) == len(bc.cases(entry))
    assert [0, None] in golden["answers"] or [bc.CE_ERR_HIP, None] in golden["answers"]


@pytest.mark.parametrize("entry", list(bc.ENTRIES))
def test_entry_answers_as_recorded(golden, entry):
    if torch.cuda.is_available():
        pytest.skip("passes made-up addresses: only for machines without a GPU")
    from cachedembedding_amd import _lib
    want = [tuple(golden["answers"][i]) for i in golden["entries"][entry]["rows"]]
    got = bc.run(_lib.lib, _lib.last_error, entry)
    assert len(got) == len(want)
    bad = [(label, (rc, msg), w) for (label, rc, msg), w in zip(got, want) if (rc, msg) != w]
    assert not bad, f"{entry}: {len(bad)} of {len(got)} cases answered differently (case, got, recorded): {bad[:5]}"
