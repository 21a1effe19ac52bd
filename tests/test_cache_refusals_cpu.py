"""What ce_cache_create refuses, with which code and message, and in which ORDER: every bad configuration of
tests/cache_refusal_cases.py -- alone and paired with every other one -- is replayed on the built library and must be
answered as in tests/golden/cache_refusals.json, recorded by tests/golden/record_cache_refusals.py from the library of
the commit named in the fixture.  ce_cache_create refuses all of them before its first HIP call; the one good
configuration reaches that call, which fails here (CE_ERR_HIP).  The addresses are made up, which is why this runs only
where nothing could be launched."""
import json
import sys
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import cache_refusal_cases as cc  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return json.loads((HERE / "golden" / "cache_refusals.json").read_text())


def test_the_fixture_was_recorded_for_this_case_list(golden):
    g = golden["create"]
    assert g["singles"] == [label for label, _, _ in cc.CREATE_SINGLES] and len(g["singles"]) == 18
    assert len(g["rows"]) == len(cc.create_cases())
    assert golden["answers"][g["rows"][0]] == [cc.CE_ERR_HIP, None]          # the good configuration


def test_create_answers_as_recorded(golden):
    if torch.cuda.is_available():
        pytest.skip("passes made-up addresses: only for machines without a GPU")
    from cachedembedding_amd import _lib
    want = [tuple(golden["answers"][i]) for i in golden["create"]["rows"]]
    got = cc.run_create(_lib)
    assert len(got) == len(want)
    bad = [(label, (rc, msg), w) for (label, rc, msg), w in zip(got, want) if (rc, msg) != w]
    assert not bad, f"{len(bad)} of {len(got)} cases answered differently (case, got, recorded): {bad[:5]}"
