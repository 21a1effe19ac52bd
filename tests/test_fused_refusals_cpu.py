"""What the fused-update switches, the set_fused_* setters and the front of embedding_bag refuse, with which exception
class and message, and in which ORDER -- and what they accept: every case of tests/fused_refusal_cases.py is replayed on
CPU tensors and must be answered as in tests/golden/fused_refusals.json, recorded by
tests/golden/record_fused_refusals.py from the commit named in the fixture, before the refusals were given one rule
set.  No kernel runs: embedding_bag ends at stand-ins for its autograd functions.  Stage B also holds every switch's
fields after the call to the recording, a refused call's included."""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE), str(HERE / "golden")]
import fused_refusal_cases as fc  # noqa: E402

PATH = HERE / "golden" / "fused_refusals.json"
FIXTURE = json.loads(PATH.read_text())


def recorded(column):
    return [tuple(FIXTURE["answers"][i]) for i in fc.decode(FIXTURE[column])]


def test_the_fixture_was_recorded_for_these_case_lists():
    from record_fused_refusals import MAX_BYTES
    assert PATH.stat().st_size < MAX_BYTES
    lists = dict(a=fc.stage_a_cases(), b=fc.stage_b_cases(), c=fc.stage_c_cases(), gpu=fc.gpu_cases())
    assert {k: [len(v), fc.digest(v)] for k, v in lists.items()} == FIXTURE["cases"]
    for column in lists:
        kinds = {k in ("accepted", "reached") for k, _ in recorded(column)}
        assert kinds == {True, False}, f"{column}: refused and accepted cases"


def test_constructors_answer_as_recorded():
    from cachedembedding_amd import functional as F
    got = fc.run_stage_a(F)
    diff = fc.differences(fc.brief_outcomes(got), recorded("a"), [(c, g) for c, g in zip(fc.stage_a_cases(), got)])
    assert not diff, diff


def test_setters_answer_as_recorded_and_leave_the_recorded_state():
    import cachedembedding_amd as ce
    from cachedembedding_amd import functional as F
    from cachedembedding_amd.parallel import RowwiseShardedEmbeddingBag
    got = fc.run_stage_b(F, ce.CachedEmbeddingBag, RowwiseShardedEmbeddingBag)
    want = list(zip(recorded("b"), (FIXTURE["states"][i] for i in fc.decode(FIXTURE["b_state"]))))
    diff = fc.differences(fc.brief_states(got), want, [(c, g[1]) for c, g in zip(fc.stage_b_cases(), got)])
    assert not diff, diff


def test_a_refused_setter_changes_nothing():
    """read off the recording itself: behind every refusal lies the state of a stub nobody has called"""
    import cachedembedding_amd as ce
    from cachedembedding_amd import functional as F
    from cachedembedding_amd.parallel import RowwiseShardedEmbeddingBag
    cases = fc.stage_b_cases()
    rows = fc.run_stage_b(F, ce.CachedEmbeddingBag, RowwiseShardedEmbeddingBag)
    refused = 0
    for (setter, dev, _), ((kind, _), state) in zip(cases, rows):
        if kind == "accepted":
            continue
        refused += 1
        untouched = "_lr=None" if setter.startswith("sharded.") else fc.stub_state(fc.make_stub(F, {**fc.STUB_BASE, **dev}))
        assert state == untouched, (setter, dev, state)
    assert refused > 1000


def test_the_front_of_embedding_bag_answers_as_recorded():
    from cachedembedding_amd import functional as F
    cases = fc.stage_c_cases()
    diff = fc.differences(fc.run_stage_c(F, cases), recorded("c"), cases)
    assert not diff, diff
    assert F._BagFn.apply.__self__ is F._BagFn               # the stand-ins are gone again
