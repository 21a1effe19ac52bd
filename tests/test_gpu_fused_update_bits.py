"""The bits of the atomic fused optimizer updates, pinned: every case of tests/fused_update_cases.py is replayed on the
built library with accumulator="cache" and with accumulator="step", and must give the bits of
tests/golden/fused_update_bits.npz -- recorded by tests/golden/record_fused_update_bits.py from the library of the
commit named in the fixture, before the copies of the row update in the two atomic paths became one function
(update_row, ce_bag_adagrad.hip).  Since then these two paths are equal by construction, so their equality no longer
says that the arithmetic stayed what it was; this file does.  A failure names the case, the path and the (step, row)
pairs."""
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import fused_update_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = fc.cases()


@pytest.fixture(scope="module")
def golden():
    with np.load(HERE / "golden" / "fused_update_bits.npz") as z:
        g = {k: z[k] for k in z.files}
    assert [str(n) for n in g["names"]] == [c.name for c in CASES], "the fixture was recorded for another case list"
    return g


def test_the_cases_cover_what_they_are_meant_to():
    names = {c.name for c in CASES}
    for kind in fc.KINDS:
        for D in fc.VEC_D:
            assert f"{kind}/slots/{D}" in names
        assert f"{kind}/src/128" in names
    for D in fc.SCALAR_D:
        assert f"fp32-adagrad/slots/{D}" in names
    # Adagrad with stochastic rounding on a 16-bit table is not pinned here but run by tests/test_gpu_stochastic_adagrad.py
    assert not any(c.adagrad and c.kind.endswith("stoch") for c in CASES)
    by = {c.name: c for c in CASES}
    assert by["fp32-adagrad/slots/6"].paths == by["bf16-sgd-stoch/src/128"].paths == ("cache", "step")


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.name for c in CASES])
def test_bits_equal_the_recorded_ones(golden, index):
    case = CASES[index]
    for path in case.paths:
        crc, mom = fc.run(case, index, path)
        if mom is not None:
            bad = fc.differing_rows(mom, golden["momentum"][index])
            assert not bad, (case.name, path, "momentum (step, row)", bad[:8])
        bad = fc.differing_rows(crc, golden["crc"][index])
        assert not bad, (case.name, path, "weight (step, row)", bad[:8])
