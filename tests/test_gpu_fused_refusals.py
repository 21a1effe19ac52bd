"""The GPU column of tests/golden/fused_refusals.json: on tensors that are not on the GPU FusedRowwiseAdagrad.check
refuses the momentum and the in-row switches' check the step count, so a CPU replay never sees what the front of
embedding_bag does behind them.  The cases of those switches (fused_refusal_cases.gpu_cases()) are replayed here with
every tensor on the device, and with them the one case the CPU cannot make: a CPU learning-rate tensor beside a device
weight.  A few tiny tensors are allocated and nothing is launched: embedding_bag ends at stand-ins for its autograd
functions."""
import json
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import fused_refusal_cases as fc  # noqa: E402


def test_the_front_of_embedding_bag_answers_as_recorded_on_device_tensors():
    import torch

    from cachedembedding_amd import functional as F
    golden = json.loads((HERE / "golden" / "fused_refusals.json").read_text())
    cases = fc.gpu_cases()
    assert [len(cases), fc.digest(cases)] == golden["cases"]["gpu"], "the fixture was recorded for another case list"
    want = [tuple(golden["answers"][i]) for i in fc.decode(golden["gpu"])]
    got = fc.run_stage_c(F, cases, torch.device("cuda", torch.cuda.current_device()))
    diff = fc.differences(got, want, cases)
    assert not diff, diff
    said = " ".join(msg for _, msg in got)
    for behind in ("the learning-rate tensor is on cpu", "momentum must have a row", "slots outside [0, C)",
                   "row_of_slot must be", "partial row-wise Adam needs exp_avg_sq", "row_of_slot: a contiguous"):
        assert behind in said, behind                        # what only this column can reach
