"""Cases of the fused-update golden test (tests/golden/fused_update_bits.npz): one generator shared by the recorder
(tests/golden/record_fused_update_bits.py) and the replay (tests/test_gpu_fused_update_bits.py).  Test infrastructure
only; it drives the public Python API and nothing else, so it runs against any commit's library.

A case is (kind, form, D): kind = table dtype - optimizer [- stochastic rounding], form = "slots" (slots + offsets with
ignored -1 lookups) or "src" (source-row keys of presort_window).  Every case runs STEPS steps from the same start on
both atomic paths -- accumulator="cache" and accumulator="step", the two that share update_row -- and yields one CRC-32
per weight row and step and the momentum bits per step.  deterministic=True keeps its own copy of the update
 and is not replayed here.

A row is looked up at most twice per step: two fp32 terms sum the same in either order, so the atomics cannot make the
paths differ, and both are held to the same recorded bits.
The gradients are standard normal -- on a grid every square would be exact and the rounding of the sum of squares,
which this test exists for, would not show."""
import zlib
from typing import NamedTuple

import numpy as np
import torch

R, STEPS, F, LR, SEED = 40, 3, 4, 0.05, 5
TWICE, ONCE, PAD = 12, 16, 8                     # 2 * 12 + 16 + 8 = 48 lookups, a multiple of F
KINDS = ["fp32-adagrad", "bf16-adagrad", "fp16-adagrad", "bf16-sgd", "fp16-sgd", "bf16-sgd-stoch", "fp16-sgd-stoch"]
# the smallest widths that reach every lane shape: vector lanes of 1 chunk in groups of 2 (8) and 32 (128), 2 chunks
# (512), 3 of 4 (768) and 4 (1024); scalar lanes (an fp32 table only) of 1 (6), 2 (70) and 3 of 4 (130) elements
VEC_D, SCALAR_D = (8, 128, 512, 768, 1024), (6, 70, 130)
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


class Case(NamedTuple):
    kind: str
    form: str
    D: int

    @property
    def name(self):
        return f"{self.kind}/{self.form}/{self.D}"

    @property
    def adagrad(self):
        return self.kind.split("-")[1] == "adagrad"

    @property
    def paths(self):
        return ("cache", "step")


def cases():
    out = []
    for kind in KINDS:
        for D in VEC_D + (SCALAR_D if kind == "fp32-adagrad" else ()):
            out.append(Case(kind, "slots", D))
        out.append(Case(kind, "src", 128))
    return out


def _ids(rng, form):
    perm = rng.permutation(R)
    ids = np.concatenate([perm[:TWICE], perm[:TWICE], perm[TWICE:TWICE + ONCE], np.full(PAD, -1)])
    return ids[rng.permutation(len(ids))]


def _fused(case, path):
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD
    acc = path
    stoch = case.kind.endswith("stoch")
    # row-wise Adagrad with stochastic rounding on a 16-bit table is not a case HERE: the fixture records a past
    # library's bits and that combination's would be the code under test's own.  tests/test_gpu_stochastic_adagrad.py
    # holds it to tests/stochastic_update_ref.py instead
    assert not (case.adagrad and stoch)
    if case.adagrad:
        f = FusedRowwiseAdagrad(LR, momentum=torch.zeros(R, device="cuda"), accumulator=acc)
    else:
        f = FusedSGD(LR, accumulator=acc)
    f.rounding, f.seed = ("stochastic" if stoch else "nearest"), SEED
    return f


def run(case, index, path):
    """(crc uint32 [STEPS, R], momentum bits uint32 [STEPS, R] or None) of one case on one path"""
    from cachedembedding_amd.functional import embedding_bag, presort_window
    assert path in case.paths
    rng = np.random.default_rng(1000 + index)
    wt = DT[case.kind.split("-")[0]]
    w = torch.from_numpy(rng.standard_normal((R, case.D)).astype(np.float32)).to(wt).cuda()
    fused = _fused(case, path)
    crc = np.zeros((STEPS, R), np.uint32)
    mom = np.zeros((STEPS, R), np.uint32) if case.adagrad else None
    for k in range(STEPS):
        ids = _ids(rng, case.form)
        nnz = len(ids)
        go = torch.from_numpy(rng.standard_normal((nnz // F, F, case.D)).astype(np.float32)).cuda()
        idx = torch.from_numpy(ids).cuda()
        offs = torch.arange(nnz + 1, device="cuda")
        pre = None
        if case.form == "src":
            pre = presort_window(idx.view(1, -1), R, offsets=offs.to(torch.int32), include_last_offset=True,
                                 hook_features=F, identity_bags=True)[0]
        w.requires_grad_(True)
        o = embedding_bag(idx, w, offs, mode="sum", include_last_offset=True, hook_features=F, fused_sgd=fused,
                          presorted=pre, masked_indices=True, output_dtype=torch.float32)
        o.backward(go.view_as(o))
        assert w.grad is None                                     # the update happened inside backward
        w.requires_grad_(False)
        rows = w.detach().cpu().contiguous().view(torch.uint8).numpy().reshape(R, -1)
        crc[k] = [zlib.crc32(r.tobytes()) for r in rows]
        if mom is not None:
            mom[k] = fused.momentum.cpu().numpy().view(np.uint32)
    return crc, mom


def differing_rows(got, want):
    """(step, row) pairs at which two [STEPS, R] arrays differ: what a failure names"""
    return [(int(k), int(r)) for k, r in zip(*np.nonzero(got != want))]
