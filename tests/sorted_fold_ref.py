"""The fold order of the sorted (deterministic) fused updates restated in numpy, fp32 operation by
operation: what the bit tests of tests/test_gpu_sorted_in_row.py predict a row's folded gradient with.  Written from the
specification's text, not from the kernels.  Test infrastructure only.

    The step's lookups are stably sorted by slot, so a slot's lookups are one run in lookup order.  A run is cut into
    chunks of CHUNK = 64 consecutive positions counted from the START OF THE RUN.  A chunk is folded from zero, strictly
    in lookup order: acc = acc + term_j, term_j the gradient row itself where s_j == 1 and otherwise the product
    s_j * g_j ROUNDED to fp32 before it is added.  The chunks' partial rows are added in ascending chunk order.

`wrong` names a plausible MISTAKE the bit tests must tell apart from the above:
    "reverse"              a chunk's lookups are added in descending lookup order
    "aligned_chunks"       chunks are cut where the SORTED POSITION is a multiple of 64, not from the start of the run
    "descending_partials"  the partial rows are added last chunk first
    "fused"                s_j * g_j is fused into the add (one rounding, an fma)"""
import numpy as np

CHUNK = 64
WRONG = ("reverse", "aligned_chunks", "descending_partials", "fused")
F32 = np.float32


def lookup_terms(values, offsets, grad_out, num_rows, mode="sum", psw=None, hook_features=0, include_last_offset=True):
    """(slots [n], gradient rows [n, D] fp32, scales [n] fp32) of the lookups that take part, in lookup order: a bag
    covers them and their slot lies in [0, num_rows).  The gradient row is the bag's grad_out row as it is (with
    hook_features = F, grad_out is [num_bags / F, F, D] and bag g = f * B + b); the scale is the per-sample weight (1
    without), divided -- in fp32 -- by the bag's length for mode "mean" where that is more than 1."""
    values = np.asarray(values, np.int64).reshape(-1)
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    go = np.asarray(grad_out, F32)
    D = go.shape[-1]
    nb = len(offsets) - 1 if include_last_offset else len(offsets)
    ends = offsets[1:] if include_last_offset else np.append(offsets[1:], len(values))
    if hook_features:
        go = go.reshape(nb // hook_features, hook_features, D).transpose(1, 0, 2)
    go = go.reshape(nb, D)
    slots, rows, scales = [], [], []
    for b in range(nb):
        lo, hi = int(offsets[b]), int(ends[b])
        for j in range(lo, hi):
            if not 0 <= values[j] < num_rows:
                continue
            s = F32(1.0) if psw is None else F32(psw[j])
            if mode == "mean" and hi - lo > 1:
                s = F32(s / F32(hi - lo))
            slots.append(int(values[j]))
            rows.append(go[b])
            scales.append(s)
    if not slots:
        return np.zeros(0, np.int64), np.zeros((0, D), F32), np.zeros(0, F32)
    return np.asarray(slots, np.int64), np.stack(rows).astype(F32), np.asarray(scales, F32)


def _fold_chunk(grads, scales, D, wrong):
    acc = np.zeros(D, F32)
    order = range(len(grads) - 1, -1, -1) if wrong == "reverse" else range(len(grads))
    for j in order:
        g, s = grads[j], scales[j]
        if s == F32(1.0):
            acc = (acc + g).astype(F32)
        elif wrong == "fused":
            acc = (acc.astype(np.float64) + g.astype(np.float64) * np.float64(s)).astype(F32)
        else:
            acc = (acc + (g * s).astype(F32)).astype(F32)
    return acc


def fold_sorted(slots, grads, scales, D, wrong=None):
    """(unique slots ascending, their folded gradients [u, D] fp32) of the lookups (slots [n], gradient rows [n, D],
    scales [n]) given in lookup order"""
    assert wrong in (None,) + WRONG
    slots = np.asarray(slots, np.int64)
    grads = np.asarray(grads, F32).reshape(len(slots), D)
    scales = np.asarray(scales, F32)
    order = np.argsort(slots, kind="stable")
    uniq, start, count = np.unique(slots[order], return_index=True, return_counts=True)
    out = np.zeros((len(uniq), D), F32)
    for u in range(len(uniq)):
        p0, n = int(start[u]), int(count[u])
        if wrong == "aligned_chunks":
            cuts = [p0] + [p for p in range((p0 // CHUNK + 1) * CHUNK, p0 + n, CHUNK)] + [p0 + n]
        else:
            cuts = list(range(p0, p0 + n, CHUNK)) + [p0 + n]
        partials = [_fold_chunk(grads[order[a:b]], scales[order[a:b]], D, wrong) for a, b in zip(cuts[:-1], cuts[1:])]
        if wrong == "descending_partials":
            partials = partials[::-1]
        total = partials[0]
        for part in partials[1:]:
            total = (total + part).astype(F32)
        out[u] = total
    return uniq, out
