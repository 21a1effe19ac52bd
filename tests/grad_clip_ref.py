"""Reference of gradient clipping in the fused updates (include/ce_api.h "Gradient clipping") in numpy:
the specification the ce_*_clip entries are held to.  Test infrastructure only.

g is a row's FOLDED gradient of the step (adam_ref.fold of rowwise_adagrad_ref.lookup_grads: after per-sample weights,
the mean scaling and the fold over the row's lookups).  The clip acts on g first; the steps of weight_decay_ref /
partial_rowwise_adam_ref then run on the clipped g, so the decay's h, the sums of squares, the moments and the step all
see it -- torch's order (clip_grad_* before optimizer.step()) and FBGEMM's.  c the threshold:
    "value":     g = g < -c ? -c : (g > c ? c : g) per element                        (a NaN stays a NaN)
    "row_norm":  n = sqrt(sum_d g[d]^2) ; k = c / (n + 1e-6) ; if k < 1: g = g * k    (clip_grad_norm_, per row)
    grad_clip=None: the steps of the existing references, exactly
Clipping does not change which rows a step names.  dtype=np.float64: fp64 throughout; np.float32: operation by operation
in fp32."""
import numpy as np

import adam_ref
import partial_rowwise_adam_ref as pradam_ref
import weight_decay_ref as wref
from rowwise_adagrad_ref import lookup_grads  # noqa: F401  (re-exported)

MODES = ("value", "row_norm")
C_VALUE = 0.05                      # the thresholds of the tests' workload (weight_decay_ref.steps): value mode, and


def threshold(mode, D):
    """... c = 0.05 * sqrt(D) in row_norm mode: the same size per element"""
    return C_VALUE if mode == "value" else C_VALUE * float(np.sqrt(D))


def clipped_mask(g, c, mode, dtype=np.float64):
    """what the clip changes: the elements beyond the threshold ("value", [n, D] bool) or the rows scaled ("row_norm",
    [n] bool)"""
    g = np.asarray(g, dtype)
    if mode == "value":
        return np.abs(g) > dtype(c)
    ss = np.sum((g * g).astype(dtype), axis=1, dtype=dtype)
    k = (dtype(c) / (np.sqrt(ss).astype(dtype) + dtype(1e-6))).astype(dtype)
    return k < dtype(1.0)


def clip(g, c, mode, dtype=np.float64):
    """the clipped copy of the folded gradients g [n, D]"""
    assert mode in MODES
    g = np.asarray(g, dtype)
    if c is None:
        return g
    c = dtype(c)
    if mode == "value":
        return np.where(g < -c, -c, np.where(g > c, c, g)).astype(dtype)
    ss = np.sum((g * g).astype(dtype), axis=1, dtype=dtype)
    k = (c / (np.sqrt(ss).astype(dtype) + dtype(1e-6))).astype(dtype)
    out = g.copy()
    sel = k < dtype(1.0)
    out[sel] = (g[sel] * k[sel, None]).astype(dtype)
    return out


def _folded(rows, grads, D, c, mode, dtype):
    """(unique rows, their clipped folded gradients): folding these again is the identity, so the steps below hand them
    to the existing references as they are"""
    uniq, g = adam_ref.fold(rows, grads, D, dtype)
    return uniq, clip(g, c, mode, dtype)


def step_sgd(W, rows, grads, lr, weight_decay=0.0, wd_mode="l2", dtype=np.float64, grad_clip=None, clip_mode="value"):
    uniq, g = _folded(rows, grads, W.shape[1], grad_clip, clip_mode, dtype)
    wref.step_sgd(W, uniq, g, lr, weight_decay, wd_mode, dtype)


def step_adagrad(W, M, rows, grads, lr, eps=1e-8, weight_decay=0.0, wd_mode="l2", dtype=np.float64, row_of=None,
                 grad_clip=None, clip_mode="value"):
    uniq, g = _folded(rows, grads, W.shape[1], grad_clip, clip_mode, dtype)
    wref.step_adagrad(W, M, uniq, g, lr, eps, weight_decay, wd_mode, dtype, row_of)


def step_adam(W, M, V, rows, grads, lr, t, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, wd_mode="l2",
              dtype=np.float64, grad_clip=None, clip_mode="value"):
    uniq, g = _folded(rows, grads, W.shape[1], grad_clip, clip_mode, dtype)
    wref.step_adam(W, M, V, uniq, g, lr, t, betas, eps, weight_decay, wd_mode, dtype)


def step_pradam(W, M, V, rows, grads, lr, t, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, wd_mode="l2",
                dtype=np.float64, row_of=None, grad_clip=None, clip_mode="value"):
    uniq, g = _folded(rows, grads, W.shape[1], grad_clip, clip_mode, dtype)
    pradam_ref.step(W, M, V, uniq, g, lr, t, betas, eps, dtype, weight_decay, wd_mode, row_of)


def run_model(opt, W0, the_steps, clip_mode, grad_clip="workload", wd=0.0, wd_mode="l2", dtype=np.float64, lr=wref.LR,
              stats=None):
    """weight_decay_ref.run_model with the clip in front (opt: "sgd" / "adagrad" / "adam" / "pradam"); grad_clip
    "workload": threshold(clip_mode, D).  Returns (W, state..., named); pradam: (W, M [R, D], V [R], named).  Adam in
    "l2" mode starts from v = weight_decay_ref.adam_v0.  stats: a dict that gets "clipped" / "kept", the number of
    elements (value) or rows (row_norm) the clip changed / left alone over the whole run."""
    R, D = W0.shape
    c = threshold(clip_mode, D) if isinstance(grad_clip, str) else grad_clip
    W = W0.astype(dtype)
    named = np.zeros(R, bool)
    if opt == "adam":
        M, V = np.zeros_like(W), np.full_like(W, wref.adam_v0(wd_mode, wd))
    elif opt == "pradam":
        M, V = np.zeros_like(W), np.zeros(R, dtype)
    else:
        M = np.zeros(R, dtype)
    if stats is not None:
        stats.update(clipped=0, kept=0)
    for t, s in enumerate(the_steps, 1):
        rows, grads = lookup_grads(s["ids"], s["off"], s["go"], R, mode=s["mode"], psw=s["psw"], hook_features=s["hook"],
                                   dtype=dtype)
        named[rows] = True
        if stats is not None and c is not None:
            mask = clipped_mask(adam_ref.fold(rows, grads, D, dtype)[1], c, clip_mode, dtype)
            stats["clipped"] += int(mask.sum())
            stats["kept"] += int(mask.size - mask.sum())
        kw = dict(weight_decay=wd, wd_mode=wd_mode, dtype=dtype, grad_clip=c, clip_mode=clip_mode)
        if opt == "adam":
            step_adam(W, M, V, rows, grads, lr, t, wref.BETAS, wref.EPS, **kw)
        elif opt == "pradam":
            step_pradam(W, M, V, rows, grads, lr, t, wref.BETAS, wref.EPS, **kw)
        elif opt == "adagrad":
            step_adagrad(W, M, rows, grads, lr, wref.EPS, **kw)
        else:
            step_sgd(W, rows, grads, lr, **kw)
    return (W, M, V, named) if opt in ("adam", "pradam") else (W, M, named)
