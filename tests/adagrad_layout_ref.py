"""Reference of the fused element-wise Adagrad update (rows w | h, h the per-element sums of squared gradients;
include/ce_api.h; torch.optim.Adagrad, FBGEMM's EXACT_ADAGRAD) in numpy: the specification the HIP
kernels are held to.  Test infrastructure only.

Per step and per UNIQUE row the step names, t the step count (from 1), g the row's folded gradient (adam_ref.fold of
rowwise_adagrad_ref.lookup_grads), lr the rate as the kernels get it (an fp32 number):
    clr_d = lr / (1 + (t - 1) * lr_decay)                       fp64
    clr   = clr_d                                               (the fp32 form rounds it once)
    g     = clip(g)                                             grad_clip_ref.clip, first
    h     = g                          no decay
    h     = g + wd * w                 wd_mode "l2"             (the product rounded, then the sum)
    w     = w * f, h = g               wd_mode "decoupled"; f = 1 - clr_d * wd (fp64; the fp32 form rounds it once)
    s'    = s + h * h                  per element              (the product rounded, then the sum)
    w'    = w - clr * (h / (sqrt(s') + eps))                    per element
Rows no lookup names keep w and s.  A row named only by lookups of weight zero has g = 0: without decay it keeps its
bits (s + 0, w - 0).
Two forms: fp64 throughout (dtype=np.float64) and fp32 operation by operation (dtype=np.float32).

`wrong` names a plausible MISTAKE the comparison must tell apart from the above:
    "s_from_unclipped"  s' is fed by the gradient as it was before the clip
    "f_from_lr"         the decoupled factor is 1 - lr * wd, not 1 - clr_d * wd
    "t_off_by_one"      clr_d = lr / (1 + t * lr_decay)
    "rowwise_s"         s' = s + mean_d(h * h) in every column (row-wise Adagrad's state, spread over the row)"""
import numpy as np

from adam_ref import fold
from grad_clip_ref import clip
from rowwise_adagrad_ref import lookup_grads  # noqa: F401  (re-exported: the lookups that take part)

WRONG = ("s_from_unclipped", "f_from_lr", "t_off_by_one", "rowwise_s")


def rate(lr, t, lr_decay, dtype=np.float64, wrong=None):
    """(clr_d as a Python float, clr as dtype): lr is rounded to fp32 first in the fp32 form, as a kernel argument is"""
    lr = float(np.float32(lr)) if dtype == np.float32 else float(lr)
    steps = t if wrong == "t_off_by_one" else t - 1
    clr_d = lr / (1.0 + float(steps) * float(lr_decay))
    return clr_d, dtype(clr_d)


def step(W, S, rows, grads, lr, t, eps=1e-10, lr_decay=0.0, dtype=np.float64, wd=0.0, wd_mode="l2", grad_clip=None,
         clip_mode="value", wrong=None):
    """One step in place on W, S [R, D]; t = the step count AFTER this step's increment (1 for the first)."""
    assert W.dtype == dtype and S.dtype == dtype and S.shape == W.shape and wrong in (None,) + WRONG
    D = W.shape[1]
    uniq, g0 = fold(rows, grads, D, dtype)
    if len(uniq) == 0:
        return
    clr_d, clr = rate(lr, t, lr_decay, dtype, wrong)
    g = clip(g0, grad_clip, clip_mode, dtype)
    w = W[uniq]
    h = g
    wd_f = float(np.float32(wd)) if dtype == np.float32 else float(wd)
    if wd and wd_mode == "l2":
        h = (g + (dtype(wd) * w).astype(dtype)).astype(dtype)
    elif wd:
        base = (float(np.float32(lr)) if dtype == np.float32 else float(lr)) if wrong == "f_from_lr" else clr_d
        w = (w * dtype(1.0 - base * wd_f)).astype(dtype)
    fed = h
    if wrong == "s_from_unclipped":
        fed = (h - g + g0).astype(dtype)                            # what h would be without the clip
    sq = (fed * fed).astype(dtype)
    if wrong == "rowwise_s":
        sq = np.repeat((np.sum(sq, axis=1, dtype=dtype) / dtype(D)).astype(dtype)[:, None], D, axis=1)
    s = (S[uniq] + sq).astype(dtype)
    q = (h / (np.sqrt(s).astype(dtype) + dtype(eps)).astype(dtype)).astype(dtype)
    W[uniq] = (w - (clr * q).astype(dtype)).astype(dtype)
    S[uniq] = s
