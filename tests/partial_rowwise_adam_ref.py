"""Reference of the fused partial row-wise Adam update (rows w | m, one second moment per row; include/ce_api.h,
DESIGN.md 3.13; FBGEMM's PARTIAL_ROWWISE_ADAM) in numpy: the specification the HIP kernels (ce_bag_adagrad.hip) are
held to.  Test infrastructure only.

The convention is tests/adam_ref.py's; only v differs.  Per step and per UNIQUE row r the step looks up, t the step
count (from 1), g the row's folded gradient (adam_ref.fold of rowwise_adagrad_ref.lookup_grads):
    omb1 = 1 - beta1, omb2 = 1 - beta2                          (fp64 difference; the fp32 form rounds it once)
    c_t  = sqrt(1 - beta2^t) / (1 - beta1^t)                    (fp64; the fp32 form rounds it once)
    h    = g                          no decay
    h    = g + wd * w                 wd_mode "l2"
    w    = w * f, h = g               wd_mode "decoupled"; f = 1 - lr * wd (fp64; the fp32 form rounds it once)
    ss   = sum of h_i^2 over the row
    v'   = v[r] + omb2 * (ss / D - v[r])                        ONE scalar per row
    m'   = m + omb1 * (h - m)                                   per element
    w'   = w - (lr * c_t) * (m' / (sqrt(v') + eps))             per element
Rows no lookup names keep w, m and v.  A row named only by lookups of weight zero has g = 0 and still decays m and v.
`row_of` (the kernels' row_of_slot): W and M are then indexed by slot and V by row_of[slot]; a slot whose row lies
outside [0, len(V)) is left alone -- no update, no decay.
Two forms: fp64 throughout (dtype=np.float64) and fp32 operation by operation (dtype=np.float32)."""
import numpy as np

from adam_ref import bias_correction, fold
from rowwise_adagrad_ref import lookup_grads  # noqa: F401  (re-exported: the lookups that take part)


def step(W, M, V, rows, grads, lr, t, betas=(0.9, 0.999), eps=1e-8, dtype=np.float64, wd=0.0, wd_mode="l2",
         row_of=None, v_from="mean"):
    """One step in place on W, M [R, D] and V [N]; t = the step count AFTER this step's increment (1 for the first).
    v_from="sum" is a WRONG form (the sum of squares instead of their mean feeds v)."""
    assert W.dtype == dtype and M.dtype == dtype and V.dtype == dtype and V.ndim == 1
    D = W.shape[1]
    uniq, g = fold(rows, grads, D, dtype)
    if len(uniq) == 0:
        return
    r = uniq if row_of is None else np.asarray(row_of, np.int64)[uniq]
    ok = (r >= 0) & (r < len(V))
    uniq, g, r = uniq[ok], g[ok], r[ok]
    omb1, omb2 = dtype(1.0 - float(betas[0])), dtype(1.0 - float(betas[1]))
    size = dtype(dtype(lr) * bias_correction(t, betas, dtype))
    w = W[uniq]
    h = g
    if wd and wd_mode == "l2":
        h = (g + (dtype(wd) * w).astype(dtype)).astype(dtype)
    elif wd:
        w = (w * dtype(1.0 - float(dtype(lr)) * float(dtype(wd)))).astype(dtype)
    ss = np.sum((h * h).astype(dtype), axis=1, dtype=dtype)
    mean = ss if v_from == "sum" else (ss / dtype(D)).astype(dtype)
    v = (V[r] + (omb2 * (mean - V[r]).astype(dtype)).astype(dtype)).astype(dtype)
    m = (M[uniq] + (omb1 * (h - M[uniq]).astype(dtype)).astype(dtype)).astype(dtype)
    q = (m / (np.sqrt(v).astype(dtype) + dtype(eps))[:, None]).astype(dtype)
    W[uniq] = (w - (size * q).astype(dtype)).astype(dtype)
    M[uniq] = m
    V[r] = v


def step_per_lookup(W, M, V, rows, grads, lr, t, betas=(0.9, 0.999), eps=1e-8, dtype=np.float64):
    """The WRONG form: the update applied once per lookup (what an optimizer over duplicated gradient rows would do)."""
    for r, gr in zip(rows, grads):
        step(W, M, V, np.asarray([r]), np.asarray([gr]), lr, t, betas, eps, dtype)
