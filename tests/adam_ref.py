"""Reference of the fused Adam update of an Adam-layout table (rows w | m | v; include/ce_api.h) in
numpy: the specification the HIP kernels (ce_bag_adagrad.hip) are held to.  Test infrastructure only.

torch.optim.SparseAdam, spelled out.  Per step and per UNIQUE row r the step looks up, t the step count (from 1):
    g    = sum over the step's lookups j of row r of scale_j * grad_out[bag(j)]   (rowwise_adagrad_ref.lookup_grads)
    omb1 = 1 - beta1, omb2 = 1 - beta2                          (fp64 difference; the fp32 form rounds it once)
    c_t  = sqrt(1 - beta2^t) / (1 - beta1^t)                    (fp64; the fp32 form rounds it once)
    m'   = m + omb1 * (g - m)
    v'   = v + omb2 * (g * g - v)
    w'   = w - (lr * c_t) * (m' / (sqrt(v') + eps))
Rows no lookup names keep w, m and v.  A row named only by lookups of weight zero has g = 0 and still decays.
Two forms: fp64 throughout (dtype=np.float64) and fp32 operation by operation (dtype=np.float32)."""
import numpy as np

from rowwise_adagrad_ref import lookup_grads  # noqa: F401  (re-exported: the lookups that take part)


def bias_correction(t, betas, dtype=np.float64):
    b1, b2 = float(betas[0]), float(betas[1])
    return dtype(np.sqrt(1.0 - b2 ** float(t)) / (1.0 - b1 ** float(t)))


def fold(rows, grads, D, dtype=np.float64):
    """(unique rows ascending, their folded gradients)"""
    if len(rows) == 0:
        return np.zeros(0, np.int64), np.zeros((0, D), dtype)
    uniq, inv = np.unique(rows, return_inverse=True)
    g = np.zeros((len(uniq), D), dtype)
    np.add.at(g, inv, np.asarray(grads, dtype))
    return uniq, g


def step(W, M, V, rows, grads, lr, t, betas=(0.9, 0.999), eps=1e-8, dtype=np.float64):
    """One Adam step in place on W, M, V [R, D]; t = the step count AFTER this step's increment (1 for the first)."""
    assert W.dtype == dtype and M.dtype == dtype and V.dtype == dtype
    uniq, g = fold(rows, grads, W.shape[1], dtype)
    if len(uniq) == 0:
        return
    omb1, omb2 = dtype(1.0 - float(betas[0])), dtype(1.0 - float(betas[1]))
    size = dtype(dtype(lr) * bias_correction(t, betas, dtype))
    m = (M[uniq] + omb1 * (g - M[uniq])).astype(dtype)
    v = (V[uniq] + omb2 * (g * g - V[uniq])).astype(dtype)
    q = (m / (np.sqrt(v).astype(dtype) + dtype(eps))).astype(dtype)
    W[uniq] = (W[uniq] - (size * q).astype(dtype)).astype(dtype)
    M[uniq] = m
    V[uniq] = v


def step_per_lookup(W, M, V, rows, grads, lr, t, betas=(0.9, 0.999), eps=1e-8, dtype=np.float64):
    """The WRONG form: the update applied once per lookup (what an optimizer over duplicated gradient rows would do)."""
    for r, gr in zip(rows, grads):
        step(W, M, V, np.asarray([r]), np.asarray([gr]), lr, t, betas, eps, dtype)
