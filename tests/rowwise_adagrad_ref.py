"""Reference of the fused exact row-wise Adagrad (FBGEMM's EXACT_ROWWISE_ADAGRAD, weight_decay = 0) in numpy: the
specification the HIP kernels (ce_bag_adagrad.hip) are held to.  Test infrastructure only.

Per step and per UNIQUE row r the step looks up:
    g     = sum over the step's lookups j of row r of scale_j * grad_out[bag(j)]     (scale_j = psw_j, 1 / len for mean)
    m[r] += sum_d g[d]^2 / D
    W[r] -= lr * g / (sqrt(m[r]) + eps)
Two forms: fp64 throughout (`step(..., dtype=np.float64)`), and the fp32 one step by step (`dtype=np.float32`)."""
import numpy as np


def lookup_grads(values, offsets, grad_out, num_rows, mode="sum", psw=None, include_last_offset=True,
                 hook_features=0, padding_idx=None, dtype=np.float64):
    """(rows [n], gradient rows [n, D]) of every lookup that takes part: out-of-range rows (slot -1) and padding are
    dropped.  grad_out is [num_bags, D] or, with hook_features = F, [num_bags / F, F, D] (bag g = f * B + b)."""
    values = np.asarray(values, dtype=np.int64).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    go = np.asarray(grad_out, dtype=dtype)
    D = go.shape[-1]
    nb = len(offsets) - 1 if include_last_offset else len(offsets)
    ends = offsets[1:] if include_last_offset else np.append(offsets[1:], len(values))
    if hook_features:
        F = hook_features
        B = nb // F
        go = go.reshape(B, F, D).transpose(1, 0, 2).reshape(nb, D)        # row g = f * B + b
    go = go.reshape(nb, D)
    rows, grads = [], []
    for b in range(nb):
        lo, hi = int(offsets[b]), int(ends[b])
        ids = values[lo:hi]
        keep = (ids >= 0) & (ids < num_rows)
        if padding_idx is not None:
            keep &= ids != padding_idx
        n_valid = int(keep.sum()) if padding_idx is not None else hi - lo
        for j in range(lo, hi):
            if not keep[j - lo]:
                continue
            s = dtype(1.0)
            if psw is not None:
                s = dtype(psw[j])
            if mode == "mean" and n_valid > 1:
                s = dtype(s / dtype(n_valid))
            rows.append(int(values[j]))
            grads.append(go[b] * s)
    if not rows:
        return np.zeros(0, np.int64), np.zeros((0, D), dtype)
    return np.asarray(rows, np.int64), np.stack(grads).astype(dtype)


def step(W, M, rows, grads, lr, eps=1e-8, dtype=np.float64, row_of=None):
    """One exact row-wise Adagrad step in place.  W [R, D] (rows as the lookups name them), M [N] the accumulator,
    row_of: W row -> M index (a cache's cached_idx_map; None = identity)."""
    assert W.dtype == dtype and M.dtype == dtype
    D = W.shape[1]
    if len(rows) == 0:
        return
    uniq, inv = np.unique(rows, return_inverse=True)
    g = np.zeros((len(uniq), D), dtype)
    np.add.at(g, inv, grads.astype(dtype))
    for k, r in enumerate(uniq):
        m_idx = r if row_of is None else int(row_of[r])
        m = dtype(M[m_idx] + dtype(np.sum(g[k] * g[k], dtype=dtype)) / dtype(D))
        M[m_idx] = m
        W[r] = W[r] - g[k] * dtype(dtype(lr) / (np.sqrt(m) + dtype(eps)))


def step_per_lookup(W, M, rows, grads, lr, eps=1e-8, dtype=np.float64):
    """The WRONG form: the update applied once per lookup (what an optimizer over duplicated gradient rows would do)."""
    D = W.shape[1]
    for r, gr in zip(rows, grads):
        M[r] = M[r] + np.sum(gr * gr) / D
        W[r] = W[r] - gr * (lr / (np.sqrt(M[r]) + eps))


def accumulation_bound(grads_abs_sum, count, dtype=np.float32):
    """|fp32 sum - exact| <= (count - 1) * u * sum |terms| (the classical recursive-summation bound, u = 2^-24)"""
    u = np.finfo(dtype).eps / 2
    return max(count - 1, 1) * u * grads_abs_sum
