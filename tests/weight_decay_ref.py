"""Reference of weight decay in the fused updates (include/ce_api.h "Weight decay") in numpy: the
specification the ce_*_wd entries are held to.  Test infrastructure only.

The decay is LAZY: in a step exactly the rows the step names -- the rows of rowwise_adagrad_ref.lookup_grads, which
drops slots outside [0, R) and lookups no bag covers and keeps lookups of weight zero -- are decayed, once.  With w the
row before the step and g its folded gradient:
    "l2":        h = g + wd * w ; the update of rowwise_adagrad_ref.step / adam_ref.step / SGD with h in place of g
                 everywhere (row-wise Adagrad's sum h^2 / D too)
    "decoupled": w_d = w * (1 - lr * wd) ; the same update with w_d in place of w and the raw g  (Adam: lr, not lr c_t)
    wd == 0:     the update of the existing references, exactly
dtype=np.float64: fp64 throughout; np.float32: operation by operation in fp32 (the factor 1 - lr wd is the fp64
difference rounded once, as the kernels form it).  A row whose momentum index lies outside M is not touched."""
import numpy as np

import adam_ref
import rowwise_adagrad_ref as adagrad_ref
from rowwise_adagrad_ref import lookup_grads  # noqa: F401  (re-exported)

MODES = ("l2", "decoupled")


def _decay(w, g, lr, wd, mode, dtype):
    """(w the update starts from, h the gradient it sees)"""
    assert mode in MODES
    if wd == 0:
        return w, g
    if mode == "l2":
        return w, (g + (dtype(wd) * w).astype(dtype)).astype(dtype)
    f = dtype(1.0 - float(dtype(lr)) * float(dtype(wd)))
    return (w * f).astype(dtype), g


def step_sgd(W, rows, grads, lr, weight_decay=0.0, mode="l2", dtype=np.float64):
    """One lazy SGD step in place: W[r] = w - lr * h for every named row."""
    assert W.dtype == dtype
    uniq, g = adam_ref.fold(rows, grads, W.shape[1], dtype)
    if len(uniq) == 0:
        return
    w, h = _decay(W[uniq], g, lr, weight_decay, mode, dtype)
    W[uniq] = (w - (dtype(lr) * h).astype(dtype)).astype(dtype)


def step_adagrad(W, M, rows, grads, lr, eps=1e-8, weight_decay=0.0, mode="l2", dtype=np.float64, row_of=None):
    """One lazy exact row-wise Adagrad step in place (rowwise_adagrad_ref.step's arithmetic, spelled the same way)."""
    assert W.dtype == dtype and M.dtype == dtype
    D = W.shape[1]
    uniq, g = adam_ref.fold(rows, grads, D, dtype)
    for k, r in enumerate(uniq):
        m_idx = r if row_of is None else int(row_of[r])
        if m_idx < 0 or m_idx >= len(M):
            continue
        w, h = _decay(W[r], g[k], lr, weight_decay, mode, dtype)
        m = dtype(M[m_idx] + dtype(np.sum(h * h, dtype=dtype)) / dtype(D))
        M[m_idx] = m
        W[r] = w - h * dtype(dtype(lr) / (np.sqrt(m) + dtype(eps)))


def step_adam(W, M, V, rows, grads, lr, t, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, mode="l2",
              dtype=np.float64):
    """One lazy Adam step in place (adam_ref.step's arithmetic); t = the step count after this step's increment."""
    assert W.dtype == dtype and M.dtype == dtype and V.dtype == dtype
    uniq, g = adam_ref.fold(rows, grads, W.shape[1], dtype)
    if len(uniq) == 0:
        return
    w, h = _decay(W[uniq], g, lr, weight_decay, mode, dtype)
    omb1, omb2 = dtype(1.0 - float(betas[0])), dtype(1.0 - float(betas[1]))
    size = dtype(dtype(lr) * adam_ref.bias_correction(t, betas, dtype))
    m = (M[uniq] + omb1 * (h - M[uniq])).astype(dtype)
    v = (V[uniq] + omb2 * (h * h - V[uniq])).astype(dtype)
    q = (m / (np.sqrt(v).astype(dtype) + dtype(eps))).astype(dtype)
    W[uniq] = (w - (size * q).astype(dtype)).astype(dtype)
    M[uniq] = m
    V[uniq] = v


# ---- the workload of the GPU test (tests/test_gpu_adam.py::_steps, restated here so that the CPU test can run it) ----

STEPS, NNZ, HOT, F = 6, 600, 3, 4
LR, WD, EPS, BETAS = 0.05, 0.05, 1e-8, (0.9, 0.999)


def steps(R, D, src, seed):
    """6 steps of 600 lookups.  Row HOT is looked up 70 times in every step; rows [R - 20, R - 5) at most once per
    step; rows [R - 5, R) never -- except row R - 1 in the tail of step 0 that no bag covers.  By step: 0 slot -1 and
    the uncovered tail, 1 mean, 2 per-sample weights with zeros (one row named ONLY with weight zero), 3 int32 offsets,
    4 hook_features, 5 a bf16 grad_out.  Source-row keys hold no per-lookup scale: there steps 1 and 2 are plain sums.
    The gradients of a step have one sign per column and magnitudes in [0.01, 0.03)."""
    import torch
    rng = np.random.default_rng(seed)
    out = []
    once = np.arange(R - 20, R - 5)
    for k in range(STEPS):
        n_once = 8
        body = rng.integers(0, R - 20, NNZ - 70 - n_once)
        body[body == HOT] = HOT + 1
        ids = np.concatenate([np.full(70, HOT), body, rng.choice(once, n_once, replace=False)])
        ids = ids[rng.permutation(NNZ)].astype(np.int64)
        cover = NNZ
        if k == 0:
            keep = ids >= R - 20
            ids[(rng.random(NNZ) < 0.1) & ~keep] = -1
            cover = NNZ - 7
            ids[cover:] = R - 1
        nb = 120
        cuts = np.sort(rng.integers(0, cover + 1, nb - 1))
        off = np.concatenate([[0], cuts, [cover]]).astype(np.int64)
        mode, psw, hook = "sum", None, 0
        if k == 1 and not src:
            mode = "mean"
        if k == 2 and not src:
            psw = rng.uniform(0.5, 1.5, NNZ).astype(np.float32)
            psw[rng.random(NNZ) < 0.15] = 0.0
            psw[ids == ids[np.isin(ids, once)][0]] = 0.0
        if k == 4:
            hook = F
        go = (rng.uniform(0.01, 0.03, (nb // F, F, D) if hook else (nb, D)) * rng.choice([-1.0, 1.0], D)).astype(np.float32)
        if k == 5:
            go = torch.from_numpy(go).to(torch.bfloat16).float().numpy()
        out.append(dict(ids=ids, off=off, off32=k == 3, mode=mode, psw=psw, hook=hook, go=go, bf16=k == 5))
    return out


def run_model(opt, W0, the_steps, mode, wd=WD, dtype=np.float64, lr=LR):
    """the whole workload through the model: (W, state..., named).  Adam in "l2" mode starts from v = 0.01, m = 0
    (g + wd w can cancel to the size of eps: DESIGN.md 3.11 / 3.12), as the tables of the GPU test do."""
    R = W0.shape[0]
    W = W0.astype(dtype)
    named = np.zeros(R, bool)
    if opt == "adam":
        M, V = np.zeros_like(W), np.full_like(W, adam_v0(mode, wd))
    else:
        M = np.zeros(R, dtype)
    for t, s in enumerate(the_steps, 1):
        rows, grads = lookup_grads(s["ids"], s["off"], s["go"], R, mode=s["mode"], psw=s["psw"], hook_features=s["hook"],
                                   dtype=dtype)
        named[rows] = True
        if opt == "adam":
            step_adam(W, M, V, rows, grads, lr, t, BETAS, EPS, wd, mode, dtype)
        elif opt == "adagrad":
            step_adagrad(W, M, rows, grads, lr, EPS, wd, mode, dtype)
        else:
            step_sgd(W, rows, grads, lr, wd, mode, dtype)
    return (W, M, V, named) if opt == "adam" else (W, M, named)


def adam_v0(mode, wd):
    return 0.01 if (mode == "l2" and wd != 0) else 0.0
