"""Inputs of the kernel-level tests of partial row-wise Adam (tests/test_gpu_partial_rowwise_adam.py) and their fp64 /
fp32 model runs; tests/test_partial_rowwise_adam_cpu.py vets on these very inputs that the fp32 reference alone keeps
the tolerance the GPU tests hold the kernels to.  Test infrastructure only."""
import numpy as np
import torch

import partial_rowwise_adam_ref as ref

LR, BETAS, EPS = 0.05, (0.9, 0.999), 1e-8
WD = 0.01
R, NNZ, NB = 200, 600, 120        # across three 64-position waves; R - 1 is named only where no bag covers it
HOT, F = 3, 4
STEPS = 7
LRS = [LR * s for s in (1.0, 0.5, 2.0, 1.0, 0.25, 1.0, 1.0)]      # the rate changes between steps


def kernel_steps(D, src, seed):
    """7 steps of 600 lookups over R = 200 rows.  Row HOT is looked up 70 times in every step; rows [R - 20, R - 5) at
    most once per step; rows [R - 5, R) never -- except in the tail no bag covers.  By step: 0 an ignored (-1) lookup,
    empty bags and an uncovered tail, 1 mean, 2 per-sample weights with zeros (one row named ONLY with weight zero), 3
    int32 offsets, 4 hook_features, 5 bf16 grad_out, 6 fp16 grad_out.  Source-row keys hold no per-lookup scale: there
    steps 1 and 2 are plain sums.  Bags are ragged in every step.

    As in tests/test_gpu_adam.py the gradients of a step have one sign per column and magnitudes in [0.01, 0.03), so no
    row's whole gradient nearly vanishes within a step and the hot row's 70 terms sum to at most 2.1: the fp32 fold
    errs by at most 69 u 2.1 = 8.7e-6, a tenth of which reaches m."""
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
        cuts = np.sort(rng.integers(0, cover + 1, NB - 1))
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
        go = (rng.uniform(0.01, 0.03, (NB // F, F, D) if hook else (NB, D)) * rng.choice([-1.0, 1.0], D)).astype(np.float32)
        act = {5: torch.bfloat16, 6: torch.float16}.get(k, torch.float32)
        go = torch.from_numpy(go).to(act).float().numpy()            # what a 16-bit grad_out holds
        out.append(dict(ids=ids, off=off, off32=k == 3, mode=mode, psw=psw, hook=hook, go=go, act=act, lr=LRS[k]))
    return out


def initial_weight(D, seed):
    return np.random.default_rng(seed).standard_normal((R, D)).astype(np.float32)


def model(W0, steps, dtype=np.float64, wd=0.0, wd_mode="l2"):
    """(W, M, V, named) of the reference after `steps`"""
    W = W0.astype(dtype)
    M, V = np.zeros_like(W), np.zeros(W.shape[0], dtype)
    named = np.zeros(W.shape[0], bool)
    for t, s in enumerate(steps, 1):
        rows, grads = ref.lookup_grads(s["ids"], s["off"], s["go"].astype(dtype), W.shape[0], mode=s["mode"],
                                       psw=s["psw"], hook_features=s["hook"], dtype=dtype)
        named[rows] = True
        ref.step(W, M, V, rows, grads, s["lr"], t, BETAS, EPS, dtype=dtype, wd=wd, wd_mode=wd_mode)
    return W, M, V, named
