"""Inputs of the kernel-level tests of element-wise Adagrad (tests/test_gpu_adagrad_layout.py) and their fp64 / fp32
model runs; tests/test_adagrad_layout_cpu.py vets on these very inputs that the fp32 reference alone keeps half the
tolerance the GPU tests hold the kernels to.  The multi-step inputs are partial row-wise Adam's kernel_steps, imported,
not copied.  Test infrastructure only."""
import numpy as np

import adagrad_layout_ref as ref
import partial_rowwise_adam_cases as kc
from partial_rowwise_adam_cases import F, HOT, NB, NNZ, R, STEPS, initial_weight, kernel_steps  # noqa: F401

EPS = 1e-10                          # torch.optim.Adagrad's default
WD = kc.WD
LR_DECAY = 0.1
INIT_ACC = 0.1
RTOL, ATOL = 1e-5, 1e-6              # the tolerance tests/test_gpu_partial_rowwise_adam.py holds Adam to
DIMS = [4, 8, 32, 128, 192, 512, 768, 1024]      # every lane shape (G = 1 / 2 / 8 / 32, idle lanes, 2 / 3 of 4 / 4 chunks)
# the multi-step cases: (name, kwargs of the model and of the kernel call)
MODEL_CASES = {
    "plain": dict(),
    "lr_decay+init": dict(lr_decay=LR_DECAY, init_acc=INIT_ACC),
    "l2": dict(wd=WD, wd_mode="l2"),
    "decoupled": dict(wd=WD, wd_mode="decoupled", lr_decay=LR_DECAY),
    "row_norm": dict(clip_mode="row_norm"),          # the threshold is row_norm_threshold(D)
}


def row_norm_threshold(D):
    """kernel_steps' gradients have magnitudes in [0.01, 0.03) per lookup: a row looked up once has a norm near
    0.02 sqrt(D), the hot row's 70 lookups one near 1.4 sqrt(D).  0.05 sqrt(D) clips the rows looked up often and leaves
    the rows looked up once or twice alone, so both sides of `k < 1` are taken in every step."""
    return 0.05 * float(np.sqrt(D))


def model(W0, steps, dtype=np.float64, lr_decay=0.0, init_acc=0.0, wd=0.0, wd_mode="l2", grad_clip=None,
          clip_mode="value", wrong=None):
    """(W, S, named) of the reference after `steps`; clip_mode "row_norm" with grad_clip None: row_norm_threshold(D)"""
    W = W0.astype(dtype)
    S = np.full_like(W, dtype(init_acc))
    if clip_mode == "row_norm" and grad_clip is None:
        grad_clip = row_norm_threshold(W0.shape[1])
    named = np.zeros(W.shape[0], bool)
    for t, s in enumerate(steps, 1):
        rows, grads = ref.lookup_grads(s["ids"], s["off"], s["go"].astype(dtype), W.shape[0], mode=s["mode"],
                                       psw=s["psw"], hook_features=s["hook"], dtype=dtype)
        named[rows] = True
        ref.step(W, S, rows, grads, s["lr"], t, EPS, lr_decay, dtype, wd, wd_mode, grad_clip, clip_mode, wrong)
    return W, S, named


# ---- rows looked up once: R distinct ids plus a few -1s, one id per bag, mode sum, fp32 grad_out, three rates.  A
# lookup adds onto zero, so the folded gradient IS the grad_out row and nothing in the update has an order to choose.

ONCE_LRS = [0.05, 0.0125, 0.2]
ONCE_NAMED = R - 12                  # rows [ONCE_NAMED, R) are never named
ONCE_SETTINGS = {
    "default": dict(),
    "lr_decay": dict(lr_decay=LR_DECAY),
    "init_acc": dict(init_acc=INIT_ACC),
    "l2": dict(wd=WD, wd_mode="l2"),
    "decoupled": dict(wd=WD, wd_mode="decoupled"),
    "decoupled+lr_decay": dict(wd=WD, wd_mode="decoupled", lr_decay=LR_DECAY),
    "value_clip": dict(grad_clip=0.5, clip_mode="value"),
    "value_clip+l2+lr_decay": dict(grad_clip=0.5, clip_mode="value", wd=WD, wd_mode="l2", lr_decay=LR_DECAY),
}


def once_steps(D, seed):
    """three steps; every step names rows [0, ONCE_NAMED) once each, in a shuffled order, with 9 ignored (-1) lookups
    among them; standard-normal gradients (a third of the elements lie beyond the value clip's 0.5)"""
    rng = np.random.default_rng(seed)
    out = []
    for lr in ONCE_LRS:
        ids = np.concatenate([np.arange(ONCE_NAMED), np.full(9, -1)])[rng.permutation(ONCE_NAMED + 9)].astype(np.int64)
        n = len(ids)
        go = rng.standard_normal((n, D)).astype(np.float32)
        out.append(dict(ids=ids, off=np.arange(n + 1, dtype=np.int64), off32=False, mode="sum", psw=None, hook=0, go=go,
                        lr=lr))
    return out
