"""Inputs of the tests of the sorted (deterministic) fold for the in-row fused optimizers, shared by
tests/test_sorted_in_row_cpu.py and tests/test_gpu_sorted_in_row.py, and the numpy models they are held to: the existing
references (adam_ref, partial_rowwise_adam_ref, adagrad_layout_ref with weight_decay_ref / grad_clip_ref in front) fed
either lookup by lookup (fp64: the authority) or with sorted_fold_ref.fold_sorted's gradient (fp32: the kernels' order).
A step is a dict(ids, off, off32, mode, psw, hook, go, act, lr) as in partial_rowwise_adam_cases.kernel_steps.  Test
infrastructure only."""
import numpy as np
import torch

import adagrad_layout_cases as ac
import adagrad_layout_ref as aref
import adam_cases
import grad_clip_ref as gref
import partial_rowwise_adam_cases as pc
import sorted_fold_ref as sf
from rowwise_adagrad_ref import lookup_grads

LAYOUTS = ("adam", "partial_rowwise_adam", "adagrad")
SPAN = {"adam": 3, "partial_rowwise_adam": 2, "adagrad": 2}
R = 96
DIMS = (8, 128, 768)                # one chunk per lane with idle lanes; NCH 1 with a full wave; NCH 4 with three chunks live
BETAS, EPS_ADAM, EPS_ADAGRAD = pc.BETAS, pc.EPS, ac.EPS
WD = pc.WD
RTOL, ATOL = ac.RTOL, ac.ATOL
STEPS = 7


def eps_of(layout):
    return EPS_ADAGRAD if layout == "adagrad" else EPS_ADAM


# ---- the models ------------------------------------------------------------------------------------------------------

def new_state(layout, W0, dtype, init_acc=0.0, v_rows=None):
    W = W0.astype(dtype)
    if layout == "adam":
        return dict(W=W, M=np.zeros_like(W), V=np.zeros_like(W))
    if layout == "partial_rowwise_adam":
        return dict(W=W, M=np.zeros_like(W), V=np.zeros(W.shape[0] if v_rows is None else v_rows, dtype))
    return dict(W=W, S=np.full_like(W, dtype(init_acc)))


def model_step(layout, st, rows, grads, lr, t, dtype, wd=0.0, wd_mode="l2", grad_clip=None, clip_mode="value",
               lr_decay=0.0, row_of=None):
    """one step of the layout's reference in place; rows / grads: the lookups that take part, or unique rows with their
    folded gradients (folding those again is the identity)"""
    if layout == "adam":
        gref.step_adam(st["W"], st["M"], st["V"], rows, grads, lr, t, BETAS, EPS_ADAM, wd, wd_mode, dtype, grad_clip,
                       clip_mode)
    elif layout == "partial_rowwise_adam":
        gref.step_pradam(st["W"], st["M"], st["V"], rows, grads, lr, t, BETAS, EPS_ADAM, wd, wd_mode, dtype, row_of,
                         grad_clip, clip_mode)
    else:
        aref.step(st["W"], st["S"], rows, grads, lr, t, EPS_ADAGRAD, lr_decay, dtype, wd, wd_mode, grad_clip, clip_mode)


def folded(s, num_rows, wrong=None):
    """(unique rows, folded gradients fp32) of one step in the sorted fold's order"""
    slots, rows, scales = sf.lookup_terms(s["ids"], s["off"], s["go"], num_rows, s["mode"], s["psw"], s["hook"])
    return sf.fold_sorted(slots, rows, scales, s["go"].shape[-1], wrong)


def model(layout, W0, steps, dtype=np.float64, init_acc=0.0, clip_mode="value", grad_clip=None, **kw):
    """(state, named) after `steps`: fp64 lookup by lookup, or fp32 with the sorted fold in front of the fp32 reference
    steps; clip_mode "row_norm" with grad_clip None: ac.row_norm_threshold(D)"""
    st = new_state(layout, W0, dtype, init_acc)
    if clip_mode == "row_norm" and grad_clip is None:
        grad_clip = ac.row_norm_threshold(W0.shape[1])
    named = np.zeros(W0.shape[0], bool)
    for t, s in enumerate(steps, 1):
        if dtype == np.float32:
            rows, grads = folded(s, W0.shape[0])
        else:
            rows, grads = lookup_grads(s["ids"], s["off"], s["go"].astype(dtype), W0.shape[0], mode=s["mode"],
                                       psw=s["psw"], hook_features=s["hook"], dtype=dtype)
        named[rows] = True
        model_step(layout, st, rows, grads, s["lr"], t, dtype, grad_clip=grad_clip, clip_mode=clip_mode, **kw)
    return st, named


def parts(layout, st):
    """the state as (name, array) pairs in the order the table's row holds them; partial row-wise Adam's V last"""
    if layout == "adagrad":
        return [("w", st["W"]), ("s", st["S"])]
    return [("w", st["W"]), ("m", st["M"]), ("v", st["V"])]


# ---- the 7-step inputs -------------------------------------------------------------------------------------------------

def zipf_steps(D, seed=11):
    """adam_cases.zipf_steps' seven first steps -- Zipf ids with heavy duplicates over adam_cases.N rows, ragged and empty
    bags, per-sample weights with zeros -- with grad_out D wide and conditioned as kernel_steps' is: one sign per column
    and magnitudes in [0.01, 0.03), so that no row's gradient nearly vanishes within a step and the comparison with
    the fp64 model says something about the kernels"""
    rng = np.random.default_rng(seed + D)
    out = []
    for k, (ids, off, _, psw) in enumerate(adam_cases.zipf_steps(seed=seed, steps=STEPS)):
        go = (rng.uniform(0.01, 0.03, (len(off) - 1, D)) * rng.choice([-1.0, 1.0], D)).astype(np.float32)
        out.append(dict(ids=ids, off=off, off32=False, mode="sum", psw=psw, hook=0, go=go, act=torch.float32,
                        lr=pc.LRS[k]))
    return out


ADAM_CASES = {"plain": dict(), "l2": dict(wd=WD, wd_mode="l2"), "decoupled": dict(wd=WD, wd_mode="decoupled"),
              "row_norm": dict(clip_mode="row_norm")}
# (layout, input, case): the seven-step runs of both test files
SEVEN = [("adam", "zipf", c) for c in ADAM_CASES] + [("adam", "kernel", "plain")] + \
        [("partial_rowwise_adam", "zipf", "plain")] + [("partial_rowwise_adam", "kernel", c) for c in ADAM_CASES] + \
        [("adagrad", "kernel", c) for c in ac.MODEL_CASES]


def seven(layout, which, case, D):
    """(W0, steps, kwargs of model() and of the kernel call)"""
    kw = (ac.MODEL_CASES if layout == "adagrad" else ADAM_CASES)[case]
    if which == "zipf":
        return np.random.default_rng(D).standard_normal((adam_cases.N, D)).astype(np.float32), zipf_steps(D), kw
    return ac.initial_weight(D, D), ac.kernel_steps(D, False, seed=D), kw


# ---- the hot-run step ----------------------------------------------------------------------------------------------------

RUNS = (1, 2, 63, 64, 65, 128, 129, 200, 4100)          # the last one crosses a 4096-lookup sort tile
HOT_FORMS = ("sum", "mean", "psw", "hook")
HOT_NB, HOT_F = 320, 4


def hot_step(D, form, seed=0, act=torch.float32):
    """ONE step over R = 96 rows whose run lengths are RUNS (nnz = 4752 plus 40 ignored lookups), the lookups shuffled
    so that every run is spread over the call and starts at a sorted position that is no multiple of 64.  form: "sum"
    (ragged bags), "mean" (ragged bags, an empty one among them), "psw" (per-sample weights, some exactly 0 and some
    exactly 1) or "hook" (the folded shape hook, F = 4).  Standard-normal gradients: the bit tests need no conditioning."""
    assert form in HOT_FORMS
    rng = np.random.default_rng(seed * 1000 + D + 17 * HOT_FORMS.index(form))
    rows = rng.permutation(R)[:len(RUNS)]
    ids = np.concatenate([np.full(n, r) for r, n in zip(rows, RUNS)] + [np.full(20, -1), np.full(20, R + 3)])
    ids = ids[rng.permutation(len(ids))].astype(np.int64)
    nnz = len(ids)
    cuts = np.sort(rng.integers(0, nnz + 1, HOT_NB - 1))
    cuts[100] = cuts[99]                                              # an empty bag, whatever the draw
    off = np.concatenate([[0], cuts, [nnz]]).astype(np.int64)
    psw = None
    if form == "psw":
        psw = rng.uniform(0.5, 1.5, nnz).astype(np.float32)
        kind = rng.random(nnz)
        psw[kind < 0.2] = 0.0
        psw[kind > 0.8] = 1.0
    shape = (HOT_NB // HOT_F, HOT_F, D) if form == "hook" else (HOT_NB, D)
    go = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(act).float().numpy()
    return dict(ids=ids, off=off, off32=False, mode="mean" if form == "mean" else "sum", psw=psw,
                hook=HOT_F if form == "hook" else 0, go=go, act=act, lr=0.05)


# ---- the ignore rules ----------------------------------------------------------------------------------------------------

IG_R = 64                           # a power of two: the ignored lookups' sort key needs a bit of its own
IG_HEAD_ONLY, IG_TAIL_ONLY, IG_ZERO_ONLY, IG_V_NEG, IG_V_PAST = 10, 11, 12, 20, 21


def ignore_step(D, seed=4):
    """ONE step, sum with per-sample weights: offsets[0] = 3 (row IG_HEAD_ONLY and row R - 1 lie in front of the first
    bag), a tail of 4 lookups behind the last bag (row IG_TAIL_ONLY, row R - 1 again), ids -1, R and R + 5 among the
    covered ones; row R - 1 three times among the covered ones; row IG_ZERO_ONLY only with weight zero; rows IG_V_NEG /
    IG_V_PAST covered (the partial layout's test points their row_of_slot outside v)."""
    rng = np.random.default_rng(seed + D)
    R_ = IG_R
    head = [IG_HEAD_ONLY, R_ - 1, IG_HEAD_ONLY]
    body = [R_ - 1, 5, -1, R_ - 1, R_, IG_ZERO_ONLY, IG_V_NEG, R_ + 5, IG_V_PAST, R_ - 1, 7, IG_ZERO_ONLY, 5, 3, -1, 0,
            IG_V_NEG, 1, 2, 5, R_, 8, 9]
    tail = [IG_TAIL_ONLY, R_ - 1, IG_TAIL_ONLY, 4]
    ids = np.asarray(head + body + tail, np.int64)
    lo, hi = len(head), len(head) + len(body)
    off = np.asarray([lo, lo + 4, lo + 4, lo + 9, lo + 15, lo + 20, hi], np.int64)
    psw = rng.uniform(0.5, 1.5, len(ids)).astype(np.float32)
    psw[ids == IG_ZERO_ONLY] = 0.0
    go = rng.standard_normal((len(off) - 1, D)).astype(np.float32)
    return dict(ids=ids, off=off, off32=False, mode="sum", psw=psw, hook=0, go=go, act=torch.float32, lr=0.05)
