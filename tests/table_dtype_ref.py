"""Reference of the 16-bit embedding table (bf16 / fp16 rows in host DRAM and in the cache) in numpy and torch-CPU: the
specification the `ce_*_w16` entries are held to.  Test infrastructure only.

Forward.  Rows are up-converted exactly, so the forward from a 16-bit table W16 is the forward from the fp32 table
W16.float(): tests/activation_dtype_ref.py's `bag_ref64`, `forward_bound` and `assert_cast_equal` apply unchanged.
Update.  Per looked-up row, with g the fp32 fold of the step's gradient rows and w = W16[r].float():
    SGD:              x = w - lr * g
    row-wise Adagrad: m[r] += sum_d g[d]^2 / D ;  x = w - lr * g / (sqrt(m[r]) + eps)   (tests/rowwise_adagrad_ref.py)
    W16[r] = round(x): to nearest even, or stochastically -- `stochastic_round`.
Against the update evaluated in fp64 (x64) a nearest-rounded row obeys |float(W16) - x64| <= u |x64| + (1 + u) E, E the
error of the fp32 evaluation of x (`sgd_fp32_error`), + 2^-25 for fp16 (half a subnormal step) -- `update_bound`."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import activation_dtype_ref as aref  # noqa: E402,F401  (re-exported: cast, assert_cast_equal, bag_ref64, forward_bound)
import rowwise_adagrad_ref as adagrad  # noqa: E402,F401

UNIT_ROUNDOFF = aref.UNIT_ROUNDOFF
U32 = aref.U32
DROPPED_BITS = {torch.bfloat16: 16, torch.float16: 13}
CODES = {torch.bfloat16: 1, torch.float16: 2}                 # CE_ACT_BF16 / CE_ACT_F16


def neighbours(x: np.ndarray, dtype: torch.dtype):
    """(lower, upper) in magnitude: the two values of `dtype` that enclose the fp32 values x (equal when x is
    representable).  Valid where stochastic rounding applies: bf16 finite, fp16 with 2^-14 <= |x| < 65504."""
    k = DROPPED_BITS[dtype]
    b = np.asarray(x, np.float32).view(np.uint32)
    lo = b & ~np.uint32((1 << k) - 1)
    hi = np.where(b == lo, lo, lo + np.uint32(1 << k))
    return lo.view(np.float32), hi.view(np.float32)


def stochastic_round(x: np.ndarray, rnd: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """Stochastic rounding of fp32 x to `dtype` with the uniform integers rnd (only their low 16 / 13 bits count): the
    integer is added to the fp32 bit pattern below the dropped bits and the sum truncated.  NaN, infinities, fp16
    results below 2^-14 or from 65504 on, and bf16 sums past the largest finite value take the nearest cast."""
    k = DROPPED_BITS[dtype]
    x = np.ascontiguousarray(x, np.float32)
    b = x.view(np.uint32)
    t = (b + (np.asarray(rnd).astype(np.uint32) & np.uint32((1 << k) - 1))) & ~np.uint32((1 << k) - 1)
    mag = b & np.uint32(0x7fffffff)
    if dtype == torch.bfloat16:
        plain = ((b & np.uint32(0x7f800000)) == np.uint32(0x7f800000)) | \
                ((t & np.uint32(0x7f800000)) == np.uint32(0x7f800000))
    else:
        plain = (mag < np.uint32(0x38800000)) | (mag >= np.uint32(0x477fe000))
    nearest = torch.from_numpy(x).to(dtype)
    sr = torch.from_numpy(t.view(np.float32).copy()).to(dtype)          # exact: the dropped bits are zero
    return torch.where(torch.from_numpy(plain), nearest, sr)


def fold_rows(rows, grads, R, dtype=np.float64):
    """(g [R, D] the folded gradient, count [R], abs_sum [R, D]) of the step's lookups"""
    D = grads.shape[1]
    g = np.zeros((R, D), dtype)
    s = np.zeros((R, D), np.float64)
    np.add.at(g, rows, grads.astype(dtype))
    np.add.at(s, rows, np.abs(grads.astype(np.float64)))
    return g, np.bincount(rows, minlength=R), s


def sgd_fp32_error(w_abs, lr, g_abs_sum, count):
    """E of the fp32 SGD update x = w - lr * (g_1 + ... + g_n): n - 1 additions, one product, one subtraction, each
    within 2^-24 relative of its exact result -- (n + 2) 2^-24 (|w| + lr sum_j |g_j|) to first order"""
    n = np.asarray(count, np.float64).reshape(-1, 1)
    return (n + 2) * U32 * (np.asarray(w_abs, np.float64) + lr * np.asarray(g_abs_sum, np.float64))


def update_bound(x64, E, dtype: torch.dtype):
    u = UNIT_ROUNDOFF[dtype]
    b = u * np.abs(x64) + (1 + u) * np.asarray(E, np.float64)
    if dtype == torch.float16:
        b = b + 2.0 ** -25
    return b


def sgd_step_nearest(W16: torch.Tensor, rows, grads32, lr) -> None:
    """the reference update of a torch-CPU 16-bit table, in place, for rows looked up ONCE per step (the fp32 form is
    then free of summation order): W16[r] = cast(fp32(W16[r]) - lr * g)"""
    rows = np.asarray(rows, np.int64)
    assert len(np.unique(rows)) == len(rows)
    w = W16[rows].float().numpy()
    x = (w - np.float32(lr) * np.asarray(grads32, np.float32)).astype(np.float32)
    W16[torch.from_numpy(rows)] = torch.from_numpy(x).to(W16.dtype)
