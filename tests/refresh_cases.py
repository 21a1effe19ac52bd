"""Inputs of the device quantizer's tests, shared by tests/test_refresh_cpu.py (which pins what the HOST quantizer makes
of the delicate rows, so that the GPU comparison cannot go vacuous) and tests/test_gpu_refresh.py (which holds the
device quantizer to the host's bytes on the same rows).  Everything is seeded; nothing here needs a GPU."""
import numpy as np
import torch

F32 = np.float32
Q8_DIMS = [16, 48, 128, 272, 1024]      # the smallest, an odd number of 16-byte units, the bench's, a partial lane group,
Q4_DIMS = [32, 96, 128, 1024]           # ... the largest with 4 chunks per lane
ROW_COUNTS = [1, 257, 9000]             # a lone group, a ragged last workgroup, several workgroups


def zero_sign_rows(D):
    """[2, D]: [1, +0, -0, 4, ...] and [1, -0, +0, 4, ...] -- the minimum is a zero and the FIRST zero's sign is the
    bias the host stores (every other element is positive)"""
    rows = (np.arange(D) % 7 + 1).astype(F32).reshape(1, D).repeat(2, axis=0)
    rows[0, :4] = [1.0, 0.0, -0.0, 4.0]
    rows[1, :4] = [1.0, -0.0, 0.0, 4.0]
    return rows


def subnormal_rows(D):
    """[2, D]: i * 1e-40f (a subnormal quotient (hi - lo) / 255) and i * 1e-44f (a zero quotient: scale 0, codes 0)"""
    i = np.arange(D).astype(F32)
    return np.stack([(i * F32(1e-40)).astype(F32), (i * F32(1e-44)).astype(F32)])


def special_rows(D):
    """name -> one or more [D] fp32 rows: what a lane reduction, a fast division or a contracted operation gets wrong"""
    i = np.arange(D).astype(F32)
    out = {"constant": np.full((1, D), F32(0.375)), "zero_sign": zero_sign_rows(D), "subnormal": subnormal_rows(D),
           "half_ties": (F32(0.5) * i).reshape(1, D),
           # subnormal once cast to fp16 (6e-8 * i) and to bf16 (1e-39 * i): the exact up-conversion of 16-bit sources
           "w16_subnormal": np.stack([(F32(6.0e-8) * i).astype(F32), (F32(1e-39) * i).astype(F32)]),
           "all_zero": np.stack([np.zeros(D, F32), -np.zeros(D, F32)]),
           "min_last": np.concatenate([np.full(D - 1, F32(2.0)), [F32(-3.0)]]).reshape(1, D)}
    return {k: np.ascontiguousarray(v, F32) for k, v in out.items()}


def drawn_rows(D, n, seed=0):
    """the kinds tests/test_q8_cpu.py draws, n rows in all: normal, the Criteo initialisation's range, a large offset
    with a small spread, two-valued rows, denormal ranges and denormal values"""
    rng = np.random.default_rng(1000 * seed + 7 + D)
    x = rng.standard_normal((n, D)).astype(F32)
    k = np.arange(n) % 6
    x[k == 1] = rng.uniform(-1 / 178e6, 1 / 178e6, (int((k == 1).sum()), D)).astype(F32)
    x[k == 2] = (F32(100) + F32(1e-3) * rng.standard_normal((int((k == 2).sum()), D)).astype(F32)).astype(F32)
    x[k == 3] = np.where(rng.random((int((k == 3).sum()), D)) < 0.5, F32(-2.5), F32(1.25))
    x[k == 4] = (F32(1e-3) + rng.integers(0, 40, (int((k == 4).sum()), D)).astype(F32) * F32(1.4e-45)).astype(F32)
    x[k == 5] = rng.integers(0, 200, (int((k == 5).sum()), D)).astype(F32) * F32(1.4e-45) + F32(1.4e-45)
    return x


def quantizer_input(D, n, seed=0):
    """[n, D] fp32: drawn rows with every special row written over them, spread over the row range (the last row
    included, so the ragged last workgroup holds one); n == 1 is the first zero-sign row"""
    x = drawn_rows(D, n, seed)
    special = np.concatenate(list(special_rows(D).values()))
    if n == 1:
        x[0] = zero_sign_rows(D)[1]
        return x
    pos = np.unique(np.linspace(0, n - 1, len(special)).astype(np.int64))
    x[pos] = special[:len(pos)]
    return x


def as_source(x, dtype):
    """the fp32 fixture as the source tensor of dtype `dtype` (bf16 / fp16: rounded once, to nearest)"""
    return torch.from_numpy(np.ascontiguousarray(x, F32)).to(dtype)


def bad_rows_input(D, n, where, seed=3):
    """[n, D] fp32 with the rows a quantizer refuses: where = {row: kind}, kind one of "nan", "+inf", "-inf", "range"
    (finite elements whose range overflows fp32: +-3e38)"""
    x = drawn_rows(D, n, seed)
    for row, kind in where.items():
        if kind == "range":
            x[row, 0], x[row, D - 1] = F32(3e38), F32(-3e38)
        else:
            x[row, (7 * row) % D] = {"nan": F32(np.nan), "+inf": F32(np.inf), "-inf": F32(-np.inf)}[kind]
    return x


def cache_batches(N, steps, hot=40, seed=19):
    """`steps` batches of 96 ids, 48 bags of 2: 48 distinct ids a batch (24 of `hot` hot ids, 24 of the rest), each
    twice -- a 64-row cache evicts from the second batch on (the stream of tests/test_gpu_q4.py, at another N)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        u = np.concatenate([rng.choice(hot, 24, replace=False), hot + rng.choice(N - hot, 24, replace=False)])
        out.append(rng.permutation(np.concatenate([u, u])))
    return out
