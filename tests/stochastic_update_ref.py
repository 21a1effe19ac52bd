"""Reference of the stochastically rounded fused updates of a 16-bit table (include/ce_api.h, the 16-bit table section;
DESIGN.md 3.5 "Arithmetic identity"), written from that specification in numpy: the random bits, the decidable
prediction of a row-wise Adagrad step, a construction in which a step is exact, the inputs of the GPU cases and the
comparisons tests/test_gpu_stochastic_adagrad.py applies -- which tests/test_stochastic_update_cpu.py feeds wrong models
to.  Test infrastructure only; the rounding itself is tests/table_dtype_ref.py's `stochastic_round`.

Random bits.  mix64 is SplitMix64's step.  With `counter` the number of update calls on the workspace, this one included,
    step_key = mix64(seed + 0xD6E8FEB86659FD93 * counter)
    row_key  = mix64(step_key ^ uint64(r))          r = row_of_slot[slot], or the slot without a map
    element e of the row: bits 16 * (e % 4) .. of mix64(row_key + e // 4); the low 16 (bf16) / 13 (fp16) of them count.
Prediction.  Row-wise Adagrad computes x = w - g * mult, mult = lr / (sqrt(m) + eps), in fp32 with one fused
multiply-add.  From the exact inputs -- the old 16-bit row w, the fp32 fold g, the fp32 momentum m AFTER the step -- the
fp64 value of x is within E = 2^-24 |x| + 6 * 2^-24 |g * mult| of the device's: one rounding of the fma, and three fp32
roundings inside mult (sqrt, add, divide), each at most 2^-23 even if only faithfully rounded.  An element is DECIDED
when x - E, x and x + E round to the same 16-bit value under the element's random bits; nothing here emulates an fp32
fma or depends on how a device rounds its division."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import fused_update_cases as fc  # noqa: E402
import table_dtype_ref as tref  # noqa: E402

GOLDEN, STEP_MUL = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93
STEP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}          # spacing of the type above 1.0
NAMES = {torch.bfloat16: "bf16", torch.float16: "fp16"}
U24 = 2.0 ** -24
CAP = 0.01                                                             # undecided share of the looked-up elements
P_EXACT = (0.25, 0.5, 0.875)
# (form, D) of the exact and of the standard-normal cases: every vector lane shape from slots, source-row keys at 128
GRID = [("slots", D) for D in fc.VEC_D] + [("src", 128)]


# ---- the random bits -------------------------------------------------------------------------------------------------

def _u64(x) -> np.ndarray:
    """x (Python ints of any sign, or an integer array) as a uint64 array of at least one dimension, modulo 2^64"""
    if isinstance(x, (int, np.integer)):
        return np.array([int(x) & (2 ** 64 - 1)], np.uint64)
    x = np.asarray(x)
    return np.atleast_1d(x if x.dtype == np.uint64 else x.astype(np.int64).view(np.uint64))


def mix64(x) -> np.ndarray:
    """SplitMix64's step on uint64, element by element (arrays wrap modulo 2^64)"""
    x = _u64(x) + np.uint64(GOLDEN)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def random_bits(seed: int, counter: int, rows, D: int) -> np.ndarray:
    """uint32 [len(rows), D]: the 16-bit field of every element of the rows `rows` (host-table rows, negative ones as
    their two's complement) in update call `counter` of a workspace"""
    assert D % 4 == 0
    step_key = mix64(_u64(seed) + np.uint64(STEP_MUL) * _u64(counter))
    row_key = mix64(step_key ^ _u64(np.asarray(rows, np.int64)))
    h = mix64(row_key[:, None] + np.arange(D // 4, dtype=np.uint64)[None, :])
    fields = (h[:, :, None] >> (np.uint64(16) * np.arange(4, dtype=np.uint64))) & np.uint64(0xffff)
    return fields.reshape(len(row_key), D).astype(np.uint32)


def apply(x32, bits, dtype: torch.dtype) -> torch.Tensor:
    """the fp32 values x32 rounded stochastically to `dtype` with the random bits `bits`"""
    return tref.stochastic_round(np.asarray(x32, np.float32), bits, dtype)


def bits16(t: torch.Tensor) -> np.ndarray:
    """the bit patterns of a 16-bit tensor, int16 -> int32 without sign extension"""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.int32) & 0xffff


# ---- the decidable prediction ----------------------------------------------------------------------------------------

def exact_x(w16: torch.Tensor, g32, m32, lr, eps):
    """(x, E) in fp64 of a row-wise Adagrad step: w16 [n, D] the old rows, g32 [n, D] the fp32 fold, m32 [n] the fp32
    momentum after the step; lr and eps as the fp32 values the kernel is handed"""
    w = w16.detach().cpu().double().numpy()
    g = np.asarray(g32, np.float32).astype(np.float64)
    m = np.asarray(m32, np.float32).astype(np.float64).reshape(-1, 1)
    mult = float(np.float32(lr)) / (np.sqrt(m) + float(np.float32(eps)))
    with np.errstate(invalid="ignore"):
        x = w - g * mult
        E = U24 * np.abs(x) + 6 * U24 * np.abs(g * mult)
    return x, E


def predict(w16: torch.Tensor, g32, m32, lr, eps, bits, dtype: torch.dtype):
    """(rows of `dtype` [n, D], decided bool [n, D]): the step's result wherever it does not depend on the fp32
    evaluation's error, i.e. where x - E, x and x + E round alike"""
    x, E = exact_x(w16, g32, m32, lr, eps)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, mid, hi = (apply((x + s * E).astype(np.float32), bits, dtype) for s in (-1.0, 0.0, 1.0))
    decided = (bits16(lo) == bits16(mid)) & (bits16(mid) == bits16(hi))
    return mid, decided


def frac_up(x64, dtype: torch.dtype):
    """(frac, valid): the position of the fp64 values x between their two 16-bit neighbours in magnitude -- the
    probability of the one farther from zero --, valid where x is not representable and stochastic rounding applies"""
    x32 = np.asarray(x64, np.float64).astype(np.float32)
    lo, hi = tref.neighbours(x32, dtype)
    lo, hi = np.abs(lo.astype(np.float64)), np.abs(hi.astype(np.float64))
    mag = np.abs(x32).view(np.uint32)
    valid = (hi > lo) & np.isfinite(hi)
    if dtype == torch.float16:
        valid &= (mag >= np.uint32(0x38800000)) & (mag < np.uint32(0x477fe000))
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.clip((np.abs(x64) - lo) / (hi - lo), 0.0, 1.0)
    return np.where(valid, frac, 0.0), valid


# ---- lookups ---------------------------------------------------------------------------------------------------------

def lookup_layout(rng, R: int, twice: int, once: int, pad: int) -> np.ndarray:
    """ids of one step in random order: `twice` rows looked up twice, `once` rows once, `pad` ignored lookups (-1); the
    remaining rows are not looked up (fused_update_cases' layout at R = 40: 12, 16, 8)"""
    assert twice + once <= R and (2 * twice + once + pad) % fc.F == 0
    perm = rng.permutation(R)
    ids = np.concatenate([perm[:twice], perm[:twice], perm[twice:twice + once], np.full(pad, -1)])
    return ids[rng.permutation(len(ids))]


def hooked_grad_rows(go: np.ndarray, nnz: int) -> np.ndarray:
    """[nnz, D]: the gradient row of every lookup j of a one-id-per-bag layout with hook_features = F: bag j = f * B + b
    reads row [b, f] of the incoming gradient go [B, F, D]"""
    B = nnz // fc.F
    j = np.arange(nnz)
    return go.reshape(B * fc.F, -1)[(j % B) * fc.F + j // B]


def fold32(ids, grads, R: int):
    """(g fp32 [R, D], count [R]) of the step: ignored lookups apart, a row's gradient rows added in fp32 -- free of
    order while no row is looked up more than twice"""
    ids = np.asarray(ids)
    ok = ids >= 0
    cnt = np.bincount(ids[ok], minlength=R)
    assert cnt.max() <= 2
    g = np.zeros((R, grads.shape[1]), np.float32)
    np.add.at(g, ids[ok], np.asarray(grads, np.float32)[ok])
    return g, cnt


def row_map(rng, R: int, momentum_rows: int) -> np.ndarray:
    """int32 [R]: distinct host-table rows in [0, momentum_rows) for the R slots"""
    return rng.permutation(momentum_rows)[:R].astype(np.int32)


# ---- the exact construction ------------------------------------------------------------------------------------------

class ExactCase:
    """One row-wise Adagrad step in which every operation is exact.  w = 1.0 everywhere, momentum 0, eps = 2^-10; every
    gradient element of a looked-up row sums to -2^-10 (two lookups of -2^-11 for a row looked up twice); lr = 2 p step.
    Then ss / D = 2^-20 = m, sqrt(m) + eps = 2^-9, mult = 512 lr and x = 1 + p step: all representable in fp32 at every
    D <= 1024 and whatever the order of the sums.  The row becomes apply(1 + p step, bits), the momentum 2^-20."""
    EPS, GSUM, M = 2.0 ** -10, -2.0 ** -10, 2.0 ** -20

    def __init__(self, dtype: torch.dtype, p: float):
        self.dtype, self.p, self.step = dtype, p, STEP[dtype]
        self.lr = 2 * p * self.step
        self.x = 1.0 + p * self.step

    def grads(self, ids, D: int) -> np.ndarray:
        """fp32 [len(ids), D]: the gradient row of every lookup (of the ignored ones too: nothing reads them)"""
        ids = np.asarray(ids)
        cnt = np.bincount(ids[ids >= 0])
        per = np.where(ids >= 0, self.GSUM / np.maximum(cnt[np.maximum(ids, 0)], 1), self.GSUM)
        return np.repeat(per.astype(np.float32)[:, None], D, axis=1)

    def expected(self, seed: int, counter: int, host_rows, D: int) -> torch.Tensor:
        """the updated rows [len(host_rows), D] of slots that hold the host-table rows `host_rows`"""
        x = np.full((len(host_rows), D), self.x, np.float32)
        return apply(x, random_bits(seed, counter, host_rows, D), self.dtype)


def exact_case(dtype: torch.dtype, p: float) -> ExactCase:
    return ExactCase(dtype, p)


def check_exact(case: ExactCase, got_w: torch.Tensor, got_m, old_w: torch.Tensor, ids, rmap, seed: int, counter: int):
    """The assertions of one exact step on a table of R slots: got_w [R, D] and got_m [momentum_rows] after the step,
    old_w before it, rmap int [R] the host row of every slot (-1 or >= momentum_rows: the slot has no state).
    Returns the share of looked-up, updated elements that took the value above 1.0."""
    R, D = got_w.shape
    got_m = np.asarray(got_m, np.float32)
    rmap = np.asarray(rmap, np.int64)
    ids = np.asarray(ids)
    looked = np.zeros(R, bool)
    looked[ids[ids >= 0]] = True
    stateful = (rmap >= 0) & (rmap < len(got_m))
    upd = looked & stateful
    want = old_w.clone()
    want[torch.from_numpy(upd)] = case.expected(seed, counter, rmap[upd], D)
    bad = np.nonzero(bits16(got_w) != bits16(want))
    assert bad[0].size == 0, ("table rows", np.unique(bad[0])[:8], "looked up", looked[np.unique(bad[0])[:8]])
    want_m = np.zeros(len(got_m), np.float32)
    want_m[rmap[upd]] = case.M
    bad = np.nonzero(got_m.view(np.uint32) != want_m.view(np.uint32))[0]
    assert bad.size == 0, ("momentum rows", bad[:8], got_m[bad[:8]])
    up = got_w[torch.from_numpy(upd)].float().numpy() == np.float32(1.0 + case.step)
    return float(up.mean()), int(up.size)


# ---- the standard-normal cases ---------------------------------------------------------------------------------------

class NormalCase:
    """Inputs of one (dtype, form, D) case with standard-normal data: fused_update_cases' R = 40, lr, seed, layout and
    steps.  weight0 the start table, ids[k] / go[k] the lookups and the incoming gradient [nnz / F, F, D] of step k, rmap
    the host row of every slot (a momentum of MOM_ROWS rows)."""
    MOM_ROWS, EPS = 64, 1e-8

    def __init__(self, dtype: torch.dtype, form: str, D: int):
        self.dtype, self.form, self.D = dtype, form, D
        rng = np.random.default_rng([fc.SEED, 16 if dtype == torch.bfloat16 else 13, D, int(form == "src")])
        self.weight0 = torch.from_numpy(rng.standard_normal((fc.R, D)).astype(np.float32)).to(dtype)
        self.rmap = row_map(rng, fc.R, self.MOM_ROWS)
        self.ids = [fc._ids(rng, form) for _ in range(fc.STEPS)]
        self.go = [rng.standard_normal((len(i) // fc.F, fc.F, D)).astype(np.float32) for i in self.ids]
        self.lr, self.seed = fc.LR, fc.SEED

    def fold(self, k: int):
        return fold32(self.ids[k], hooked_grad_rows(self.go[k], len(self.ids[k])), fc.R)


def normal_cases():
    return [NormalCase(dt, form, D) for dt in (torch.bfloat16, torch.float16) for form, D in GRID]


def check_step(case: NormalCase, k: int, old_w, got_w, twin_w, got_m, twin_m, old_m):
    """The assertions of step k (0-based; update call k + 1 of the workspace) of a standard-normal case: old_w the table
    before the step, got_w / got_m after it with stochastic rounding, twin_w / twin_m after the same step from the same
    start with nearest rounding.  Returns (sum(up - frac), sum(frac (1 - frac)), undecided share)."""
    g, cnt = case.fold(k)
    looked = cnt > 0
    got_m, twin_m, old_m = (np.asarray(a, np.float32) for a in (got_m, twin_m, old_m))
    bad = np.nonzero(got_m.view(np.uint32) != twin_m.view(np.uint32))[0]
    assert bad.size == 0, (k, "momentum differs from the nearest twin's at", bad[:8])
    rows = case.rmap[looked].astype(np.int64)
    still = np.setdiff1d(np.arange(len(got_m)), rows)
    assert np.array_equal(got_m[still].view(np.uint32), old_m[still].view(np.uint32)), (k, "momentum of other rows moved")
    sel = torch.from_numpy(looked)
    assert np.array_equal(bits16(got_w[~sel]), bits16(old_w[~sel])), (k, "a row that was not looked up moved")
    # equal to the nearest twin's value or its neighbour: same sign, magnitude patterns 0 or 1 apart
    a, b = bits16(got_w[sel]), bits16(twin_w[sel])
    near = ((a & 0x8000) == (b & 0x8000)) & (np.abs((a & 0x7fff) - (b & 0x7fff)) <= 1)
    assert near.all(), (k, "not the nearest twin's value nor its neighbour", np.argwhere(~near)[:4])
    bits = random_bits(case.seed, k + 1, rows, case.D)
    want, decided = predict(old_w[sel], g[looked], twin_m[rows], case.lr, case.EPS, bits, case.dtype)
    wrong = decided & (a != bits16(want))
    assert not wrong.any(), (k, "decided elements", int(wrong.sum()), "of", int(decided.sum()), np.argwhere(wrong)[:4])
    undecided = 1.0 - float(decided.mean())
    assert undecided <= CAP, (k, "undecided share", undecided)
    x, _ = exact_x(old_w[sel], g[looked], twin_m[rows], case.lr, case.EPS)
    frac, valid = frac_up(x, case.dtype)
    lo, hi = tref.neighbours(x.astype(np.float32), case.dtype)
    up = (bits16(got_w[sel]) & 0x7fff) == (bits16(torch.from_numpy(hi).to(case.dtype)) & 0x7fff)
    return float((up[valid] - frac[valid]).sum()), float((frac[valid] * (1 - frac[valid])).sum()), undecided


# ---- a numpy model of the kernel, right or wrong in one place --------------------------------------------------------

def model_step(dtype, w16, mom, ids, grads, rmap, lr, eps, seed, counter, *, key="row", fields="forward",
               counter_offset=0, rounding="stochastic"):
    """One fused row-wise Adagrad step in numpy fp32: (rows [R, D] of `dtype`, momentum fp32).  The keywords make it
    wrong in one place each: key="slot" (bits keyed by the slot), fields="reversed" (the four 16-bit fields of a hash
    in the opposite order), counter_offset=-1 (the counter read before it is incremented), rounding="nearest" /
    "toward_zero" (always the neighbour toward zero)."""
    R, D = w16.shape
    g, cnt = fold32(ids, grads, R)
    rmap = np.asarray(rmap, np.int64)
    mom = np.array(mom, np.float32)
    upd = np.nonzero((cnt > 0) & (rmap >= 0) & (rmap < len(mom)))[0]
    ss = (g[upd].astype(np.float64) ** 2).sum(1).astype(np.float32)
    m = (mom[rmap[upd]] + ss / np.float32(D)).astype(np.float32)
    mom[rmap[upd]] = m
    mult = (np.float32(lr) / (np.sqrt(m) + np.float32(eps))).astype(np.float32)
    w = w16[torch.from_numpy(upd)].double().numpy()
    with np.errstate(invalid="ignore"):
        x = (w - g[upd].astype(np.float64) * mult.astype(np.float64)[:, None]).astype(np.float32)
    bits = random_bits(seed, counter + counter_offset, rmap[upd] if key == "row" else upd, D)
    if fields == "reversed":
        bits = bits.reshape(len(upd), D // 4, 4)[:, :, ::-1].reshape(len(upd), D)
    if rounding == "nearest":
        new = torch.from_numpy(x).to(dtype)
    elif rounding == "toward_zero":
        new = apply(x, np.zeros_like(bits), dtype)
    else:
        new = apply(x, bits, dtype)
    out = w16.clone()
    out[torch.from_numpy(upd)] = new
    return out, mom


MUTANTS = {"slot_keyed": dict(key="slot"), "fields_reversed": dict(fields="reversed"),
           "counter_one_too_small": dict(counter_offset=-1), "nearest": dict(rounding="nearest"),
           "toward_zero": dict(rounding="toward_zero")}
