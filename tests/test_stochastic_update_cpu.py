"""CPU tests of tests/stochastic_update_ref.py, the reference tests/test_gpu_stochastic_adagrad.py holds the
stochastically rounded row-wise Adagrad update of a 16-bit table to: known answers of the hash, the layout of the random
bits, exactness of the exact construction (in rational arithmetic), the decidable prediction against a numpy fp32 model
of the update, the 1 % cap on undecided elements for the inputs of every standard-normal GPU case, and -- the point of
it all -- that the GPU tests' comparisons reject a model that is wrong in one place."""
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import fused_update_cases as fc  # noqa: E402
import stochastic_update_ref as sref  # noqa: E402
import table_dtype_ref as tref  # noqa: E402

W16 = [torch.bfloat16, torch.float16]
IDS = lambda d: sref.NAMES[d]  # noqa: E731


def test_mix64_known_answers():
    """SplitMix64's first two outputs for seed 0"""
    assert int(sref.mix64(0)[0]) == 0xE220A8397B1DCDAF
    assert int(sref.mix64(0x9E3779B97F4A7C15)[0]) == 0x6E789E6AA1B965F4
    both = sref.mix64(np.array([0, 0x9E3779B97F4A7C15], np.uint64))
    assert [int(v) for v in both] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]
    assert int(sref.mix64(-1)[0]) == int(sref.mix64(2 ** 64 - 1)[0]), "a negative row is its two's complement"


def test_random_bits_follow_the_specification():
    """one element spelled out with Python integers: seed 11, call 2, row 7, element 9 = field 1 of chunk 2"""
    M = 2 ** 64 - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    step_key = mix((11 + 0xD6E8FEB86659FD93 * 2) & M)
    h = mix((mix(step_key ^ 7) + 2) & M)
    bits = sref.random_bits(11, 2, [3, 7], 16)
    assert bits.dtype == np.uint32 and bits.shape == (2, 16)
    assert int(bits[1, 9]) == (h >> 16) & 0xffff and int(bits[1, 8]) == h & 0xffff and int(bits[1, 11]) == h >> 48
    neg = mix((mix(step_key ^ (M - 0)) + 0) & M)                          # row -1
    assert int(sref.random_bits(11, 2, [-1], 8)[0, 2]) == (neg >> 32) & 0xffff


def test_random_bits_are_distinct_per_row_counter_and_seed():
    a = sref.random_bits(11, 1, [5], 128)
    for other in (sref.random_bits(11, 1, [6], 128), sref.random_bits(11, 2, [5], 128),
                  sref.random_bits(12, 1, [5], 128)):
        assert (a != other).mean() > 0.99
    two = sref.random_bits(11, 1, [5, 6], 128)
    assert np.array_equal(two[0], a[0]) and (two[0] != two[1]).mean() > 0.99


def test_random_bits_do_not_depend_on_the_row_length():
    """element e is a function of (e // 4, e % 4) only: no lane shape enters"""
    rows = [0, 3, 1999, -1]
    wide = sref.random_bits(5, 3, rows, 1024)
    for D in (8, 128, 512, 768):
        assert np.array_equal(sref.random_bits(5, 3, rows, D), wide[:, :D])
    # uniform enough to be random bits at all: every one of the 16 bits is set about half the time
    share = [float(((wide >> b) & 1).mean()) for b in range(16)]
    assert all(abs(s - 0.5) <= 6 * np.sqrt(0.25 / wide.size) for s in share), share
    assert int(wide.max()) < 2 ** 16


@pytest.mark.parametrize("p", sref.P_EXACT)
@pytest.mark.parametrize("wt", W16, ids=IDS)
def test_exact_case_is_exact(wt, p):
    """every intermediate of the step, in rational arithmetic, is an fp32 value (so no rounding can occur, in any order
    of the sums), and the result lies between 1.0 and the next value of the type at p of the way"""
    c = sref.exact_case(wt, p)

    def is_fp32(q: Fraction) -> bool:
        return Fraction(float(np.float32(float(q)))) == q and Fraction(float(q)) == q

    lr, eps, gsum = Fraction(c.lr), Fraction(c.EPS), Fraction(c.GSUM)
    assert lr == 2 * Fraction(p) * Fraction(c.step) and all(is_fp32(q) for q in (lr, eps, gsum, gsum / 2))
    for D in fc.VEC_D:
        sq = gsum * gsum
        # the partial sums of the squares, whatever their order, are k * 2^-20 with k <= D <= 1024
        assert all(is_fp32(k * sq) for k in range(1, D + 1))
        m = D * sq / D
        assert m == Fraction(c.M) and is_fp32(m)
        root = Fraction(2) ** -10
        assert root * root == m
        den = root + eps
        assert den == Fraction(2) ** -9 and is_fp32(den)
        mult = lr / den
        assert mult == 512 * lr and is_fp32(mult)
        x = 1 - gsum * mult
        assert x == 1 + Fraction(p) * Fraction(c.step) == Fraction(c.x) and is_fp32(x)
    # the gradient rows: a row looked up twice gets two halves, whose sum is exact
    ids = np.array([3, 1, 3, -1, 0])
    g = c.grads(ids, 8)
    assert g.dtype == np.float32 and g.shape == (5, 8)
    assert (g[[0, 2]] == np.float32(c.GSUM / 2)).all() and (g[[1, 4]] == np.float32(c.GSUM)).all()
    # and the numpy fp32 model of the kernel, which rounds wherever a kernel would, reproduces the expectation
    rmap = np.array([9, 4, 7, 2], np.int32)
    w = torch.ones(4, 8, dtype=wt)
    out, mom = sref.model_step(wt, w, np.zeros(12, np.float32), ids, g, rmap, c.lr, c.EPS, 11, 1)
    share, n = sref.check_exact(c, out, mom, w, ids, rmap, 11, 1)
    assert n == 3 * 8 and mom[[9, 4, 2]].tolist() == [c.M] * 3 and mom.sum() == np.float32(3 * c.M)


SPECIAL = {torch.bfloat16: [0x7fc0, 0x7f80, 0xff80, 0x0000, 0x8000, 0x7f7f, 0xff7f, 0x0001, 0x3f80],
           torch.float16: [0x7e00, 0x7c00, 0xfc00, 0x0000, 0x8000, 0x7bff, 0xfbff, 0x0001, 0x83ff, 0x3c00]}


def special_rows(wt, D):
    """rows of NaN, +-inf, +-0, +- the largest finite value (65504 for fp16), subnormals and 1.0, one value per row"""
    pat = np.array(SPECIAL[wt], np.uint16).astype(np.int16)
    return torch.from_numpy(np.repeat(pat[:, None], D, axis=1).copy()).view(wt)


@pytest.mark.parametrize("wt", W16, ids=IDS)
def test_a_zero_gradient_keeps_every_representable_value(wt):
    D = 8
    w = special_rows(wt, D)
    R = w.shape[0]
    ids = np.arange(R)
    for mom0 in (0.0, 0.37):
        out, mom = sref.model_step(wt, w, np.full(R, mom0, np.float32), ids, np.zeros((R, D), np.float32),
                                   np.arange(R), 0.05, 1e-8, 5, 1)
        a, b = sref.bits16(out), sref.bits16(w)
        nan = torch.isnan(w.float()).numpy()
        assert np.array_equal(a[~nan], b[~nan]) and torch.isnan(out.float()).numpy()[nan].all()
        assert (mom == np.float32(mom0)).all()
        want, decided = sref.predict(w, np.zeros((R, D), np.float32), mom, 0.05, 1e-8, sref.random_bits(5, 1, ids, D), wt)
        ok = decided & ~nan
        assert np.array_equal(sref.bits16(want)[ok], a[ok])
        # (-0 is not decided: -0 + E is +0; the GPU test compares the special rows' bits directly)
        assert decided[sref.bits16(w) == 0x0000].all() and decided[sref.bits16(w) == 0x0001].all()


_TRAJ = {}


def model_trajectory(case):
    """the case's steps under the numpy fp32 model (stochastic, and the nearest twin of every step from the same start),
    computed once: [(old_w, got_w, twin_w, got_m, twin_m, old_m, m64)]"""
    key = (case.dtype, case.form, case.D)
    if key not in _TRAJ:
        w, mom, m64, out = case.weight0, np.zeros(case.MOM_ROWS, np.float32), np.zeros(case.MOM_ROWS), []
        for k in range(fc.STEPS):
            grads = sref.hooked_grad_rows(case.go[k], len(case.ids[k]))
            args = (case.dtype, w, mom, case.ids[k], grads, case.rmap, case.lr, case.EPS, case.seed, k + 1)
            got_w, got_m = sref.model_step(*args)
            twin_w, twin_m = sref.model_step(*args, rounding="nearest")
            g, cnt = case.fold(k)
            m64 = m64.copy()
            m64[case.rmap[cnt > 0]] += (g[cnt > 0].astype(np.float64) ** 2).sum(1) / case.D
            out.append((w, got_w, twin_w, got_m, twin_m, mom, m64))
            w, mom = got_w, got_m
        _TRAJ[key] = out
    return _TRAJ[key]


CASES = sref.normal_cases()
CASE_IDS = [f"{sref.NAMES[c.dtype]}/{c.form}/{c.D}" for c in CASES]


def test_the_normal_cases_are_the_grid():
    assert len(CASES) == 2 * (len(fc.VEC_D) + 1) == 12
    for c in CASES:
        assert c.weight0.shape == (fc.R, c.D) and len(np.unique(c.rmap)) == fc.R and c.rmap.max() < c.MOM_ROWS
        assert not np.array_equal(c.rmap, np.arange(fc.R)), "the map must not be the identity"
        for ids in c.ids:
            cnt = np.bincount(ids[ids >= 0], minlength=fc.R)
            assert ((cnt == 2).sum(), (cnt == 1).sum(), (ids < 0).sum()) == (fc.TWICE, fc.ONCE, fc.PAD)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_undecided_share_is_capped_for_the_gpu_cases_inputs(case):
    """a condition on the inputs, computed from the reference alone (m from the fp64 model of the momentum)"""
    for k, (old_w, _, _, _, _, _, m64) in enumerate(model_trajectory(case)):
        g, cnt = case.fold(k)
        looked = cnt > 0
        rows = case.rmap[looked].astype(np.int64)
        _, decided = sref.predict(old_w[torch.from_numpy(looked)], g[looked], m64[rows].astype(np.float32), case.lr,
                                  case.EPS, sref.random_bits(case.seed, k + 1, rows, case.D), case.dtype)
        share = 1.0 - float(decided.mean())
        assert share <= sref.CAP, (k, share)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_predict_reproduces_the_fp32_model(case):
    """decided elements exactly, and every other assertion of the GPU comparison"""
    z = n = 0.0
    for k, step in enumerate(model_trajectory(case)):
        dz, dn, _ = sref.check_step(case, k, *step[:6])
        z, n = z + dz, n + dn
    assert n > 0 and abs(z) / np.sqrt(n) <= 6


@pytest.mark.parametrize("name", sorted(sref.MUTANTS))
@pytest.mark.parametrize("wt", W16, ids=IDS)
def test_a_wrong_kernel_is_rejected(wt, name):
    """each single mistake fails the exact comparison and the standard-normal comparison the GPU tests use"""
    mutant = sref.MUTANTS[name]
    # the exact construction, 40 slots over 64 host rows, D = 128
    rng = np.random.default_rng(3)
    R, D, seed = fc.R, 128, 11
    ids = sref.lookup_layout(rng, R, fc.TWICE, fc.ONCE, fc.PAD)
    rmap = sref.row_map(rng, R, 64)
    w = torch.ones(R, D, dtype=wt)
    for p in sref.P_EXACT:
        c = sref.exact_case(wt, p)
        args = (wt, w, np.zeros(64, np.float32), ids, c.grads(ids, D), rmap, c.lr, c.EPS, seed, 1)
        out, mom = sref.model_step(*args)
        sref.check_exact(c, out, mom, w, ids, rmap, seed, 1)                      # the right model passes
        out, mom = sref.model_step(*args, **mutant)
        with pytest.raises(AssertionError, match="table rows"):
            sref.check_exact(c, out, mom, w, ids, rmap, seed, 1)
    # standard-normal data
    case = next(c for c in CASES if c.dtype == wt and c.form == "slots" and c.D == 128)
    for k, (old_w, _, twin_w, got_m, twin_m, old_m, _) in enumerate(model_trajectory(case)):
        grads = sref.hooked_grad_rows(case.go[k], len(case.ids[k]))
        bad_w, bad_m = sref.model_step(wt, old_w, old_m, case.ids[k], grads, case.rmap, case.lr, case.EPS, case.seed,
                                       k + 1, **mutant)
        with pytest.raises(AssertionError, match="decided elements"):
            sref.check_step(case, k, old_w, bad_w, twin_w, bad_m, twin_m, old_m)


def test_the_comparisons_see_what_else_can_go_wrong():
    """momentum that differs from the twin's, a moved row that was not looked up, a value two steps from the twin's"""
    case = next(c for c in CASES if c.dtype == torch.bfloat16 and c.form == "slots" and c.D == 8)
    old_w, got_w, twin_w, got_m, twin_m, old_m, _ = model_trajectory(case)[0]
    looked = np.bincount(case.ids[0][case.ids[0] >= 0], minlength=fc.R) > 0
    m = got_m.copy()
    m[case.rmap[looked][0]] = np.nextafter(m[case.rmap[looked][0]], np.float32(1))
    with pytest.raises(AssertionError, match="nearest twin"):
        sref.check_step(case, 0, old_w, got_w, twin_w, m, twin_m, old_m)
    w = got_w.clone()
    w[int(np.nonzero(~looked)[0][0]), 3] += 1
    with pytest.raises(AssertionError, match="not looked up"):
        sref.check_step(case, 0, old_w, w, twin_w, got_m, twin_m, old_m)
    w = got_w.clone().view(torch.int16)
    w[int(np.nonzero(looked)[0][0]), 1] = twin_w.view(torch.int16)[int(np.nonzero(looked)[0][0]), 1] + 2
    with pytest.raises(AssertionError, match="neighbour"):
        sref.check_step(case, 0, old_w, w.view(torch.bfloat16), twin_w, got_m, twin_m, old_m)
    # the frac statistic is what stochastic rounding is: P(up) = the dropped bits / 2^k, over all random integers
    for wt in W16:
        k = tref.DROPPED_BITS[wt]
        x = np.float32(1.0 + 0.3 * sref.STEP[wt])
        frac, valid = sref.frac_up(np.array([float(x)]), wt)
        ups = (sref.apply(np.full(1 << k, x, np.float32), np.arange(1 << k), wt).float().numpy() > x).mean()
        assert valid[0] and abs(ups - frac[0]) <= 2.0 ** -k
