"""GPU tests of row-wise Adagrad with stochastic rounding on a 16-bit table -- what `CachedEmbeddingBag(table_dtype=bf16 /
fp16).set_fused_rowwise_adagrad(lr)` runs by default: `k_rows_apply<f32x4, WT, NCH, true, true>`, two table types times
four lane shapes -- against tests/stochastic_update_ref.py, and of stochastic rounding through the cache module for both
optimizers.  Shapes are the smallest that reach every lane shape (fused_update_cases.VEC_D) on the 40-row layout of
tests/fused_update_cases.py, 256 rows for the share statistics, the 2000 x 32 toy of tests/test_gpu_table_dtype.py for
the cache; the kernels only ever see in-range slots and the documented ignored slot -1.

The first test anchors the reference on a kernel whose bits tests/golden/fused_update_bits.npz already pins (SGD with
stochastic rounding): if it fails, the reference is wrong, not the kernel, and nothing else in this file means anything.
tests/test_stochastic_update_cpu.py shows, without a GPU, that the comparisons used here reject a kernel that keys the
bits by the slot, takes a hash's four fields in another order, reads the counter before it is incremented, rounds to
nearest or always toward zero."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import fused_update_cases as fc  # noqa: E402
import stochastic_update_ref as sref  # noqa: E402
from test_gpu_table_dtype import (B_TOY, LR_TOY, N_TOY, _fp32_fill, _Sr, _toy_batches,  # noqa: E402
                                  _toy_module)

pytestmark = pytest.mark.gpu
W16 = [torch.bfloat16, torch.float16]
IDS = lambda d: "table_" + sref.NAMES[d]  # noqa: E731
GRID_IDS = [f"{form}-{D}" for form, D in sref.GRID]
MOM_ROWS = 64


def _host(*tensors):
    """the tensors on the host, behind a synchronize of its own: a kernel's fault raises there, a copy's fault at the
    copy"""
    torch.cuda.synchronize()
    out = [t.detach().cpu() for t in tensors]
    return out[0] if len(out) == 1 else out


def _workspace_is_clean(ws: torch.Tensor, calls: int) -> None:
    """zero except the step counter behind acc and flags, which counts the calls"""
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws[:-256])) == 0, "the workspace must be left zero-filled"
    assert int(ws[-256:-248].view(torch.int64).item()) == calls and int(torch.count_nonzero(ws[-248:])) == 0


# ---- a. the reference against a pinned kernel: SGD with stochastic rounding ------------------------------------------

class _Sr256(_Sr):
    R = 256


@pytest.mark.parametrize("wt", W16, ids=IDS)
def test_reference_bits_equal_the_pinned_sgd_kernels(wt):
    """x = 1 + p step for every element of 256 x 128, lr = 1: the table must be apply(x, random_bits(...)) bit for bit,
    with and without a permuted row_of_slot, for two seeds and at counters 1 and 2"""
    step = sref.STEP[wt]
    rmap = torch.randperm(_Sr256.R, generator=torch.Generator().manual_seed(2)).to(torch.int32)
    for rm in (None, rmap):
        s = _Sr256(wt, rmap=None if rm is None else rm.cuda())
        rows = np.arange(s.R) if rm is None else rm.numpy()
        for p in (0.25, 0.875):
            s.go.fill_(-p * step)
            x = np.full((s.R, s.D), 1.0 + p * step, np.float32)
            for seed in (11, 12):
                s.reset(zero_ws=True)
                seen = []
                for counter in (1, 2):
                    s.reset()
                    s.call(seed)
                    got = _host(s.w)
                    assert int(s.ws[-256:-248].view(torch.int64).item()) == counter
                    want = sref.apply(x, sref.random_bits(seed, counter, rows, s.D), wt)
                    bad = np.nonzero(sref.bits16(got) != sref.bits16(want))
                    assert bad[0].size == 0, ("the REFERENCE is wrong", rm is not None, p, seed, counter, bad[0][:8])
                    seen.append(got)
                assert not torch.equal(seen[0], seen[1])


# ---- b. row-wise Adagrad, the exact construction ---------------------------------------------------------------------

def _step(w, fused, ids, go, form, R):
    """one forward + fused backward through embedding_bag: one id per bag, hook_features = F, go [nnz / F, F, D]"""
    from cachedembedding_amd.functional import embedding_bag, presort_window
    idx = torch.from_numpy(np.asarray(ids)).cuda()
    nnz = idx.numel()
    offs = torch.arange(nnz + 1, device="cuda")
    pre = None
    if form == "src":
        pre = presort_window(idx.view(1, -1), R, offsets=offs.to(torch.int32), include_last_offset=True,
                             hook_features=fc.F, identity_bags=True)[0]
    w.requires_grad_(True)
    o = embedding_bag(idx, w, offs, mode="sum", include_last_offset=True, hook_features=fc.F, fused_sgd=fused,
                      presorted=pre, masked_indices=True, output_dtype=torch.float32)
    o.backward(go.view_as(o))
    assert w.grad is None                                         # the update happened inside backward
    w.requires_grad_(False)


def _hooked(grads: np.ndarray) -> torch.Tensor:
    """go [nnz / F, F, D] on the device such that lookup j reads grads[j] (the inverse of sref.hooked_grad_rows)"""
    nnz, D = grads.shape
    B = nnz // fc.F
    j = np.arange(nnz)
    go = np.zeros((B * fc.F, D), np.float32)
    go[(j % B) * fc.F + j // B] = grads
    assert np.array_equal(sref.hooked_grad_rows(go.reshape(B, fc.F, D), nnz), grads)
    return torch.from_numpy(go.reshape(B, fc.F, D)).cuda()


class _Exact:
    """the exact construction on R slots that hold distinct host rows of a momentum of MOM_ROWS rows; one looked-up slot
    has row_of_slot = -1 and one row_of_slot >= MOM_ROWS: neither their rows nor any momentum entry may move"""

    def __init__(self, wt, D, R=fc.R, twice=fc.TWICE, once=fc.ONCE, pad=fc.PAD, seed=11):
        rng = np.random.default_rng([R, D])
        self.wt, self.D, self.R, self.seed = wt, D, R, seed
        self.ids = sref.lookup_layout(rng, R, twice, once, pad)
        self.rmap = sref.row_map(rng, R, MOM_ROWS if R <= MOM_ROWS else 2 * R)
        self.mom_rows = MOM_ROWS if R <= MOM_ROWS else 2 * R
        cnt = np.bincount(self.ids[self.ids >= 0], minlength=R)
        self.no_state = (int(np.nonzero(cnt == 2)[0][0]), int(np.nonzero(cnt == 1)[0][0]))
        self.rmap[self.no_state[0]] = -1
        self.rmap[self.no_state[1]] = self.mom_rows + 3
        self.w0 = torch.ones(R, D, dtype=wt)
        self.w = self.w0.clone().cuda()
        self.mom = torch.zeros(self.mom_rows, device="cuda")
        self.rmap_dev = torch.from_numpy(self.rmap).cuda()

    def fused(self, lr):
        from cachedembedding_amd.functional import FusedRowwiseAdagrad
        f = FusedRowwiseAdagrad(lr, eps=sref.ExactCase.EPS, momentum=self.mom, row_of_slot=self.rmap_dev)
        assert f.rounding == "stochastic", "the default this file exists for"
        f.seed = self.seed
        return f

    def reset(self):
        self.w.copy_(self.w0)
        self.mom.zero_()

    def check(self, case, counter):
        got_w, got_m = _host(self.w, self.mom)
        share = sref.check_exact(case, got_w, got_m.numpy(), self.w0, self.ids, self.rmap, self.seed, counter)
        for s in self.no_state:
            assert np.array_equal(sref.bits16(got_w[s]), sref.bits16(self.w0[s])), "a slot without state moved"
        return got_w, share


@pytest.mark.parametrize("form,D", sref.GRID, ids=GRID_IDS)
@pytest.mark.parametrize("wt", W16, ids=IDS)
def test_exact_step_bit_for_bit(wt, form, D):
    e = _Exact(wt, D)
    looked = np.bincount(e.ids[e.ids >= 0], minlength=e.R)
    assert ((looked == 2).sum(), (looked == 1).sum(), (looked == 0).sum(), (e.ids < 0).sum()) == (12, 16, 12, 8)
    for p in sref.P_EXACT:
        case = sref.exact_case(wt, p)
        go = _hooked(case.grads(e.ids, D))
        fused = e.fused(case.lr)
        e.reset()
        _step(e.w, fused, e.ids, go, form, e.R)
        first, _ = e.check(case, 1)
        _workspace_is_clean(fused._ws16, 1)
        e.reset()                                                 # weights and momentum again, the workspace kept
        _step(e.w, fused, e.ids, go, form, e.R)
        second, _ = e.check(case, 2)
        _workspace_is_clean(fused._ws16, 2)
        assert not torch.equal(first, second), "a second call must draw other bits"


@pytest.mark.parametrize("wt", W16, ids=IDS)
def test_exact_step_rounds_up_with_probability_p(wt):
    """256 rows x 128: 76 looked up twice, 104 once, 76 not, 8 ignored lookups; the share of elements that took the
    value above 1.0 is within 6 sigma of p (the bound of test_update_stochastic)"""
    e = _Exact(wt, 128, R=256, twice=76, once=104, pad=8)
    for p in sref.P_EXACT:
        case = sref.exact_case(wt, p)
        fused = e.fused(case.lr)
        e.reset()
        _step(e.w, fused, e.ids, _hooked(case.grads(e.ids, 128)), "slots", e.R)
        _, (share, n) = e.check(case, 1)
        assert n == (76 + 104 - 2) * 128
        print(f"{sref.NAMES[wt]} p={p}: share {share:.5f} of n={n}, bound {6 * np.sqrt(p * (1 - p) / n):.5f}")
        assert abs(share - p) <= 6 * np.sqrt(p * (1 - p) / n), (p, share)


# ---- c. row-wise Adagrad, standard-normal gradients, three steps -----------------------------------------------------

_NORMAL = {}


def _normal_case(wt, form, D):
    """runs the case once per process: every step from the same start with "stochastic" and with "nearest", all of
    check_step's assertions; returns [(sum(up - frac), sum(frac (1 - frac)), undecided share)] per step"""
    from cachedembedding_amd.functional import FusedRowwiseAdagrad
    key = (wt, form, D)
    if key in _NORMAL:
        return _NORMAL[key]
    case = sref.NormalCase(wt, form, D)
    rmap = torch.from_numpy(case.rmap).cuda()
    w, mom = case.weight0.clone().cuda(), torch.zeros(case.MOM_ROWS, device="cuda")
    stoch = FusedRowwiseAdagrad(case.lr, eps=case.EPS, momentum=mom, row_of_slot=rmap)
    assert stoch.rounding == "stochastic"
    stoch.seed = case.seed
    out = []
    for k in range(fc.STEPS):
        old_w, old_m = _host(w, mom)
        twin_w, twin_m = w.clone(), mom.clone()
        near = FusedRowwiseAdagrad(case.lr, eps=case.EPS, momentum=twin_m, row_of_slot=rmap)
        near.rounding = "nearest"
        go = torch.from_numpy(case.go[k]).cuda()
        _step(w, stoch, case.ids[k], go, form, fc.R)
        _step(twin_w, near, case.ids[k], go, form, fc.R)
        got_w, got_m, tw, tm = _host(w, mom, twin_w, twin_m)
        out.append(sref.check_step(case, k, old_w, got_w, tw, got_m.numpy(), tm.numpy(), old_m.numpy()))
        _workspace_is_clean(stoch._ws16, k + 1)
        print(f"{sref.NAMES[wt]}/{form}/{D} step {k}: undecided {out[-1][2]:.5f}")
    _NORMAL[key] = out
    return out


@pytest.mark.parametrize("form,D", sref.GRID, ids=GRID_IDS)
@pytest.mark.parametrize("wt", W16, ids=IDS)
def test_normal_steps_against_the_nearest_twin_and_the_prediction(wt, form, D):
    assert len(_normal_case(wt, form, D)) == fc.STEPS


def test_normal_steps_round_up_as_often_as_they_should():
    """over all steps of the D >= 128 cases: sum(up - frac) / sqrt(sum(frac (1 - frac))) within +-6"""
    z = n = 0.0
    for wt in W16:
        for form, D in sref.GRID:
            if D >= 128:
                for dz, dn, _ in _normal_case(wt, form, D):
                    z, n = z + dz, n + dn
    print(f"sum(up - frac) = {z:.2f}, sqrt(sum(frac (1 - frac))) = {np.sqrt(n):.2f}, ratio {z / np.sqrt(n):.3f}")
    assert n > 1e4 and abs(z) / np.sqrt(n) <= 6


# ---- d. special values -----------------------------------------------------------------------------------------------

SPECIAL = {torch.bfloat16: [0x7fc0, 0x7f80, 0xff80, 0x0000, 0x8000, 0x7f7f, 0xff7f, 0x0001],
           torch.float16: [0x7e00, 0x7c00, 0xfc00, 0x0000, 0x8000, 0x7bff, 0xfbff, 0x0001, 0x83ff]}


@pytest.mark.parametrize("D", [8, 128])
@pytest.mark.parametrize("wt", W16, ids=IDS)
def test_special_values_survive_a_zero_gradient(wt, D):
    """rows of NaN, +-inf, +-0, +- the largest finite value (65504 for fp16) and subnormals, looked up with an all-zero
    gradient: their bits stay (NaN stays NaN), their momentum stays 0; the rows around them follow the exact step"""
    e = _Exact(wt, D)
    case = sref.exact_case(wt, 0.5)
    cnt = np.bincount(e.ids[e.ids >= 0], minlength=e.R)
    free = [s for s in np.nonzero(cnt > 0)[0] if s not in e.no_state]
    special = np.array(free[:len(SPECIAL[wt])])
    assert set(cnt[special]) == {1, 2}, "special rows looked up once and twice"
    pat = np.array(SPECIAL[wt], np.uint16).astype(np.int16)
    e.w0[torch.from_numpy(special)] = torch.from_numpy(np.repeat(pat[:, None], D, axis=1).copy()).view(wt)
    grads = case.grads(e.ids, D)
    grads[np.isin(e.ids, special)] = 0.0
    fused = e.fused(case.lr)
    e.reset()
    _step(e.w, fused, e.ids, _hooked(grads), "slots", e.R)
    got_w, got_m = _host(e.w, e.mom)
    a, b = sref.bits16(got_w[torch.from_numpy(special)]), sref.bits16(e.w0[torch.from_numpy(special)])
    nan = torch.isnan(e.w0[torch.from_numpy(special)].float()).numpy()
    assert nan.sum() == D and np.array_equal(a[~nan], b[~nan]), "a special value moved"
    assert torch.isnan(got_w[torch.from_numpy(special)].float()).numpy()[nan].all(), "NaN must stay NaN"
    assert int(np.count_nonzero(got_m.numpy()[e.rmap[special]])) == 0
    # everything else as in the exact step: the special slots leave the layout
    others = np.where(np.isin(e.ids, special), -1, e.ids)
    keep = torch.ones(e.R, dtype=torch.bool)
    keep[torch.from_numpy(special)] = False
    w_rest, w0_rest = got_w.clone(), e.w0.clone()
    w_rest[~keep], w0_rest[~keep] = 1.0, 1.0
    sref.check_exact(case, w_rest, got_m.numpy(), w0_rest, others, e.rmap, e.seed, 1)
    _workspace_is_clean(fused._ws16, 1)


# ---- e. the learning rate from device memory -------------------------------------------------------------------------

def test_device_learning_rate_gives_the_by_value_bits():
    """ce_bag_backward_update_lrdev with CE_ACC_CACHE: the exact step's bits, bf16 at D = 128"""
    wt, D = torch.bfloat16, 128
    e = _Exact(wt, D)
    case = sref.exact_case(wt, 0.875)
    go = _hooked(case.grads(e.ids, D))
    by_value = e.fused(case.lr)
    e.reset()
    _step(e.w, by_value, e.ids, go, "slots", e.R)
    want, _ = e.check(case, 1)
    lr = torch.tensor([case.lr], dtype=torch.float32, device="cuda")
    from_device = e.fused(lr)
    assert from_device.accumulator == "cache"
    e.reset()
    _step(e.w, from_device, e.ids, go, "slots", e.R)
    got, _ = e.check(case, 1)
    assert np.array_equal(sref.bits16(got), sref.bits16(want))
    _workspace_is_clean(from_device._ws16, 1)


# ---- f. a captured backward ------------------------------------------------------------------------------------------

def test_captured_backward_draws_the_bits_of_consecutive_counters():
    """the C entry captured after a warm-up on a side stream (test_update_stochastic's pattern), bf16 at D = 128: two
    replays from reset weights and momentum equal the predictions for counters 2 and 3"""
    from cachedembedding_amd import _lib
    wt, D = torch.bfloat16, 128
    e = _Exact(wt, D)
    case = sref.exact_case(wt, 0.25)
    ids = torch.from_numpy(e.ids).cuda()
    nnz = ids.numel()
    off = torch.arange(nnz + 1, device="cuda")
    go = torch.from_numpy(case.grads(e.ids, D)).cuda()                 # no hook: bag j reads row j
    ws = torch.zeros(_lib.lib.ce_bag_backward_w16_workspace(e.R, D), dtype=torch.uint8, device="cuda")

    def call():
        _lib.check(_lib.lib.ce_bag_backward_update_w16(
            e.w.data_ptr(), _lib.ACT_DTYPES[wt], e.R, D, ids.data_ptr(), nnz, off.data_ptr(), 1, nnz, 1, None,
            _lib.CE_MODE_SUM, 0, go.data_ptr(), _lib.CE_ACT_F32, None, e.rmap_dev.data_ptr(), e.mom.data_ptr(),
            e.mom_rows, case.lr, case.EPS, _lib.CE_OPT_ROWWISE_ADAGRAD, _lib.CE_ROUND_STOCHASTIC, e.seed,
            ws.data_ptr(), ws.numel(), _lib.stream_ptr()))

    e.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    first, _ = e.check(case, 1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    seen = [first]
    for counter in (2, 3):
        e.reset()
        graph.replay()
        got, _ = e.check(case, counter)
        _workspace_is_clean(ws, counter)
        seen.append(got)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- g. through the cache: residency is invisible --------------------------------------------------------------------

@pytest.mark.parametrize("opt", ["adagrad", "sgd"])
@pytest.mark.parametrize("strategy,transport", [("dataset", "zerocopy"), ("lfu", "worker")])
@pytest.mark.parametrize("wt", W16, ids=IDS)
def test_through_the_cache_stochastic(wt, strategy, transport, opt):
    """30 steps on the 2000 x 32 toy behind a cache of 200 rows that evicts from step 4 on, the module's rounding left at
    its default, against the same steps on the whole 16-bit table on the device with no cache and no row map: the random
    bits follow the host-table row (cached_idx_map[slot]), so the flushed host table and the momentum are the twin's bit
    for bit.  ids are unique within a step, so no sum depends on the order of the atomics."""
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD, embedding_bag
    ids, grads = _toy_batches(30)
    assert all(len(np.unique(i)) == len(i) for i in ids)
    emb = _toy_module(strategy, transport, wt, output_dtype=torch.float32)
    assert emb.weight_rounding == "stochastic"
    if opt == "adagrad":
        emb.set_fused_rowwise_adagrad(LR_TOY)
        twin = FusedRowwiseAdagrad(LR_TOY, momentum=torch.zeros(N_TOY, device="cuda"))
    else:
        emb.set_fused_sgd(LR_TOY)
        twin = FusedSGD(LR_TOY)
    fused = emb._fused()
    assert fused.rounding == twin.rounding == "stochastic" and fused.seed == twin.seed and twin.row_of_slot is None
    assert fused.row_of_slot is emb.cache_weight_mgr.cached_idx_map
    # a third run of the same steps, rounded to nearest: what the table would be if nothing were drawn at all
    near = FusedSGD(LR_TOY)
    if opt == "adagrad":
        near = FusedRowwiseAdagrad(LR_TOY, momentum=torch.zeros(N_TOY, device="cuda"))
    near.rounding = "nearest"
    fill = _fp32_fill().to(wt)
    w, w_near = fill.clone().cuda(), fill.clone().cuda()
    off = torch.arange(B_TOY + 1, device="cuda")
    for i, g in zip(ids, grads):
        idx, go = torch.from_numpy(i).cuda(), torch.from_numpy(g).cuda()
        out = emb(idx, off)
        assert out.dtype == torch.float32
        out.backward(go)
        for table, f in ((w, twin), (w_near, near)):
            table.requires_grad_(True)
            o = embedding_bag(idx, table, off, mode="sum", include_last_offset=True, fused_sgd=f,
                              output_dtype=torch.float32)
            o.backward(go)
            table.requires_grad_(False)
    torch.cuda.synchronize()
    assert sum(emb.num_write_back_history[:3]) == 0 and sum(emb.num_write_back_history[3:]) > 0
    emb.flush()
    want = _host(w)
    bad = np.unique(np.nonzero(sref.bits16(emb.weight) != sref.bits16(want))[0])
    assert bad.size == 0, ("residency must be invisible; host rows", bad[:8])
    if opt == "adagrad":
        got_m, want_m = _host(emb.cache_weight_mgr.momentum1, twin.momentum)
        assert torch.equal(got_m.view(torch.int32), want_m.view(torch.int32))
        assert int(torch.count_nonzero(got_m)) == len(np.unique(np.concatenate(ids)))
    never = np.setdiff1d(np.arange(N_TOY), np.concatenate(ids))
    assert never.size > 0 and np.array_equal(sref.bits16(emb.weight[never]), sref.bits16(fill[never]))
    # and the rounding was stochastic.  One stochastic rounding differs from the nearest one with probability
    # min(f, 1 - f), f the position of x between its neighbours: 1/4 on average for f spread evenly, per step a row
    # takes part in, so at least about a quarter of the looked-up rows' elements differ from the nearest run's (none
    # would if nothing were drawn).  The bound leaves that expectation a wide margin and is not a measurement.
    differ = (sref.bits16(_host(w_near)) != sref.bits16(want))[np.unique(np.concatenate(ids))]
    print(f"share of looked-up elements that differ from the nearest run: {differ.mean():.4f}")
    assert differ.mean() > 0.1, ("the default rounding did not draw anything", float(differ.mean()))
    for f in (fused, twin):
        _workspace_is_clean(f._ws16, 30)
