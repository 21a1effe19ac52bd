"""CPU tests of element-wise Adagrad with its state carried in the row (rows w | h): the numpy model
(tests/adagrad_layout_ref.py) against torch.optim.Adagrad, its fp32 form against its fp64 form on the very inputs the
GPU tests use, the wrong forms the comparison must tell apart, and the refusals of the C entries and of the Python
surface that can be reached without a device."""
import ctypes
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import adagrad_layout_cases as ac  # noqa: E402
import adagrad_layout_ref as ref  # noqa: E402
import adam_cases as cases  # noqa: E402

RTOL, ATOL = ac.RTOL, ac.ATOL
LAYOUT = "adagrad"
LR = 0.05


def _ratio(got, want):
    """max |got - want| / (atol + rtol |want|): above 1 fails assert_allclose"""
    want = np.asarray(want, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - want) / (ATOL + RTOL * np.abs(want))).max())


def _model_run(steps, dtype=np.float64, init_acc=0.0, use_psw=True, **kw):
    W = cases.initial_weight().astype(dtype)
    S = np.full_like(W, dtype(init_acc))
    for t, (ids, off, go, psw) in enumerate(steps, 1):
        rows, grads = ref.lookup_grads(ids, off, go.astype(dtype), cases.N, psw=psw if use_psw else None, dtype=dtype)
        ref.step(W, S, rows, grads, LR, t, dtype=dtype, **kw)
    return W, S


# ---- the reference against torch.optim.Adagrad ---------------------------------------------------------------------

def _torch_run(steps, sparse, lr_decay=0.0, init_acc=0.0, wd=0.0, eps=1e-10):
    """(w, sum) [N, D] of torch.optim.Adagrad after `steps`, fp64; loss = <out, grad_out>"""
    bag = torch.nn.EmbeddingBag(cases.N, cases.D, mode="sum", sparse=sparse, include_last_offset=True,
                                _weight=torch.tensor(cases.initial_weight(), dtype=torch.float64))
    opt = torch.optim.Adagrad(bag.parameters(), lr=LR, lr_decay=lr_decay, weight_decay=wd,
                              initial_accumulator_value=init_acc, eps=eps)
    for ids, off, go, psw in steps:
        opt.zero_grad()
        out = bag(torch.from_numpy(ids), torch.from_numpy(off), per_sample_weights=torch.tensor(psw, dtype=torch.float64))
        (out * torch.tensor(go, dtype=torch.float64)).sum().backward()
        opt.step()
    return bag.weight.detach().numpy(), opt.state[bag.weight]["sum"].numpy()


@pytest.mark.parametrize("lr_decay, init_acc", [(0.0, 0.0), (0.1, 0.0), (0.0, 0.1), (0.05, 0.25)])
def test_fp64_model_equals_torch_adagrad_on_sparse_gradients(lr_decay, init_acc):
    steps = cases.zipf_steps()
    W, S = _model_run(steps, lr_decay=lr_decay, init_acc=init_acc)
    w, s = _torch_run(steps, sparse=True, lr_decay=lr_decay, init_acc=init_acc)
    np.testing.assert_allclose(W, w, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(S, s, rtol=1e-12, atol=1e-12)
    # the row no step names keeps its weight and its initial accumulator
    np.testing.assert_array_equal(W[cases.NEVER], cases.initial_weight()[cases.NEVER].astype(np.float64))
    assert (S[cases.NEVER] == init_acc).all() and (S[:cases.NEVER] != init_acc).any()


def _dense_steps(seed=31, steps=6):
    """every step names every row (torch refuses weight_decay with sparse gradients, and a dense gradient decays every
    row: the two agree where every row is named)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        ids = np.concatenate([np.arange(cases.N), rng.integers(0, cases.N, 32)])[rng.permutation(cases.N + 32)]
        cuts = np.sort(rng.integers(0, len(ids) + 1, 15))
        off = np.concatenate([[0], cuts, [len(ids)]]).astype(np.int64)
        go = rng.standard_normal((len(off) - 1, cases.D)).astype(np.float32)
        out.append((ids.astype(np.int64), off, go, rng.uniform(0.5, 1.5, len(ids)).astype(np.float32)))
    return out


@pytest.mark.parametrize("lr_decay, init_acc", [(0.0, 0.0), (0.1, 0.1)])
def test_fp64_model_equals_torch_adagrad_with_l2_decay_on_dense_gradients(lr_decay, init_acc):
    steps = _dense_steps()
    W, S = _model_run(steps, lr_decay=lr_decay, init_acc=init_acc, wd=0.01, wd_mode="l2")
    w, s = _torch_run(steps, sparse=False, lr_decay=lr_decay, init_acc=init_acc, wd=0.01)
    np.testing.assert_allclose(W, w, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(S, s, rtol=1e-12, atol=1e-12)
    plain = _model_run(steps, lr_decay=lr_decay, init_acc=init_acc)
    assert _ratio(plain[0], W) > 10                                  # (the decay is no rounding matter)


def test_model_by_hand():
    """the specification's lines on numbers small enough to follow"""
    W0 = np.arange(5 * 4, dtype=np.float64).reshape(5, 4) / 8
    go = np.asarray([[1.0, 2, 3, 4], [0.5, 0, 0, 0], [9, 9, 9, 9]])
    ids, off, psw = [1, -1, 2, 7, 3, 3], [0, 2, 4, 4], [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]
    rows, grads = ref.lookup_grads(ids, off, go, 5, psw=psw)
    assert rows.tolist() == [1, 2]                                   # -1, 7 and the uncovered tail take no part
    W, S = W0.copy(), np.full_like(W0, 0.5)
    ref.step(W, S, rows, grads, 0.1, 3, eps=1e-10, lr_decay=0.5)
    clr = 0.1 / (1 + 2 * 0.5)
    for r in (0, 2, 3, 4):                                           # row 2: g = 0 -- s + 0, w - 0: unchanged bits
        np.testing.assert_array_equal(W[r], W0[r])
        assert (S[r] == 0.5).all()
    np.testing.assert_allclose(S[1], 0.5 + go[0] ** 2, rtol=1e-15)
    np.testing.assert_allclose(W[1], W0[1] - clr * go[0] / (np.sqrt(S[1]) + 1e-10), rtol=1e-15)
    for mode in ("l2", "decoupled"):
        W, S = W0.copy(), np.zeros_like(W0)
        ref.step(W, S, rows, grads, 0.1, 3, lr_decay=0.5, wd=0.5, wd_mode=mode)
        h = go[0] + 0.5 * W0[1] if mode == "l2" else go[0]
        base = W0[1] if mode == "l2" else W0[1] * (1 - clr * 0.5)
        np.testing.assert_allclose(S[1], h * h, rtol=1e-15)
        np.testing.assert_allclose(W[1], base - clr * h / (np.sqrt(h * h) + 1e-10), rtol=1e-14)
    # the clip comes first: the state is fed by the clipped gradient
    W, S = W0.copy(), np.zeros_like(W0)
    ref.step(W, S, rows, grads, 0.1, 1, grad_clip=2.5, clip_mode="value")
    np.testing.assert_allclose(S[1], np.asarray([1.0, 4, 6.25, 6.25]), rtol=1e-15)
    # eps == 0 on a zero state: 0 / 0, as in torch
    W, S = W0.copy(), np.zeros_like(W0)
    with np.errstate(invalid="ignore"):
        ref.step(W, S, np.asarray([2]), np.zeros((1, 4)), 0.1, 1, eps=0.0)
    assert np.isnan(W[2]).all() and not np.isnan(W[1]).any()
    # the fp32 form rounds the rate once, from the fp64 quotient
    clr_d, clr = ref.rate(0.1, 4, 0.3, np.float32)
    assert clr_d == float(np.float32(0.1)) / (1.0 + 3 * 0.3) and clr == np.float32(clr_d) and clr.dtype == np.float32


# ---- the tolerance of the GPU tests, vetted on their inputs: the fp32 reference alone keeps HALF of it ---------------

@pytest.mark.parametrize("case", list(ac.MODEL_CASES))
@pytest.mark.parametrize("D", ac.DIMS)
def test_fp32_model_keeps_half_the_tolerance_on_the_kernel_tests_inputs(D, case):
    kw = ac.MODEL_CASES[case]
    for src in (False, True):
        steps = ac.kernel_steps(D, src, seed=D)
        W0 = ac.initial_weight(D, D)
        want = ac.model(W0, steps, np.float64, **kw)
        got = ac.model(W0, steps, np.float32, **kw)
        assert not want[2][ac.R - 5:].any() and want[2][ac.R - 20:ac.R - 5].any() and want[2][ac.HOT]
        for name, g, w in zip("ws", got, want):
            r = _ratio(g, w)
            print(f"D={D} src={src} {case} {name}: fp32 model, max |err| / (atol + rtol |ref|) = {r:.3g}")
            assert r <= 0.5, (name, r)


def test_row_norm_threshold_takes_both_sides_in_every_step():
    from adam_ref import fold
    from grad_clip_ref import clipped_mask
    for D in (4, 192):
        for s in ac.kernel_steps(D, False, seed=D):
            rows, grads = ref.lookup_grads(s["ids"], s["off"], s["go"].astype(np.float64), ac.R, mode=s["mode"],
                                           psw=s["psw"], hook_features=s["hook"])
            mask = clipped_mask(fold(rows, grads, D)[1], ac.row_norm_threshold(D), "row_norm")
            assert mask.any() and not mask.all()


# ---- the comparison rejects plausible mistakes: each moves the model by more than ten times the tolerance ------------

WRONG_SETTINGS = {
    "s_from_unclipped": dict(clip_mode="row_norm"),
    "f_from_lr": dict(wd=ac.WD, wd_mode="decoupled", lr_decay=ac.LR_DECAY),
    "t_off_by_one": dict(lr_decay=ac.LR_DECAY),
    "rowwise_s": dict(),
}


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_wrong_forms_are_told_apart(wrong):
    D = 32
    kw = WRONG_SETTINGS[wrong]
    steps = ac.kernel_steps(D, False, seed=D)
    W0 = ac.initial_weight(D, D)
    if wrong == "f_from_lr":
        # (f differs from the right one by (lr - clr) wd: with wd = 0.01 that is a few 1e-5 of w per step, so the
        # mistake is shown where the decay is large enough to matter at all)
        kw = dict(kw, wd=0.5)
    want = ac.model(W0, steps, np.float64, **kw)
    got = ac.model(W0, steps, np.float64, wrong=wrong, **kw)
    r = max(_ratio(got[0], want[0]), _ratio(got[1], want[1]))
    print(f"{wrong}: max |err| / (atol + rtol |ref|) = {r:.3g}")
    assert r > 10
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(got[0], want[0], rtol=RTOL, atol=ATOL)


# ---- the C entries, without a GPU: everything is refused before a HIP call ------------------------------------------

def _entries():
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    return _lib, _lib.lib


def _call(lib, src, dim=8, lr_decay=0.0, lr=0.1, eps=1e-10, step=0x1000, acc=0, ws=0x10000, ws_bytes=1 << 30,
          weight=0x2000, nnz=5, num_rows=10, wd=0.0, wd_mode=0, clip=0.0, clip_mode=0):
    """pointers are fake (aligned, never dereferenced: every call here is refused before a launch)"""
    p = ctypes.c_void_p
    tail = (lr_decay, lr, None, eps, wd, wd_mode, clip, clip_mode, p(step) if step else None, acc, p(ws), ws_bytes, None)
    if src:
        return lib.ce_bag_backward_adagrad_src(p(weight), num_rows, dim, nnz, p(0x3000), 0, p(0x4000), *tail)
    return lib.ce_bag_backward_adagrad(p(weight), num_rows, dim, p(0x5000), nnz, p(0x6000), 1, nnz, 1, None, 0, 0,
                                       p(0x3000), 0, None, *tail)


@pytest.mark.parametrize("src", [False, True])
def test_c_entries_refuse_in_the_stated_order(src):
    _lib, lib = _entries()
    bad = _lib.CE_ERR_INVALID
    assert _call(lib, src, step=0, acc=7, lr_decay=-1.0, dim=6) == bad and "step" in _lib.last_error()
    assert _call(lib, src, acc=7, lr_decay=-1.0, dim=6) == bad and "accumulator" in _lib.last_error()
    assert _call(lib, src, wd_mode=9, lr_decay=-1.0) == bad and "weight_decay_mode" in _lib.last_error()
    assert _call(lib, src, wd=-1.0, wd_mode=1, lr_decay=-1.0) == bad and "weight_decay" in _lib.last_error()
    assert _call(lib, src, clip_mode=9, lr_decay=-1.0) == bad and "grad_clip_mode" in _lib.last_error()
    assert _call(lib, src, clip=0.0, clip_mode=1, lr_decay=-1.0) == bad and "grad_clip" in _lib.last_error()
    for d in (-1e-9, float("nan"), -float("inf")):
        assert _call(lib, src, lr_decay=d, eps=-1.0, dim=6) == bad and "lr_decay" in _lib.last_error()
    assert _call(lib, src, eps=-1e-10, lr=-0.1, dim=6) == bad and "eps" in _lib.last_error()
    assert _call(lib, src, lr=-0.1, dim=6) == bad and "lr" in _lib.last_error()
    for dim in (0, 2, 6, 7, 1028, 2048):
        assert _call(lib, src, dim=dim, weight=0, ws_bytes=0) == _lib.CE_ERR_UNSUPPORTED, dim
        assert "dim % 4 == 0" in _lib.last_error()
    assert _call(lib, src, weight=0, ws_bytes=0) == bad and "null" in _lib.last_error()
    assert _call(lib, src, weight=0x2004) == bad and "aligned" in _lib.last_error()
    for acc in (_lib.CE_ACC_CACHE, _lib.CE_ACC_STEP):
        need = lib.ce_bag_backward_adagrad_workspace(10, 5, 8, acc)
        assert need > 0 and need == lib.ce_bag_backward_adam_workspace(10, 5, 8, acc)
        assert _call(lib, src, acc=acc, ws_bytes=need - 1) == bad and "workspace too small" in _lib.last_error()
    assert lib.ce_bag_backward_adagrad_workspace(70, 600, 4, 2) == 0
    assert lib.ce_version() == 6


def test_forward_entries_refuse_as_the_partial_adam_forwards_do():
    _lib, lib = _entries()
    p = ctypes.c_void_p
    for dim in (2, 6, 1028):
        rc = lib.ce_bag_forward_adagrad(p(0x2000), 10, dim, p(0x5000), 5, p(0x6000), 1, 5, 1, None, 0, 0, p(0x3000), 0, None)
        assert rc == _lib.CE_ERR_UNSUPPORTED and "dim % 4 == 0" in _lib.last_error()
        rc = lib.ce_bag_forward_src_keys_adagrad(p(0x2000), 10, dim, 5, p(0x4000), p(0x3000), 0, None)
        assert rc == _lib.CE_ERR_UNSUPPORTED and "dim % 4 == 0" in _lib.last_error()
    rc = lib.ce_bag_forward_adagrad(p(0x2004), 10, 8, p(0x5000), 5, p(0x6000), 1, 5, 1, None, 0, 0, p(0x3000), 0, None)
    assert rc == _lib.CE_ERR_INVALID and "aligned" in _lib.last_error()
    assert lib.ce_bag_forward_adagrad(None, 10, 8, None, 5, None, 1, 5, 1, None, 0, 0, None, 0, None) == _lib.CE_ERR_INVALID


def test_host_fill_is_the_partial_adam_fill_with_the_initial_accumulator():
    _lib, lib = _entries()
    n, d = 37, 12
    pradam = np.full((n, 2 * d), np.nan, np.float32)
    assert lib.ce_host_fill_uniform_pradam(pradam.ctypes.data, n, d, -0.5, 0.25, 1024, 3) == 0
    for init_acc in (0.0, 0.1, 2.5):
        for threads in (1, 5):
            t = np.full((n, 2 * d), np.nan, np.float32)
            assert lib.ce_host_fill_uniform_adagrad(t.ctypes.data, n, d, -0.5, 0.25, 1024, init_acc, threads) == 0
            np.testing.assert_array_equal(t[:, :d], pradam[:, :d])
            assert (t[:, d:] == np.float32(init_acc)).all()
    t = np.zeros((1, 16), np.float32)
    for init_acc in (-0.1, float("nan")):
        assert lib.ce_host_fill_uniform_adagrad(t.ctypes.data, 1, 6, 0.0, 1.0, 1, init_acc, 1) == _lib.CE_ERR_INVALID
        assert "init_acc" in _lib.last_error()
    assert lib.ce_host_fill_uniform_adagrad(t.ctypes.data, 1, 6, 0.0, 1.0, 1, 0.0, 1) == _lib.CE_ERR_UNSUPPORTED


# ---- the Python surface: what is refused before a device is asked for -----------------------------------------------

def test_python_refusals_without_a_device():
    import cachedembedding_amd as ce
    from cachedembedding_amd import _lib
    from cachedembedding_amd.functional import FusedAdagrad
    from cachedembedding_amd.modules import FusedSparseModules
    from cachedembedding_amd.parallel import ParallelCachedEmbeddingBag
    from cachedembedding_amd.tablewise import ParallelCachedEmbeddingBagTablewise
    assert ce.FusedAdagrad is FusedAdagrad and "FusedAdagrad" in ce.__all__
    assert "adagrad" in _lib.LAYOUTS and _lib.LAYOUT_SPAN["adagrad"] == 2
    for dt in (torch.bfloat16, torch.float16, torch.uint8, torch.quint4x2):
        with pytest.raises(NotImplementedError, match="fp32 table"):
            ce.CachedEmbeddingBag(64, 32, fused_optimizer=LAYOUT, table_dtype=dt, cuda_row_num=8)
    for kw in (dict(mode="max"), dict(max_norm=1.0), dict(sparse=True)):
        with pytest.raises(NotImplementedError, match="Adagrad-layout"):
            ce.CachedEmbeddingBag(64, 8, fused_optimizer=LAYOUT, cuda_row_num=8, **kw)
    for dim in (6, 2, 1028):
        with pytest.raises(NotImplementedError, match="embedding_dim % 4 == 0"):
            ce.CachedEmbeddingBag(64, dim, fused_optimizer=LAYOUT, cuda_row_num=8)
    with pytest.raises(ValueError, match="'adagrad'"):               # the message names the new layout
        ce.CachedEmbeddingBag(64, 8, fused_optimizer="rowwise_adagrad", cuda_row_num=8)
    with pytest.raises(ValueError, match="'adagrad'"):
        ce.HostTable.allocate(8, 8, layout="rowwise")
    # the initial accumulator: negative or NaN, or with any other layout
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="initial_accumulator_value"):
            ce.CachedEmbeddingBag(64, 8, fused_optimizer=LAYOUT, cuda_row_num=8, initial_accumulator_value=bad)
    for layout in (None, "adam", "partial_rowwise_adam"):
        with pytest.raises(ValueError, match="initial_accumulator_value"):
            ce.CachedEmbeddingBag(64, 8, fused_optimizer=layout, cuda_row_num=8, initial_accumulator_value=0.1)
    # the sharded and table-wise modules keep refusing in-row layouts
    with pytest.raises(NotImplementedError, match="fused_optimizer='adagrad'"):
        ParallelCachedEmbeddingBag(64, 8, fused_optimizer=LAYOUT, cuda_row_num=8)
    with pytest.raises(NotImplementedError, match="fused_optimizer='adagrad'"):
        ParallelCachedEmbeddingBagTablewise([], 8, fused_optimizer=LAYOUT)
    with pytest.raises(NotImplementedError, match="fused_optimizer='adagrad'"):
        FusedSparseModules([64], 8, fused_optimizer=LAYOUT, use_tablewise_parallel=True)
    # the switch: torch.optim.Adagrad's defaults, its own refusals
    f = FusedAdagrad(0.1)
    assert (f.eps, f.lr_decay, f.accumulator, f.weight_decay, f.grad_clip) == (1e-10, 0.0, "step", 0.0, None)
    assert f.layout == "adagrad" and f.span == 2 and f.step is None
    with pytest.raises(NotImplementedError, match="deterministic"):
        FusedAdagrad(0.1, deterministic=True)
    for kw in (dict(eps=-1e-10), dict(eps=float("nan")), dict(lr_decay=-0.1), dict(lr_decay=float("nan")),
               dict(accumulator="row"), dict(weight_decay=-1.0), dict(weight_decay_mode="l1"), dict(grad_clip=0.0),
               dict(grad_clip=1.0, grad_clip_mode="norm")):
        with pytest.raises(ValueError):
            FusedAdagrad(0.1, **kw)
    with pytest.raises(ValueError):
        FusedAdagrad(torch.zeros(2))                                 # a tensor lr: one fp32 element (check_lr)
    with pytest.raises(NotImplementedError, match="Adagrad-layout rows"):
        f.check(torch.zeros(4, 9))
    with pytest.raises(NotImplementedError, match="Adagrad-layout rows"):
        f.check(torch.zeros(4, 16, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="embedding_dim % 4 == 0"):
        f.check(torch.zeros(4, 12))                                  # D = 6
    with pytest.raises(ValueError, match="lr="):
        FusedAdagrad(-0.1).check(torch.zeros(4, 16))
    with pytest.raises(ValueError, match="step count"):
        f.check(torch.zeros(4, 16))                                  # no step tensor
    FusedAdagrad(None).check(torch.zeros(4, 16))                     # lr=None: the forward alone needs no step count


def _stub(layout, no_weight_decay=None):
    """what the set_fused_* / load_* methods look at before they reach the library"""
    return types.SimpleNamespace(fused_optimizer=layout, table_dtype=torch.float32, mode="sum", num_embeddings=9,
                                 embedding_dim=8, _no_weight_decay=no_weight_decay)


def test_layouts_refuse_each_others_updates():
    import cachedembedding_amd as ce
    E = ce.CachedEmbeddingBag
    a = _stub(LAYOUT)
    for call in (lambda: E.set_fused_sgd(a, 0.1), lambda: E.set_fused_rowwise_adagrad(a, 0.1)):
        with pytest.raises(NotImplementedError, match=r"Adagrad-layout module \(fused_optimizer='adagrad'\)"):
            call()
    with pytest.raises(ValueError, match="set_fused_adam needs"):
        E.set_fused_adam(a, 0.1)
    with pytest.raises(ValueError, match="load_adam_state"):
        E.load_adam_state(a, torch.zeros(9, 8), torch.zeros(9, 8), 1)
    for layout in (None, "adam", "partial_rowwise_adam"):
        with pytest.raises(ValueError, match="set_fused_adagrad needs"):
            E.set_fused_adagrad(_stub(layout), 0.1)
        with pytest.raises(ValueError, match="load_adagrad_state needs"):
            E.load_adagrad_state(_stub(layout), torch.zeros(9, 8), 1)
        with pytest.raises(AttributeError, match="state_sum"):
            E.state_sum.fget(_stub(layout))
    with pytest.raises(AttributeError):
        E.exp_avg.fget(a)
    # the Adam layouts go on refusing as before
    with pytest.raises(NotImplementedError, match="Adam-layout"):
        E.set_fused_sgd(_stub("adam"), 0.1)
    # set_fused_adagrad's own argument checks come before the switch is touched
    for kw in (dict(lr=-0.1), dict(lr=0.1, weight_decay=-1.0), dict(lr=0.1, grad_clip=-1.0)):
        with pytest.raises(ValueError):
            E.set_fused_adagrad(a, **kw)
    with pytest.raises(NotImplementedError, match="ce_rows_axpy"):
        E.set_fused_adagrad(_stub(LAYOUT, "a sharded module"), 0.1, weight_decay=0.1)


def test_load_adagrad_state_checks_shapes_before_it_flushes():
    import cachedembedding_amd as ce
    E = ce.CachedEmbeddingBag
    a = _stub(LAYOUT)                                                # (no flush attribute: reaching it would raise)
    for bad in (torch.zeros(9, 4), torch.zeros(8, 8), torch.zeros(9), torch.zeros(9, 16)):
        with pytest.raises(ValueError, match="state_sum must be"):
            E.load_adagrad_state(a, bad, 1)
    with pytest.raises(ValueError, match="step="):
        E.load_adagrad_state(a, torch.zeros(9, 8), -1)


def test_host_table_state_round_trip():
    import cachedembedding_amd as ce
    n, d = 9, 8
    rng = np.random.default_rng(2)
    # (HostTable.allocate needs a device for its pinned memory: the same object over plain host memory)
    t = ce.HostTable(torch.zeros(n, 2 * d), 0, 0, registered=False, layout=LAYOUT, init_acc=0.25)
    assert t.span == 2 and t.init_acc == 0.25
    w = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32))
    s = torch.from_numpy(rng.random((n, d)).astype(np.float32))
    t.set_weight_(w.double())                                        # (another dtype is cast)
    assert torch.equal(t.tensor[:, :d], w) and (t.tensor[:, d:] == 0.25).all()
    t.set_state_sum_(s.double())
    assert torch.equal(t.tensor[:, :d], w) and torch.equal(t.tensor[:, d:], s)
    with pytest.raises(AssertionError):
        t.set_state_sum_(s[:, :4])
    with pytest.raises(AssertionError):
        t.set_moments_(s)                                            # Adam's moments: not this layout's
    with pytest.raises(AssertionError):
        ce.HostTable(torch.zeros(n, 2 * d), 0, 0, registered=False, layout="partial_rowwise_adam").set_state_sum_(s)
    for layout, bad in ((LAYOUT, -1.0), (LAYOUT, float("nan")), (None, 0.5), ("adam", 0.5)):
        with pytest.raises(ValueError, match="init_acc"):
            ce.HostTable(torch.zeros(n, 6 * d), 0, 0, registered=False, layout=layout, init_acc=bad)


def test_example_parses_the_flag_and_keeps_it_exclusive():
    import importlib
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "examples"))
    dm = importlib.import_module("dlrm_main")
    a = dm.parse_args(["--use_cache", "--adagrad_elementwise"])
    assert a.adagrad_elementwise and not a.adagrad and dm._fused_optimizer(a) == LAYOUT
    assert dm._fused_optimizer(dm.parse_args(["--use_cache", "--adam"])) == "adam"
    assert dm._fused_optimizer(dm.parse_args(["--use_cache", "--adagrad"])) is None
    for other in (["--adagrad"], ["--adam"], ["--adam", "--adam_partial_rowwise"], ["--fused_sgd"]):
        with pytest.raises(ValueError, match="--adagrad_elementwise takes the place"):
            dm.main(["--use_cache", "--adagrad_elementwise"] + other)
    with pytest.raises(NotImplementedError, match="--table_dtype fp32"):
        dm.main(["--use_cache", "--adagrad_elementwise", "--table_dtype", "bf16"])
    with pytest.raises(NotImplementedError, match="one process"):
        dm.main(["--use_cache", "--adagrad_elementwise", "--use_tablewise"])
    # the decay and the clip are taken with it (checked before a device is touched), and refused for what they are
    dm.check_embed_weight_decay(dm.parse_args(["--use_cache", "--adagrad_elementwise", "--embed_weight_decay", "0.01"]))
    dm.check_embed_grad_clip(dm.parse_args(["--use_cache", "--adagrad_elementwise", "--embed_grad_clip", "1.0"]))
    dm.check_step_accumulator(dm.parse_args(["--use_cache", "--adagrad_elementwise", "--step_accumulator"]))
    with pytest.raises(ValueError, match="weight_decay"):
        dm.main(["--use_cache", "--adagrad_elementwise", "--embed_weight_decay", "-1"])


def test_the_new_signatures_leave_row_wise_adagrads_alone():
    """(the new entries' ctypes list has a name of its own: the row-wise Adagrad entries keep their 15 / 25 arguments)"""
    from cachedembedding_amd import _lib
    assert len(_lib.SIGNATURES["ce_bag_backward_rowwise_adagrad_src_act"][1]) == 15
    assert len(_lib.SIGNATURES["ce_bag_backward_rowwise_adagrad_act"][1]) == 23
    assert len(_lib.SIGNATURES["ce_bag_backward_adagrad_src"][1]) == 20
    assert len(_lib.SIGNATURES["ce_bag_backward_adagrad"][1]) == 28
