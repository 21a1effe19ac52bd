"""The learning rate from device memory (include/ce_api.h, the ce_*_lrdev entries), as far as it can be
held without a GPU: the four entries exist and are bound; each refuses what its by-value sibling refuses -- same code,
same message, same order, asked of both in this process -- plus a null `lr` and an unknown accumulator, first; the
Python switches refuse a tensor they cannot use when it is set; the example's dense step with a tensor learning rate
follows torch.optim; the trainer's change point is the reference's.

The C calls pass made-up addresses: a call that passes every check reaches its first launch, which fails here
(CE_ERR_HIP).  That is why they run only where nothing could be launched."""
import importlib
import re
import subprocess
import sys
import types
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))

import bag_refusal_cases as bc  # noqa: E402

NAMES = ["ce_bag_backward_sgd_lrdev", "ce_bag_backward_sgd_src_lrdev", "ce_bag_backward_update_lrdev",
         "ce_bag_backward_update_src_lrdev"]
LR_PTR = bc._p(7)
F32, BF16, F16 = 0, 1, 2
SGD, ADAGRAD, NEAREST, STOCH, CACHE, STEP = 0, 1, 0, 1, 0, 1
CE_ERR_INVALID, CE_ERR_UNSUPPORTED = 1, 5

no_gpu = pytest.mark.skipif(torch.cuda.is_available(),
                            reason="passes made-up addresses: only for machines without a GPU")


def test_the_four_entries_are_declared_exported_and_bound():
    from cachedembedding_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ce_api.h").read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (ce_[a-z0-9_]+)", out))
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in exported and n in _lib.SIGNATURES and getattr(_lib.lib, n) is not None
    assert (_lib.CE_ACC_CACHE, _lib.CE_ACC_STEP) == (0, 1) == (CACHE, STEP)
    assert (_lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED) == (CE_ERR_INVALID, CE_ERR_UNSUPPORTED)
    assert _lib.lib.ce_version() == 6


def _answer(_lib, fn, args):
    rc = int(fn(*args))
    return rc, (_lib.last_error() if rc not in (0, bc.CE_ERR_HIP) else None)


# ---- the sgd pair: the case lists of tests/bag_refusal_cases.py (singles and pairs; `lr` has no bad value there)

@no_gpu
@pytest.mark.parametrize("entry, sibling", [("ce_bag_backward_sgd_lrdev", "ce_bag_backward_sgd_act"),
                                            ("ce_bag_backward_sgd_src_lrdev", "ce_bag_backward_sgd_src_act")])
def test_sgd_entries_refuse_as_their_siblings(entry, sibling):
    from cachedembedding_amd import _lib
    lr_pos = [name for name, _, _ in bc.ENTRIES[sibling]].index("lr")
    cases = bc.cases(sibling)
    assert len(cases) > 300
    bad, refused = [], 0
    for label, args in cases:
        want = _answer(_lib, getattr(_lib.lib, sibling), args)
        dev = list(args)
        dev[lr_pos] = LR_PTR
        got = _answer(_lib, getattr(_lib.lib, entry), dev)
        refused += want[1] is not None
        if got != want:
            bad.append((label, got, want))
    assert not bad, f"{entry}: {len(bad)} of {len(cases)} cases answered differently (case, got, sibling): {bad[:5]}"
    assert refused > 100                                 # the walk did meet the refusals


# ---- the update pair: every argument's bad values one at a time, per covered entry

def _update_spec(src, wdtype, opt, rounding, acc, lib):
    """[(argument, kind, good value)] of the lrdev entry, in the order of its declaration"""
    rows, dim, nnz = 1000, 128, 64
    if acc == STEP:
        need = lib.ce_bag_backward_update_compact_workspace(rows, nnz, dim)
    elif wdtype == F32:
        need = lib.ce_bag_backward_rowwise_adagrad_workspace(rows, dim)
    else:
        need = lib.ce_bag_backward_w16_workspace(rows, dim)
    head = ([bc._W, ("weight_dtype", "wd", wdtype)] + bc._src("grad_out")[1:] if src
            else [bc._W, ("weight_dtype", "wd", wdtype)] + bc._bag(bc._W, "grad_out")[1:])
    keys = [("keys", "ptr", bc._p(4))] if src else [("presorted", "optptr", None)]
    return head + [bc._ACT] + keys + [
        ("row_of_slot", "optptr", None), ("momentum", "ptr", bc._p(8)), ("momentum_rows", "size", rows),
        ("lr", "keep", None), ("eps", "eps", 1e-8), ("optimizer", "code", opt), ("rounding", "code", rounding),
        ("seed", "keep", 5), ("accumulator", "keep", acc), ("workspace", "ptr", bc._p(9)),
        ("workspace_bytes", "bytes", need), ("stream", "keep", None)]


def _bad(kind, good):
    if kind == "wd":
        return {"f32": F32, "bf16": BF16, "f16": F16, "7": 7}
    if kind == "eps":
        return {"0": 0.0, "-1": -1.0}
    if kind == "code":
        return {"7": 7, "-1": -1}
    if kind == "bytes":
        return {"0": 0, "need-1": good - 1}
    return bc._bad_values(kind, good)


def _sibling(src, wdtype, acc):
    """(name, the lrdev arguments it does not have) of the entry a call with this table and accumulator is"""
    tail = "_src" if src else ""
    if acc == STEP:
        return "ce_bag_backward_update_compact" + tail, {"accumulator"}
    if wdtype == F32:
        return ("ce_bag_backward_rowwise_adagrad_src_act" if src else "ce_bag_backward_rowwise_adagrad_act",
                {"accumulator", "weight_dtype", "optimizer", "rounding", "seed"})
    return ("ce_bag_backward_update_src_w16" if src else "ce_bag_backward_update_w16"), {"accumulator"}


# one line per covered entry and per kernel family it launches; the last two are what the covered entry itself refuses
CONFIGS = [(F32, ADAGRAD, NEAREST, CACHE), (BF16, SGD, NEAREST, CACHE), (BF16, ADAGRAD, STOCH, CACHE),
           (F16, SGD, STOCH, CACHE), (F32, ADAGRAD, NEAREST, STEP), (BF16, SGD, STOCH, STEP),
           (F16, ADAGRAD, NEAREST, STEP), (F32, SGD, NEAREST, STEP), (BF16, ADAGRAD, STOCH, STEP)]


@no_gpu
@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_update_entries_refuse_as_the_entry_they_cover(src, cfg):
    from cachedembedding_amd import _lib
    wdtype, opt, rounding, acc = cfg
    entry = "ce_bag_backward_update_src_lrdev" if src else "ce_bag_backward_update_lrdev"
    spec = _update_spec(src, wdtype, opt, rounding, acc, _lib.lib)
    names = [n for n, _, _ in spec]
    sib, missing = _sibling(src, wdtype, acc)
    good = [g for _, _, g in spec]
    calls = [("good", good)]
    for pos, (name, kind, g) in enumerate(spec):
        if name in missing or kind == "keep":
            continue                                 # the sibling has no such argument to set to the same bad value
        for label, b in _bad(kind, g).items():
            if name == "weight_dtype" and (b == F32) != (wdtype == F32) and acc == CACHE:
                continue                             # (that call is another covered entry's: its own line of CONFIGS)
            args = list(good)
            args[pos] = b
            calls.append((f"{name}={label}", args))
    assert len(calls) > 30
    bad, refused = [], 0
    for label, args in calls:
        sib_args = [0.1 if n == "lr" else a for n, a in zip(names, args) if n not in missing]
        want = _answer(_lib, getattr(_lib.lib, sib), sib_args)
        dev = [LR_PTR if n == "lr" else a for n, a in zip(names, args)]
        got = _answer(_lib, getattr(_lib.lib, entry), dev)
        refused += want[1] is not None
        if got != want:
            bad.append((label, got, want))
    assert not bad, f"{entry} as {sib}: {len(bad)} of {len(calls)} answered differently (case, got, sibling): {bad[:5]}"
    assert refused >= 10
    if cfg in CONFIGS[-2:]:                            # what the step-sized entries do not take, refused here as there
        rc, msg = _answer(_lib, getattr(_lib.lib, entry), [LR_PTR if n == "lr" else a for n, a in zip(names, good)])
        assert rc == CE_ERR_UNSUPPORTED and msg


@no_gpu
@pytest.mark.parametrize("src", [False, True], ids=["slots", "src"])
def test_update_entries_own_refusals(src):
    """lr == NULL first, an unknown accumulator second, CE_OPT_SGD on an fp32 table where the not-taken check stands"""
    from cachedembedding_amd import _lib
    entry = getattr(_lib.lib, "ce_bag_backward_update_src_lrdev" if src else "ce_bag_backward_update_lrdev")
    spec = _update_spec(src, BF16, SGD, NEAREST, CACHE, _lib.lib)
    names = [n for n, _, _ in spec]

    def call(**over):
        args = {n: (LR_PTR if n == "lr" else g) for n, _, g in spec}
        args.update(over)
        return _answer(_lib, entry, [args[n] for n in names])

    assert call()[0] == bc.CE_ERR_HIP                    # every check passed: the first launch fails without a GPU
    for over in ({}, {"act_dtype": 9}, {"weight_dtype": 7}, {"nnz": 0}, {"accumulator": 5}, {"weight": None}):
        rc, msg = call(lr=None, **over)
        assert rc == CE_ERR_INVALID and "lr" in msg and "null" in msg, (over, rc, msg)
    for over in ({}, {"act_dtype": 9}, {"weight_dtype": 7}, {"nnz": 0}):
        for code in (2, -1, 5):
            rc, msg = call(accumulator=code, **over)
            assert rc == CE_ERR_INVALID and "accumulator" in msg, (over, code, rc, msg)
    # SGD on an fp32 table has no accumulator of either size: after the unknown-code checks, before the pointers
    for acc in (CACHE, STEP):
        rc, msg = call(weight_dtype=F32, accumulator=acc)
        assert rc == CE_ERR_UNSUPPORTED and "fp32" in msg and "CE_OPT_SGD" in msg, (acc, rc, msg)
        assert call(weight_dtype=F32, accumulator=acc, optimizer=7) == \
            (CE_ERR_INVALID, "unknown optimizer 7 (CE_OPT_SGD / CE_OPT_ROWWISE_ADAGRAD)")
        assert call(weight_dtype=F32, accumulator=acc, weight=None)[0] == CE_ERR_UNSUPPORTED
    # the cache-sized fp32 update has neither rounding nor seed: not looked at
    assert call(weight_dtype=F32, optimizer=ADAGRAD, rounding=7,
                workspace_bytes=_lib.lib.ce_bag_backward_rowwise_adagrad_workspace(1000, 128))[0] == bc.CE_ERR_HIP


@no_gpu
@pytest.mark.parametrize("entry, sibling", [("ce_bag_backward_sgd_lrdev", "ce_bag_backward_sgd_act"),
                                            ("ce_bag_backward_sgd_src_lrdev", "ce_bag_backward_sgd_src_act")])
def test_sgd_entries_refuse_a_null_lr_first(entry, sibling):
    from cachedembedding_amd import _lib
    spec = bc.ENTRIES[sibling]
    names = [n for n, _, _ in spec]
    for over in ({}, {"act_dtype": 9}, {"nnz": 0}, {"weight": None}, {"dim": 0}):
        args = {n: g for n, _, g in spec}
        args.update(over)
        args["lr"] = None
        rc, msg = _answer(_lib, getattr(_lib.lib, entry), [args[n] for n in names])
        assert rc == CE_ERR_INVALID and "lr" in msg and "null" in msg, (over, rc, msg)


# ---- Python: what is refused when the learning rate is set

def _bad_tensors():
    return [torch.zeros(1, dtype=torch.float64), torch.zeros(2), torch.zeros(1, requires_grad=True),
            torch.zeros(1, dtype=torch.float16), torch.zeros(1, dtype=torch.int32), torch.zeros(0)]


def _stub():
    """what CachedEmbeddingBag.set_fused_* touch, without the GPU its constructor needs"""
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD
    mgr = types.SimpleNamespace(momentum1=torch.zeros(4), cached_idx_map=None, num_embeddings=4, device="cpu")
    return types.SimpleNamespace(mode="sum", table_dtype=torch.float32, weight_rounding="stochastic",
                                 fused_sgd=FusedSGD(), fused_adagrad=FusedRowwiseAdagrad(), cache_weight_mgr=mgr)


def test_a_tensor_that_cannot_be_a_learning_rate_is_refused_when_it_is_set():
    from cachedembedding_amd import CachedEmbeddingBag
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD
    for t in _bad_tensors():
        for make in (lambda: FusedSGD(t), lambda: FusedRowwiseAdagrad(t),
                     lambda: setattr(FusedSGD(0.1), "lr", t), lambda: setattr(FusedRowwiseAdagrad(0.1), "lr", t),
                     lambda: CachedEmbeddingBag.set_fused_sgd(_stub(), t),
                     lambda: CachedEmbeddingBag.set_fused_rowwise_adagrad(_stub(), t)):
            with pytest.raises((ValueError, TypeError)):
                make()
    good = torch.full((1,), 0.1)
    for f in (FusedSGD(good), FusedRowwiseAdagrad(good)):
        assert f.lr is good                               # kept by reference, not copied
        f.lr = 0.5
        assert f.lr == 0.5
        f.lr = None
        assert f.lr is None
    s = _stub()
    CachedEmbeddingBag.set_fused_sgd(s, good)
    assert s.fused_sgd.lr is good
    s = _stub()
    CachedEmbeddingBag.set_fused_rowwise_adagrad(s, good)
    assert s.fused_adagrad.lr is good


def test_a_tensor_learning_rate_with_the_sorted_updates_or_max_is_not_implemented():
    from cachedembedding_amd import CachedEmbeddingBag
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD, check_lr_path
    t = torch.full((1,), 0.1)
    for make in (lambda: FusedSGD(t, deterministic=True), lambda: FusedRowwiseAdagrad(t, deterministic=True),
                 lambda: CachedEmbeddingBag.set_fused_sgd(_stub(), t, deterministic=True),
                 lambda: CachedEmbeddingBag.set_fused_rowwise_adagrad(_stub(), t, deterministic=True),
                 lambda: check_lr_path(t, False, "max")):
        with pytest.raises(NotImplementedError):
            make()
    smax = _stub()
    smax.mode = "max"
    with pytest.raises(NotImplementedError):
        CachedEmbeddingBag.set_fused_sgd(smax, t)
    FusedSGD(0.1, deterministic=True)                      # a float keeps every path it had
    check_lr_path(0.1, True, "max")


def test_the_row_wise_sharded_embedding_refuses_a_tensor():
    from cachedembedding_amd.parallel import RowwiseShardedEmbeddingBag
    stub = types.SimpleNamespace(_lr=[None])
    with pytest.raises(NotImplementedError):
        RowwiseShardedEmbeddingBag.set_fused_sgd(stub, torch.full((1,), 0.1))
    RowwiseShardedEmbeddingBag.set_fused_sgd(stub, 0.25)
    assert stub._lr == [0.25]


# ---- the example trainer

def _dlrm_main():
    sys.path.insert(0, str(ROOT / "examples"))
    return importlib.import_module("dlrm_main")


@pytest.mark.parametrize("adagrad", [False, True], ids=["sgd", "adagrad"])
def test_dense_step_with_a_tensor_learning_rate_follows_torch_optim(adagrad):
    dm = _dlrm_main()
    g = torch.Generator().manual_seed(3)
    init = [torch.randn(5, 3, generator=g), torch.randn(7, generator=g), torch.randn(2, 2, 2, generator=g)]
    grads = [[torch.randn(p.shape, generator=g) for p in init] for _ in range(5)]
    lrs = [0.1, 0.1, 0.1, 0.025, 0.025]                     # a change after step 2
    ref = [p.clone().requires_grad_(True) for p in init]
    opt = (torch.optim.Adagrad if adagrad else torch.optim.SGD)(ref, lr=lrs[0])
    mine = [p.clone().requires_grad_(True) for p in init]
    lr_t = torch.full((1,), lrs[0])
    step = dm.DenseStep(mine, lr_t, adagrad=adagrad)
    for k in range(5):
        for grp in opt.param_groups:
            grp["lr"] = lrs[k]
        lr_t.fill_(lrs[k])
        for p, q, gr in zip(ref, mine, grads[k]):
            p.grad, q.grad = gr.clone(), gr.clone()
        opt.step()
        step.step()
        for p, q in zip(ref, mine):
            torch.testing.assert_close(q.detach(), p.detach())
        step.zero_grad()
        assert all(q.grad is None for q in mine)
    assert not torch.equal(mine[0].detach(), init[0])


@pytest.mark.parametrize("total, point", [(20, 0.5), (20, 0.8), (10, 0.0), (7, 0.33), (100, 0.8), (5, 0.99), (4, 1.0)])
def test_change_point_is_the_reference_s(total, point):
    """the reference (baselines/dlrm_main.py:453-462) checks `it * (epoch + 1) / limit_train_batches > lr_change_point`
    after iteration `it` has trained and then sets every group's lr, once; here the progress is counted over the run's
    total iterations (epoch + 1 == 1, limit = total)"""
    dm = _dlrm_main()
    want, changed = [], False
    for it in range(total):
        want.append(changed)                                    # whether iteration `it` trains with the new rate
        if not changed and (it * 1 / total) > point:
            changed = True
    args = dm.parse_args(["--change_lr", "--lr_change_point", str(point), "--lr_after_change_point", "0.05",
                          "--learning_rate", "0.4"])
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.4, "lr_scale": 1}, {"lr": 0.8, "lr_scale": 2}])
    change = dm.LrChange(args, total, opt, embed=None)
    got = []
    for it in range(total):
        got.append(opt.param_groups[0]["lr"] != 0.4)
        assert dm.lr_changes_after(it, total, point) == ((it * 1 / total) > point)
        change.after_iteration()
    assert got == want
    if any(want):
        assert [g["lr"] for g in opt.param_groups] == [0.05, 0.1]
    # the tensor form: the same iteration, the tensor rewritten in place
    lr_t = torch.full((1,), 0.4)
    change = dm.LrChange(args, total, None, embed=None, lr_tensor=lr_t)
    got = []
    for it in range(total):
        got.append(float(lr_t) != pytest.approx(0.4))
        change.after_iteration()
    assert got == want


def test_trainer_flags():
    dm = _dlrm_main()
    a = dm.parse_args([])
    assert (a.change_lr, a.lr_change_point, a.lr_after_change_point) == (False, 0.80, 0.20)
