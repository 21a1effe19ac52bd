"""CPU tests of the sorted (deterministic) fold for the in-row fused optimizers: the fp32 model the GPU
tests predict bits with -- sorted_fold_ref.fold_sorted in front of the existing fp32 reference steps -- keeps half the
tolerance the GPU tests hold the kernels to on their very inputs; the bit tests' input tells wrong fold orders apart;
the Python switch, the C entries' refusals (before any HIP call) and the example's flag."""
import ctypes
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import sorted_fold_ref as sf  # noqa: E402
import sorted_in_row_cases as sc  # noqa: E402

RTOL, ATOL = sc.RTOL, sc.ATOL


def _ratio(got, want):
    return float((np.abs(got - want) / (ATOL + RTOL * np.abs(want))).max())


# ---- the fp64 references stay authoritative -----------------------------------------------------------------------------

@pytest.mark.parametrize("layout,which,case", sc.SEVEN)
@pytest.mark.parametrize("D", [128, 768])
def test_sorted_fold_with_the_fp32_steps_keeps_half_the_tolerance(D, layout, which, case):
    W0, steps, kw = sc.seven(layout, which, case, D)
    want, named = sc.model(layout, W0, steps, np.float64, **kw)
    got, named32 = sc.model(layout, W0, steps, np.float32, **kw)
    assert (named == named32).all() and named.any() and not named.all()
    for (name, g), (_, w) in zip(sc.parts(layout, got), sc.parts(layout, want)):
        r = _ratio(g.astype(np.float64), w)
        print(f"D={D} {layout} {which} {case} {name}: max |err| / (atol + rtol |ref|) = {r:.3g}")
        assert r <= 0.5, name
        assert g.dtype == np.float32


def test_fold_sorted_is_a_plain_sum_where_nothing_has_an_order():
    """one lookup per row: the term itself (scaled: the rounded product); against adam_ref.fold in fp64 otherwise"""
    from adam_ref import fold
    rng = np.random.default_rng(0)
    D = 12
    g = rng.standard_normal((5, D)).astype(np.float32)
    s = np.asarray([1.0, 0.5, 0.0, 1.0, 1.25], np.float32)
    uniq, out = sf.fold_sorted([4, 2, 9, 0, 7], g, s, D)
    assert list(uniq) == [0, 2, 4, 7, 9]
    np.testing.assert_array_equal(out, (g * s[:, None]).astype(np.float32)[[3, 1, 0, 4, 2]])
    step = sc.hot_step(8, "psw")
    slots, rows, scales = sf.lookup_terms(step["ids"], step["off"], step["go"], sc.R, "sum", step["psw"], 0)
    assert len(slots) == sum(sc.RUNS)                               # every covered, in-range lookup and no other
    uniq, out = sf.fold_sorted(slots, rows, scales, 8)
    u64, g64 = fold(slots, rows.astype(np.float64) * scales[:, None].astype(np.float64), 8)
    assert (uniq == u64).all() and sorted(np.bincount(slots)[uniq]) == sorted(sc.RUNS)
    np.testing.assert_allclose(out, g64, rtol=1e-4, atol=1e-4)


# ---- the bit tests have power ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wrong", sf.WRONG)
def test_wrong_folds_change_bits_on_the_hot_run_input(wrong):
    """(the per-sample-weight form: the only one in which a product is rounded at all)"""
    D = 8
    step = sc.hot_step(D, "psw")
    right = sc.folded(step, sc.R)
    got = sc.folded(step, sc.R, wrong=wrong)
    assert (right[0] == got[0]).all()
    differ = (right[1].view(np.uint32) != got[1].view(np.uint32)).any(axis=1)
    print(f"{wrong}: rows whose folded gradient changes: {int(differ.sum())} of {len(differ)}")
    assert differ.any()
    counts = np.bincount(step["ids"][(step["ids"] >= 0) & (step["ids"] < sc.R)], minlength=sc.R)[right[0]]
    if wrong in ("aligned_chunks", "descending_partials"):
        assert not differ[counts == 1].any()                        # a run of one has no chunks to cut or order


def test_the_hot_run_input_is_what_the_issue_names():
    for form in sc.HOT_FORMS:
        s = sc.hot_step(128, form)
        ids = s["ids"]
        valid = ids[(ids >= 0) & (ids < sc.R)]
        assert sorted(np.bincount(valid)[np.unique(valid)]) == sorted(sc.RUNS) and max(sc.RUNS) > 4096
        lens = np.diff(s["off"])
        assert (lens == 0).any() and s["off"][-1] == len(ids) and len(ids) > len(valid)
        # runs longer than a chunk that start at a sorted position which is no multiple of 64: cutting chunks at
        # aligned positions is then another fold
        order = np.argsort(valid, kind="stable")
        run_starts = np.flatnonzero(np.diff(valid[order], prepend=-1))
        run_lens = np.diff(np.append(run_starts, len(valid)))
        assert ((run_starts % 64 != 0) & (run_lens > 64)).any()
    assert {0.0, 1.0} <= set(sc.hot_step(8, "psw")["psw"].tolist())


# ---- the Python surface ----------------------------------------------------------------------------------------------------

def _stub(layout):
    return types.SimpleNamespace(fused_optimizer=layout, table_dtype=torch.float32, mode="sum", num_embeddings=9,
                                 embedding_dim=8, _no_weight_decay=None)


def test_python_switch_is_accumulator_sorted():
    import cachedembedding_amd as ce
    from cachedembedding_amd.functional import (FusedAdagrad, FusedAdam, FusedRowwiseAdagrad, FusedSGD,
                                                check_accumulator)
    lr_t = torch.full((1,), 0.1)
    for lr in (0.1, lr_t):                                          # a tensor lr is accepted, unlike 3.5's entries
        for f in (FusedAdam(lr, accumulator="sorted"), FusedAdam(lr, accumulator="sorted", layout="partial_rowwise_adam"),
                  FusedAdagrad(lr, accumulator="sorted")):
            assert f.accumulator == "sorted" and f.deterministic is False
    f = FusedAdam(0.1, accumulator="sorted", weight_decay=0.01, weight_decay_mode="decoupled", grad_clip=1.0)
    assert (f.weight_decay, f.grad_clip) == (0.01, 1.0)
    for cls in (FusedAdam, FusedAdagrad):
        with pytest.raises(ValueError, match="accumulator='row'"):
            cls(0.1, accumulator="row")
        with pytest.raises(NotImplementedError, match="deterministic.*accumulator='sorted'"):
            cls(0.1, deterministic=True)
    # the setters
    E = ce.CachedEmbeddingBag
    for layout in ("adam", "partial_rowwise_adam"):
        m = _stub(layout)
        m.fused_adam = FusedAdam(None, layout=layout)
        E.set_fused_adam(m, lr_t, accumulator="sorted", weight_decay=0.01)
        assert m.fused_adam.accumulator == "sorted" and m.fused_adam.lr is lr_t
        with pytest.raises(ValueError, match="accumulator='row'"):
            E.set_fused_adam(m, 0.1, accumulator="row")
        with pytest.raises(NotImplementedError, match="deterministic"):
            E.set_fused_adam(m, 0.1, deterministic=True)
    m = _stub("adagrad")
    m.fused_elementwise_adagrad = FusedAdagrad(None)
    E.set_fused_adagrad(m, 0.1, accumulator="sorted", lr_decay=0.1, grad_clip=0.5)
    assert m.fused_elementwise_adagrad.accumulator == "sorted"
    with pytest.raises(ValueError, match="accumulator='row'"):
        E.set_fused_adagrad(m, 0.1, accumulator="row")
    # SGD and row-wise Adagrad are not widened: their deterministic fold is deterministic=True
    with pytest.raises(ValueError, match="accumulator='sorted'"):
        check_accumulator("sgd", None, "sorted")
    with pytest.raises(ValueError):
        FusedRowwiseAdagrad(0.1, accumulator="sorted")
    with pytest.raises(ValueError):
        FusedSGD(0.1, accumulator="sorted")


# ---- the C entries, without a GPU: everything is refused before a HIP call ------------------------------------------

def _entries():
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    return _lib, _lib.lib


def _call(lib, layout, dim=8, lr=0.1, lr_dev=0, eps=1e-8, step=0x1000, ws=0x10000, ws_bytes=1 << 30, weight=0x2000,
          go=0x3000, nnz=5, num_rows=10, num_bags=5, mode=0, hook=0, act=0, wd=0.0, wd_mode=0, clip=0.0, clip_mode=0,
          b1=0.9, b2=0.999, lr_decay=0.0, v=0x7000, v_rows=10, indices=0x5000, offsets=0x6000):
    """pointers are fake (aligned, never dereferenced: every call here returns before a launch)"""
    p = lambda x: ctypes.c_void_p(x) if x else None  # noqa: E731
    head = (p(weight), num_rows, dim, p(indices), nnz, p(offsets), 1, num_bags, 1, None, mode, hook, p(go), act)
    tail = (lr, p(lr_dev), eps, wd, wd_mode, clip, clip_mode, p(step), p(ws), ws_bytes, None)
    if layout == "adagrad":
        return lib.ce_bag_backward_adagrad_sorted(*head, lr_decay, *tail)
    if layout == "partial_rowwise_adam":
        return lib.ce_bag_backward_pradam_sorted(*head, None, p(v), v_rows, b1, b2, *tail)
    return lib.ce_bag_backward_adam_sorted(*head, b1, b2, *tail)


def test_workspace_is_aligned_and_does_not_depend_on_num_rows():
    _lib, lib = _entries()
    fn = lib.ce_bag_backward_in_row_sorted_workspace
    for nnz, dim in ((0, 8), (1, 4), (5, 8), (4752, 768), (1 << 20, 128)):
        need = fn(10, nnz, dim)
        assert need > 0 and need % 256 == 0
        assert need == fn(1, nnz, dim) == fn(1 << 30, nnz, dim)
        assert need >= max(nnz, 1) * dim * 4                        # a partial row per lookup behind the sort's arrays
    assert fn(10, 5, 8) <= fn(10, 6, 8) <= fn(10, 6, 12)
    for nnz, dim in ((-1, 8), (2 ** 31 - 1, 8), (5, 0), (5, -4)):
        assert fn(10, nnz, dim) == 0
    assert lib.ce_version() == 6
    for name in ("ce_bag_backward_adam_sorted", "ce_bag_backward_pradam_sorted", "ce_bag_backward_adagrad_sorted"):
        clip = name.replace("_sorted", "_clip") if "adagrad" not in name else "ce_bag_backward_adagrad"
        # the clipped atomic entry's list without `presorted` and `accumulator`
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[clip][1]) - 2


@pytest.mark.parametrize("layout", sc.LAYOUTS)
def test_c_entries_refuse_in_the_stated_order(layout):
    """every call piles the LATER mistakes on top of the one that must be named"""
    _lib, lib = _entries()
    bad, unsup = _lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED
    adagrad = layout == "adagrad"
    late = dict(eps=-1.0, lr=-0.1, act=9, weight=0, nnz=-1, mode=7, hook=3, ws=0x10004, dim=6)

    def refused(code, word, **kw):
        rc = _call(lib, layout, **kw)
        assert rc == code and word in _lib.last_error(), (kw, rc, _lib.last_error())

    state = dict(lr_decay=-1.0) if adagrad else dict(b1=1.0)
    refused(bad, "step", step=0, wd_mode=9, clip_mode=9, **state, **late)
    refused(bad, "weight_decay_mode", wd_mode=9, clip_mode=9, **state, **late)
    refused(bad, "weight_decay", wd=-1.0, wd_mode=1, clip_mode=9, **state, **late)
    refused(bad, "grad_clip_mode", clip_mode=9, **state, **late)
    refused(bad, "grad_clip", clip=0.0, clip_mode=1, **state, **late)
    if adagrad:
        for d in (-1e-9, float("nan")):
            refused(bad, "lr_decay", lr_decay=d, **late)
    else:
        for kw in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=float("nan"))):
            refused(bad, "beta", **kw, **late)
    refused(bad, "eps", **late)
    late.pop("eps")
    refused(bad, "lr must be", **late)
    # lr < 0 is looked at by value only: with a device rate the next check speaks
    refused(bad, "activation dtype", lr_dev=0x8000, **late)
    late.pop("lr")
    refused(bad, "activation dtype", **late)
    late.pop("act")
    refused(bad, "null pointer", **late)
    late.pop("weight")
    refused(bad, "null pointer", go=0, **late)
    refused(bad, "null pointer", ws=0, **{k: v for k, v in late.items() if k != "ws"})
    if layout == "partial_rowwise_adam":
        refused(bad, "second moment", v=0, **late)
        refused(bad, "second moment", v_rows=0, **late)
    refused(bad, "nnz out of range", **late)
    late.pop("nnz")
    refused(bad, "num_rows out of range", num_rows=0, **late)
    refused(bad, "num_bags out of range", num_bags=-1, **late)
    refused(bad, "dim must be positive", **dict(late, dim=0))
    refused(unsup, "mode must be sum or mean", **late)
    late.pop("mode")
    refused(bad, "hook_features", **late)                           # 3 does not divide 5 bags
    late.pop("hook")
    refused(bad, "aligned", **late)                                 # the workspace: 4 bytes off
    refused(bad, "aligned", weight=0x2004, **dict(late, ws=0x10000))
    refused(bad, "aligned", step=0x1004, **dict(late, ws=0x10000))
    refused(bad, "aligned", go=0x3004, **dict(late, ws=0x10000))
    late.pop("ws")
    need = lib.ce_bag_backward_in_row_sorted_workspace(10, 5, 8)
    refused(bad, "workspace too small", ws_bytes=need - 1, dim=8)
    for dim in (2, 6, 7, 1028, 2048):
        refused(unsup, "dim % 4 == 0", dim=dim)
    # nnz == 0 / num_bags == 0: CE_OK after the checks, with no launch (the pointers are fake); the checks still run
    assert _call(lib, layout, nnz=0, num_bags=0) == _lib.CE_OK
    assert _call(lib, layout, nnz=0, num_bags=0, indices=0, offsets=0) == _lib.CE_OK
    assert _call(lib, layout, num_bags=0) == _lib.CE_OK
    refused(bad, "eps", nnz=0, num_bags=0, eps=-1.0)
    refused(unsup, "dim % 4 == 0", nnz=0, num_bags=0, dim=6)
    # behind every other check: lookups without their arrays
    refused(bad, "null pointer", indices=0)
    refused(bad, "null pointer", offsets=0)


# ---- the example ---------------------------------------------------------------------------------------------------------------

def test_example_flag_argument_checks():
    import importlib
    sys.path.insert(0, str(HERE.parent / "examples"))
    dm = importlib.import_module("dlrm_main")
    for opt in (["--adam"], ["--adam", "--adam_partial_rowwise"], ["--adagrad_elementwise"]):
        a = dm.parse_args(["--use_cache", "--embed_sorted_update"] + opt)
        dm.check_embed_sorted_update(a)
        assert dm._accumulator(a) == "sorted"
    # the rate is read from device memory: --graph_step --change_lr pass the argument checks with it
    a = dm.parse_args(["--use_cache", "--adam", "--embed_sorted_update", "--graph_step", "--change_lr"])
    dm.check_embed_sorted_update(a)
    assert dm._accumulator(dm.parse_args(["--use_cache", "--adam"])) == "cache"
    assert dm._accumulator(dm.parse_args(["--use_cache", "--adam", "--step_accumulator"])) == "step"
    for other in ([], ["--fused_sgd"]):
        with pytest.raises(ValueError, match="--embed_sorted_update"):
            dm.main(["--use_cache", "--embed_sorted_update"] + other)
    with pytest.raises(ValueError, match="--adagrad_deterministic"):
        dm.main(["--use_cache", "--embed_sorted_update", "--adagrad"])
    with pytest.raises(ValueError, match="--step_accumulator"):
        dm.main(["--use_cache", "--embed_sorted_update", "--adam", "--step_accumulator"])
