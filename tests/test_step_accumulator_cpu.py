"""CPU tests of the step-sized accumulator of the atomic fused updates (ce_bag_backward_update_compact*): the C ABI of
the three new entries, the workspace bound, the accumulator= keyword and the example's flag, and every refusal -- from
the C entries with no GPU present, and from Python before the forward.  Every call into an update entry passes nnz = 0,
with which it launches nothing whatever else its arguments are."""
import inspect
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = ["ce_bag_backward_update_compact_workspace", "ce_bag_backward_update_compact",
                "ce_bag_backward_update_compact_src"]
C2, NNZ2, D2 = 1779442, 425984, 128               # configs[2]: cache rows, lookups of a step, dim


def _lib():
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    return _lib


def _bound(L, num_rows, nnz, dim):
    cap = min(nnz, num_rows)
    return 6 * num_rows + cap * (4 * dim + 4) + 8 * L.lib.ce_bag_presort_len(nnz) + 65536


def test_header_declares_and_library_exports_the_entries():
    L = _lib()
    header = (ROOT / "include" / "ce_api.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", body), name
        assert re.search(rf" T {name}\b", out), name
        assert name in L.SIGNATURES
        assert getattr(L.lib, name).argtypes == L.SIGNATURES[name][1]
    assert L.SIGNATURES["ce_bag_backward_update_compact"][1] == L.SIGNATURES["ce_bag_backward_update_w16"][1]
    assert L.SIGNATURES["ce_bag_backward_update_compact_src"][1] == L.SIGNATURES["ce_bag_backward_update_src_w16"][1]
    assert L.lib.ce_version() == 6
    m = re.search(r"#define CE_COMPACT_BLOCK (\d+)", header)
    assert m and int(m.group(1)) == L.CE_COMPACT_BLOCK


def test_workspace_obeys_the_bound_and_does_not_follow_rows_times_dim():
    L = _lib()
    f = L.lib.ce_bag_backward_update_compact_workspace
    for R, nnz, D in ((C2, NNZ2, D2), (1000, 5, 8), (5, 1000, 8), (1, 1, 1), (3 * 4096 + 17, 16384, 6),
                      (200000, 4096, 128), (2 ** 27, NNZ2, 1024), (100, 0, 128)):
        assert 0 < f(R, nnz, D) <= _bound(L, R, nnz, D), (R, nnz, D)
        assert f(R, nnz, D) % 256 == 0
        cap = min(nnz, R)
        assert f(R, nnz, D) >= R + cap * D * 4 + 4 * R + 4 * cap + 8        # flags, acc, cidx, list, the counter
    # configs[2]: against the cache-sized accumulator (the formula gives 0.254)
    full = L.lib.ce_bag_backward_rowwise_adagrad_workspace(C2, D2)
    assert f(C2, NNZ2, D2) <= 0.27 * full
    assert f(C2, NNZ2, D2) <= 0.27 * L.lib.ce_bag_backward_w16_workspace(C2, D2)
    # at fixed nnz nothing grows with num_rows * dim: more rows cost the 6 bytes per row of the bound at most ...
    for D in (8, 128, 1024):
        a, b = f(10 ** 6, NNZ2, D), f(10 ** 7, NNZ2, D)
        assert 0 <= b - a <= 6 * (10 ** 7 - 10 ** 6) + 65536, D
    # ... and a wider row costs what the cap rows cost, whatever the number of rows
    for R in (10 ** 6, 10 ** 7):
        assert f(R, NNZ2, 256) - f(R, NNZ2, 128) == NNZ2 * 128 * 4
    # cap = min(nnz, num_rows)
    assert f(1000, 10 ** 6, 128) - f(1000, 10 ** 5, 128) <= 8 * (L.lib.ce_bag_presort_len(10 ** 6) -
                                                                  L.lib.ce_bag_presort_len(10 ** 5))
    assert f(-1, 10, 8) == 0 and f(10, -1, 8) == 0 and f(10, 10, -1) == 0 and f(2 ** 31, 10, 8) == 0 and \
        f(10, 2 ** 31, 8) == 0


def _calls(L):
    lib = L.lib
    p = [0x7f0000000000 + 0x100000 * i for i in range(8)]            # made-up, non-null, 256-byte aligned
    R, D = 1000, 128
    wsb = lib.ce_bag_backward_update_compact_workspace(R, 0, D)
    table = dict(weight=p[0], wd=L.CE_ACT_F32, R=R, D=D)
    tail = dict(rmap=None, mom=p[4], mrows=R, lr=0.1, eps=1e-8, opt=L.CE_OPT_ROWWISE_ADAGRAD, rnd=L.CE_ROUND_NEAREST,
                seed=0, ws=p[5], wsb=wsb, stream=None)
    slots = dict(table, idx=p[1], nnz=0, off=p[2], off64=1, nb=0, last=1, psw=None, mode=L.CE_MODE_SUM, hook=0,
                 go=p[3], act=L.CE_ACT_F32, keys=None, **tail)
    src = dict(table, nnz=0, go=p[3], act=L.CE_ACT_F32, keys=p[6], **tail)

    def call_slots(**kw):
        return lib.ce_bag_backward_update_compact(*dict(slots, **kw).values())

    def call_src(**kw):
        return lib.ce_bag_backward_update_compact_src(*dict(src, **kw).values())
    return (call_slots, call_src), p, wsb


def test_refusals_come_from_the_arguments_alone():
    """one bad argument at a time; nnz = 0, so a call that were NOT refused would still launch nothing"""
    L = _lib()
    calls, p, wsb = _calls(L)
    sgd = dict(opt=L.CE_OPT_SGD, mom=None, mrows=0, eps=0.0)
    for call in calls:
        assert call() == L.CE_OK                                      # fp32 table, row-wise Adagrad
        assert call(rnd=L.CE_ROUND_STOCHASTIC) == L.CE_OK            # an fp32 table is not rounded: the code is ignored
        for wd in (L.CE_ACT_BF16, L.CE_ACT_F16):
            assert call(wd=wd) == L.CE_OK
            assert call(wd=wd, **sgd) == L.CE_OK
            assert call(wd=wd, rnd=L.CE_ROUND_STOCHASTIC, **sgd) == L.CE_OK
            # the two refusals of this entry
            assert call(wd=wd, rnd=L.CE_ROUND_STOCHASTIC) == L.CE_ERR_UNSUPPORTED
            assert "CE_ROUND_STOCHASTIC" in L.last_error()
        assert call(**sgd) == L.CE_ERR_UNSUPPORTED and "no accumulator" in L.last_error()
        assert call(rnd=L.CE_ROUND_STOCHASTIC, **sgd) == L.CE_ERR_UNSUPPORTED
        # those of the cache-sized entries (the same update_check)
        for bad in (dict(weight=None), dict(go=None), dict(ws=None), dict(mom=None)):
            assert call(**bad) == L.CE_ERR_INVALID, bad
        for bad in (dict(act=7), dict(wd=7), dict(opt=2), dict(rnd=2), dict(D=0), dict(lr=-1.0), dict(eps=0.0),
                    dict(mrows=0), dict(ws=p[5] + 8), dict(wsb=wsb - 1), dict(R=0), dict(R=2 ** 31, wsb=2 ** 40),
                    dict(nnz=-1), dict(nnz=2 ** 31, wsb=2 ** 40)):
            assert call(**bad) == L.CE_ERR_INVALID, bad
            assert L.last_error()
        assert call(act=7) == L.CE_ERR_INVALID and "activation dtype" in L.last_error()
        assert call(wd=7) == L.CE_ERR_INVALID and "weight_dtype" in L.last_error()
        assert call(opt=2) == L.CE_ERR_INVALID and "optimizer" in L.last_error()
        assert call(rnd=2) == L.CE_ERR_INVALID and "rounding" in L.last_error()
        assert call(wsb=wsb - 1) == L.CE_ERR_INVALID and "workspace too small" in L.last_error()
        assert call(wd=L.CE_ACT_BF16, D=20) == L.CE_ERR_UNSUPPORTED and "dim % 8" in L.last_error()
        assert call(wd=L.CE_ACT_F16, weight=p[0] + 8) == L.CE_ERR_INVALID
        assert call(D=2048, wsb=2 ** 30) == L.CE_ERR_UNSUPPORTED and "too large for this build" in L.last_error()
        # the workspace is sized by the call's nnz: one that fits nnz = 0 does not fit a step of lookups
        assert call(nnz=4096) == L.CE_ERR_INVALID and "workspace too small" in L.last_error()


def test_keyword_exists_and_defaults_to_cache():
    _lib()
    import cachedembedding_amd as ce
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD
    for cls in (FusedRowwiseAdagrad, FusedSGD):
        assert inspect.signature(cls.__init__).parameters["accumulator"].default == "cache"
        f = cls(0.1)
        assert f.accumulator == "cache" and f._ws_step is None
        assert cls(0.1, accumulator="step").accumulator == "step"
        with pytest.raises(ValueError, match="accumulator"):
            cls(0.1, accumulator="row")
        with pytest.raises(NotImplementedError, match="deterministic"):
            cls(0.1, deterministic=True, accumulator="step")
    for m in (ce.CachedEmbeddingBag.set_fused_rowwise_adagrad, ce.CachedEmbeddingBag.set_fused_sgd):
        assert inspect.signature(m).parameters["accumulator"].default == "cache"


def test_python_refuses_before_the_forward():
    """embedding_bag raises on CPU tensors, i.e. before it asks for the GPU, let alone runs a kernel"""
    _lib()
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD, check_accumulator, embedding_bag
    i, o = torch.zeros(4, dtype=torch.long), torch.arange(5)

    def bag(w, fused):
        return embedding_bag(i, w, o, mode="sum", include_last_offset=True, fused_sgd=fused)

    w32, w16 = torch.zeros(10, 8), torch.zeros(10, 8, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="fp32 table"):
        bag(w32, FusedSGD(0.1, accumulator="step"))
    ada = FusedRowwiseAdagrad(0.1, momentum=torch.zeros(10), accumulator="step")
    assert ada.rounding == "stochastic"
    with pytest.raises(NotImplementedError, match="stochastic"):
        bag(w16, ada)
    for fused in (FusedSGD(0.1), FusedRowwiseAdagrad(0.1, momentum=torch.zeros(10))):
        fused.accumulator = "row"                                      # set behind the constructor's back
        with pytest.raises(ValueError, match="accumulator"):
            bag(w16, fused)
        fused.accumulator, fused.deterministic = "step", True
        with pytest.raises(NotImplementedError, match="deterministic"):
            bag(w16, fused)
    # what is NOT refused gets as far as asking for the GPU (or, for Adagrad, for its device momentum)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            bag(w16, FusedSGD(0.1, accumulator="step"))
    # the host logic the module and the example share
    check_accumulator("sgd", torch.float16, "step", False, "stochastic")
    check_accumulator("rowwise_adagrad", torch.float32, "step", False, "stochastic")
    check_accumulator("rowwise_adagrad", torch.bfloat16, "step", False, "nearest")
    check_accumulator("sgd", torch.float32, "cache", True, "stochastic")
    for bad in (("sgd", torch.float32, "step", False, "nearest"), ("rowwise_adagrad", torch.float16, "step", False,
                                                                   "stochastic"),
                ("rowwise_adagrad", torch.float32, "step", True, "nearest"), ("sgd", torch.bfloat16, "step", True,
                                                                              "nearest")):
        with pytest.raises(NotImplementedError):
            check_accumulator(*bad)
    with pytest.raises(ValueError):
        check_accumulator("sgd", torch.bfloat16, "rows")


def test_module_setters_refuse_without_touching_the_module():
    """CachedEmbeddingBag.set_fused_*: the refusal comes first, so a stand-in without a cache shows it"""
    _lib()
    import cachedembedding_amd as ce

    class Stub:
        weight_rounding = "stochastic"

        def __init__(self, dtype):
            self.table_dtype = dtype

    C = ce.CachedEmbeddingBag
    with pytest.raises(NotImplementedError, match="fp32 table"):
        C.set_fused_sgd(Stub(torch.float32), 0.1, accumulator="step")
    with pytest.raises(NotImplementedError, match="stochastic"):
        C.set_fused_rowwise_adagrad(Stub(torch.bfloat16), 0.1, accumulator="step")
    for setter in (C.set_fused_sgd, C.set_fused_rowwise_adagrad):
        with pytest.raises(NotImplementedError, match="deterministic"):
            setter(Stub(torch.float16), 0.1, deterministic=True, accumulator="step")
        with pytest.raises(ValueError, match="accumulator"):
            setter(Stub(torch.float16), None, accumulator="rows")


def test_example_parses_the_flag_and_raises_the_same_refusals():
    sys.path.insert(0, str(ROOT / "examples"))
    import importlib
    dm = importlib.import_module("dlrm_main")
    assert dm.parse_args(["--use_cache", "--adagrad", "--step_accumulator"]).step_accumulator
    assert not dm.parse_args(["--use_cache", "--adagrad"]).step_accumulator
    with pytest.raises(ValueError, match="--step_accumulator"):
        dm.main(["--use_cache", "--step_accumulator"])
    with pytest.raises(NotImplementedError, match="fp32 table"):
        dm.main(["--use_cache", "--fused_sgd", "--step_accumulator"])
    with pytest.raises(NotImplementedError, match="deterministic"):
        dm.main(["--use_cache", "--adagrad", "--adagrad_deterministic", "--step_accumulator"])
    with pytest.raises(NotImplementedError, match="stochastic"):
        dm.main(["--use_cache", "--adagrad", "--table_dtype", "bf16", "--step_accumulator"])
    # the valid combinations pass the check
    for argv in (["--adagrad"], ["--adagrad", "--table_dtype", "fp16", "--weight_rounding", "nearest"],
                 ["--fused_sgd", "--table_dtype", "bf16"]):
        dm.check_step_accumulator(dm.parse_args(["--use_cache", "--step_accumulator"] + argv))
