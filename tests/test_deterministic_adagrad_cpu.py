"""CPU tests of the deterministic, accumulator-free fused row-wise Adagrad (ce_bag_backward_update_sorted): the keyword
and the example's flag, the C ABI of the two new entries, the workspace size, and the refusals that come before the
first launch.  Every call into the update entry passes nnz = 0, with which the entry launches nothing whatever else
its arguments are."""
import inspect
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = ["ce_bag_backward_update_sorted_workspace", "ce_bag_backward_update_sorted"]


def _lib():
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    return _lib


def test_keyword_exists_and_defaults_to_false():
    _lib()
    import cachedembedding_amd as ce
    from cachedembedding_amd.functional import FusedRowwiseAdagrad
    p = inspect.signature(FusedRowwiseAdagrad.__init__).parameters["deterministic"]
    assert p.default is False
    f = FusedRowwiseAdagrad(0.1)
    assert f.deterministic is False and f._ws is None and f._ws16 is None and f._ws_sorted is None
    assert FusedRowwiseAdagrad(0.1, deterministic=True).deterministic is True
    p = inspect.signature(ce.CachedEmbeddingBag.set_fused_rowwise_adagrad).parameters["deterministic"]
    assert p.default is False


def test_example_parses_the_flag_and_refuses_it_without_adagrad():
    sys.path.insert(0, str(ROOT / "examples"))
    import importlib
    dm = importlib.import_module("dlrm_main")
    args = dm.parse_args(["--use_cache", "--adagrad", "--adagrad_deterministic"])
    assert args.adagrad and args.adagrad_deterministic and not args.fused_sgd
    args = dm.parse_args(["--use_cache", "--adagrad"])
    assert not args.adagrad_deterministic
    assert not dm.parse_args(["--use_cache", "--adagrad_deterministic"]).adagrad          # it implies nothing else
    with pytest.raises(ValueError, match="--adagrad_deterministic"):
        dm.main(["--use_cache", "--adagrad_deterministic"])
    with pytest.raises(ValueError, match="--adagrad_deterministic"):
        dm.main(["--use_cache", "--fused_sgd", "--adagrad_deterministic"])


def test_header_declares_and_library_exports_the_entries():
    _lib_ = _lib()
    header = (ROOT / "include" / "ce_api.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib_.LIB_PATH)], capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", body), name
        assert re.search(rf" T {name}\b", out), name
        assert name in _lib_.SIGNATURES
    assert _lib_.lib.ce_version() == 6
    m = re.search(r"#define CE_SORTED_CHUNK (\d+)", header)
    assert m and int(m.group(1)) == _lib_.CE_SORTED_CHUNK == 64


def test_workspace_follows_the_lookups_not_the_table():
    lib = _lib().lib
    f = lib.ce_bag_backward_update_sorted_workspace
    nnz, dim = 425984, 128
    assert f(2 ** 20, nnz, dim) == f(2 ** 27, nnz, dim) > 0
    assert f(2 ** 20, nnz, dim) < lib.ce_bag_backward_rowwise_adagrad_workspace(1779442, dim) // 8
    # 5 int32 per lookup, 256 histogram bins per 4096-lookup tile (+ the scan's total), 2 partial rows per chunk of 64
    # lookups; every array rounded up to 256 bytes
    want = 5 * nnz * 4 + 256 * (nnz // 4096) * 4 + 256 + 2 * (nnz // 64) * dim * 4
    assert f(1, nnz, dim) == want
    assert f(1000, 2 * nnz, dim) > f(1000, nnz, dim) and f(1000, nnz, 2 * dim) > f(1000, nnz, dim)
    assert f(1000, -1, dim) == 0 and f(1000, nnz, 0) == 0 and f(1000, 2 ** 31, dim) == 0
    assert f(1000, 0, dim) > 0


def test_everything_refusable_is_refused_before_the_first_launch():
    """one bad argument at a time; nnz = 0, so a call that were NOT refused would still launch nothing"""
    L = _lib()
    lib = L.lib
    p = [0x7f0000000000 + 0x100000 * i for i in range(8)]            # made-up, non-null, 256-byte aligned
    R, D = 1000, 128
    ws_bytes = lib.ce_bag_backward_update_sorted_workspace(R, 0, D)
    good = dict(weight=p[0], wd=L.CE_ACT_F32, R=R, D=D, idx=p[1], nnz=0, off=p[2], off64=1, nb=0, last=1, psw=None,
                mode=L.CE_MODE_SUM, hook=0, go=p[3], act=L.CE_ACT_F32, rmap=None, mom=p[4], mrows=R, lr=0.1, eps=1e-8,
                opt=L.CE_OPT_ROWWISE_ADAGRAD, rnd=L.CE_ROUND_NEAREST, seed=0, ws=p[5], wsb=ws_bytes, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ce_bag_backward_update_sorted(*a.values())

    assert call() == L.CE_OK                                         # nothing to do, nothing launched
    assert call(wd=L.CE_ACT_BF16) == L.CE_OK
    assert call(rnd=L.CE_ROUND_STOCHASTIC) == L.CE_OK               # an fp32 table is not rounded: the code is ignored
    for wd in (L.CE_ACT_BF16, L.CE_ACT_F16):                         # a 16-bit table is rounded to nearest only
        assert call(wd=wd, rnd=L.CE_ROUND_STOCHASTIC) == L.CE_ERR_UNSUPPORTED and "CE_ROUND_STOCHASTIC" in L.last_error()
    assert call(opt=L.CE_OPT_SGD, mom=None, mrows=0, eps=0.0) == L.CE_OK
    for bad in (dict(weight=None), dict(go=None), dict(ws=None), dict(mom=None)):
        assert call(**bad) == L.CE_ERR_INVALID, bad
    for bad in (dict(act=7), dict(wd=7), dict(opt=2), dict(rnd=2), dict(D=0), dict(lr=-1.0), dict(eps=0.0),
                dict(mrows=0), dict(ws=p[5] + 8), dict(wsb=ws_bytes - 1), dict(mode=2)):
        assert call(**bad) != L.CE_OK, bad
        assert L.last_error()
    assert call(act=7) == L.CE_ERR_INVALID and "activation dtype" in L.last_error()
    assert call(wd=7) == L.CE_ERR_INVALID and "weight_dtype" in L.last_error()
    assert call(opt=2) == L.CE_ERR_INVALID and "optimizer" in L.last_error()
    assert call(rnd=2) == L.CE_ERR_INVALID and "rounding" in L.last_error()
    assert call(wsb=ws_bytes - 1) == L.CE_ERR_INVALID and "workspace too small" in L.last_error()
    for bad in (dict(R=2 ** 31), dict(nnz=2 ** 31, wsb=2 ** 40), dict(nb=2 ** 31)):
        assert call(**bad) == L.CE_ERR_UNSUPPORTED and "2^31" in L.last_error(), bad
    # the 16-bit table's dim rule, and the lane shapes' limit for an fp32 table
    assert call(wd=L.CE_ACT_BF16, D=20) == L.CE_ERR_UNSUPPORTED and "dim % 8" in L.last_error()
    assert call(wd=L.CE_ACT_F16, weight=p[0] + 8) == L.CE_ERR_INVALID
    assert call(D=2048, wsb=2 ** 30) == L.CE_ERR_UNSUPPORTED and "too large for this build" in L.last_error()
