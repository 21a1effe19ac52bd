"""CPU tests of the 16-bit embedding table: the new C entries are declared, exported and bound; the 16-bit host fill is
the cast of the fp32 fill; every new bag entry refuses from its arguments alone, before any launch; the Python refusals
come before a GPU is asked for; the reference's stochastic rounding has the properties the kernels are held to."""
import ctypes
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))

import table_dtype_ref as ref  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
ENTRY_POINTS = ["ce_host_fill_uniform_w16", "ce_bag_forward_w16", "ce_bag_forward_src_keys_w16",
                "ce_bag_backward_w16_workspace", "ce_bag_backward_update_w16", "ce_bag_backward_update_src_w16"]


def _lib():
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_w16_entry_points():
    _l = _lib()
    header = (ROOT / "include" / "ce_api.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_l.LIB_PATH)], capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", body), name
        assert re.search(rf" T {name}\b", out), name
        assert name in _l.SIGNATURES
    for name in ("CE_OPT_SGD", "CE_OPT_ROWWISE_ADAGRAD", "CE_ROUND_NEAREST", "CE_ROUND_STOCHASTIC"):
        val = re.search(rf"#define {name} (\d+)", header)
        assert val and getattr(_l, name) == int(val.group(1)), name
    assert _l.lib.ce_version() == 6
    assert ctypes.sizeof(_l.CeCacheConfig) == 112
    # acc fp32 [rows, D] + one flag byte per row + the step counter, each 256-byte aligned
    assert _l.lib.ce_bag_backward_w16_workspace(1000, 128) == 1000 * 128 * 4 + 1024 + 256
    assert _l.lib.ce_bag_backward_w16_workspace(-1, 128) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [1024, 7])
@pytest.mark.parametrize("threads", [1, 3])
def test_host_fill_w16_is_the_cast_of_the_fp32_fill(dtype, seed, threads):
    _l = _lib()
    n = 1000
    for lo, hi in ((-1e-3, 1e-3), (-3e-5, 3e-5)):              # the second range reaches fp16's subnormals
        f32 = np.zeros(n, np.float32)
        w16 = np.zeros(n, np.int16)
        assert _l.lib.ce_host_fill_uniform(f32.ctypes.data, n, lo, hi, seed, threads) == 0
        assert _l.lib.ce_host_fill_uniform_w16(w16.ctypes.data, n, lo, hi, seed, ref.CODES[dtype], threads) == 0
        want = torch.from_numpy(f32).to(dtype)
        assert torch.equal(torch.from_numpy(w16), want.view(torch.int16))
    assert _l.lib.ce_host_fill_uniform_w16(w16.ctypes.data, n, -1.0, 1.0, seed, _l.CE_ACT_F32, 1) == _l.CE_ERR_INVALID
    assert _l.lib.ce_host_fill_uniform_w16(None, n, -1.0, 1.0, seed, ref.CODES[dtype], 1) == _l.CE_ERR_INVALID


def test_w16_entries_refuse_from_their_arguments_before_their_first_launch():
    """Every refusal comes from the arguments alone -- nothing is launched, so the workspace stays zero-filled.  The
    pointers are made-up addresses, which is why this runs only where nothing could be launched."""
    if torch.cuda.is_available():
        pytest.skip("passes made-up addresses: only for machines without a GPU")
    _l = _lib()
    lib = _l.lib
    R, n = 1000, 64
    p = [0x7f0000000000 + 0x100000 * i for i in range(8)]            # non-null, 256-byte aligned
    BF, SGD, ADA, NEAR = _l.CE_ACT_BF16, _l.CE_OPT_SGD, _l.CE_OPT_ROWWISE_ADAGRAD, _l.CE_ROUND_NEAREST

    def calls(wd=BF, D=128, ws=p[6], ws_bytes=None, lr=0.1, opt=SGD, rnd=NEAR, act=_l.CE_ACT_F32, upd_only=False):
        if ws_bytes is None:
            ws_bytes = lib.ce_bag_backward_w16_workspace(R, D)
        bag = (p[1], n, p[2], 0, n, 1, None, _l.CE_MODE_SUM, 0)       # indices ... hook_features
        tail = (None, p[5], R, lr, 1e-8, opt, rnd, 0, ws, ws_bytes, None)   # row_of_slot ... stream
        out = [lambda: lib.ce_bag_backward_update_w16(p[0], wd, R, D, *bag, p[3], act, None, *tail),
               lambda: lib.ce_bag_backward_update_src_w16(p[0], wd, R, D, n, p[3], act, p[4], *tail)]
        if not upd_only:
            out += [lambda: lib.ce_bag_forward_w16(p[0], wd, R, D, *bag, p[3], act, None),
                    lambda: lib.ce_bag_forward_src_keys_w16(p[0], wd, R, D, n, p[4], p[3], act, None)]
        return out

    INV, UNS = _l.CE_ERR_INVALID, _l.CE_ERR_UNSUPPORTED
    cases = [(dict(wd=_l.CE_ACT_F32), INV, "16-bit table is CE_ACT_BF16 or CE_ACT_F16"),
             (dict(wd=7), INV, "16-bit table is CE_ACT_BF16 or CE_ACT_F16"),
             (dict(act=9), INV, "unknown activation dtype"),
             (dict(D=12), UNS, "dim % 8 == 0"),
             (dict(D=2048), UNS, "dim <= 1024"),
             (dict(ws_bytes=lib.ce_bag_backward_w16_workspace(R, 128) - 1, upd_only=True), INV, "workspace too small"),
             (dict(ws=p[6] + 64, upd_only=True), INV, "256-byte aligned"),
             (dict(lr=-0.1, upd_only=True), INV, "lr must be >= 0"),
             (dict(opt=5, upd_only=True), INV, "unknown optimizer"),
             (dict(rnd=5, upd_only=True), INV, "unknown rounding")]
    for kw, code, msg in cases:
        for call in calls(**kw):
            assert call() == code, (kw, _l.last_error())
            assert msg in _l.last_error(), (kw, _l.last_error())
    # row-wise Adagrad without its state
    bag = (p[1], n, p[2], 0, n, 1, None, _l.CE_MODE_SUM, 0)
    ws_bytes = lib.ce_bag_backward_w16_workspace(R, 128)
    rc = lib.ce_bag_backward_update_w16(p[0], BF, R, 128, *bag, p[3], _l.CE_ACT_F32, None, None, None, 0, 0.1, 1e-8, ADA,
                                        NEAR, 0, p[6], ws_bytes, None)
    assert rc == INV and "momentum" in _l.last_error()


def test_python_refusals_before_a_gpu_is_needed(monkeypatch):
    import torch.distributed as dist

    import cachedembedding_amd as ce
    from cachedembedding_amd import _lib
    from cachedembedding_amd.cache_mgr import HostTable
    from cachedembedding_amd.functional import FusedSGD, embedding_bag
    from cachedembedding_amd.modules import FusedSparseModules
    from cachedembedding_amd.parallel import (GraphedShardedWindow, ParallelCachedEmbeddingBag,
                                              RowwiseShardedEmbeddingBag)
    from cachedembedding_amd.tablewise import ParallelCachedEmbeddingBagTablewise
    gpu_asked = []
    monkeypatch.setattr(_lib, "require_gpu", lambda: gpu_asked.append(1) or (_ for _ in ()).throw(RuntimeError("gpu")))
    for bad in (torch.float64, torch.int8, "bf16"):
        with pytest.raises(NotImplementedError, match="table_dtype"):
            ce.CachedEmbeddingBag(100, 8, cache_ratio=0.1, table_dtype=bad)
        with pytest.raises(NotImplementedError, match="table_dtype"):
            HostTable.allocate(100, 8, bad)
    # dtype= keeps its refusal: the new keyword has its own name
    with pytest.raises(NotImplementedError, match="fp32 tables"):
        ce.CachedEmbeddingBag(100, 8, cache_ratio=0.1, dtype=torch.bfloat16)
    i, o = torch.zeros(2, dtype=torch.long), torch.arange(2)
    for dt in DTYPES:
        for D in (12, 2048):
            with pytest.raises(NotImplementedError, match="embedding_dim % 8 == 0"):
                ce.CachedEmbeddingBag(100, D, cache_ratio=0.1, table_dtype=dt)
            with pytest.raises(NotImplementedError, match="embedding_dim % 8 == 0"):
                HostTable.allocate(100, D, dt)
            with pytest.raises(NotImplementedError, match="embedding_dim % 8 == 0"):
                HostTable.wrap(torch.zeros(4, D, dtype=dt))
            with pytest.raises(NotImplementedError, match="embedding_dim % 8 == 0"):
                embedding_bag(i, torch.zeros(4, D, dtype=dt), o, mode="sum")
        w = torch.zeros(4, 8, dtype=dt)
        with pytest.raises(NotImplementedError, match="mode='max' with a 16-bit table"):
            embedding_bag(i, w, o, mode="max")
        with pytest.raises(NotImplementedError, match="max_norm with a 16-bit table"):
            embedding_bag(i, w, o, mode="sum", max_norm=1.0)
        with pytest.raises(NotImplementedError, match="sparse=True with a 16-bit table"):
            embedding_bag(i, w, o, mode="sum", sparse=True)
        with pytest.raises(NotImplementedError, match=r"FusedSGD\(deterministic=True\) with a 16-bit table"):
            embedding_bag(i, w, o, mode="sum", fused_sgd=FusedSGD(0.1, deterministic=True))
        with pytest.raises(NotImplementedError, match="per_sample_weights with a 16-bit table"):
            embedding_bag(i, w, o, mode="sum", per_sample_weights=torch.ones(2, requires_grad=True))
        for kw in (dict(mode="max"), dict(max_norm=1.0), dict(sparse=True)):
            with pytest.raises(NotImplementedError, match="with a 16-bit table"):
                ce.CachedEmbeddingBag(100, 8, cache_ratio=0.1, table_dtype=dt, **kw)
        with pytest.raises(NotImplementedError, match="RowwiseShardedEmbeddingBag with table_dtype"):
            RowwiseShardedEmbeddingBag(100, 8, table_dtype=dt)
        with pytest.raises(NotImplementedError, match="GraphedShardedWindow with table_dtype"):
            GraphedShardedWindow(None, 2, 8, None, None, 8, table_dtype=dt)
        with pytest.raises(NotImplementedError, match="ParallelCachedEmbeddingBagTablewise with table_dtype"):
            ParallelCachedEmbeddingBagTablewise([], 8, table_dtype=dt)
        with pytest.raises(NotImplementedError, match="use_tablewise_parallel=True, table_dtype"):
            FusedSparseModules([10, 10], 8, use_cache=True, use_tablewise_parallel=True, table_dtype=dt)
    # set_weight_rounding is meaningful only with a 16-bit table
    fake = ce.CachedEmbeddingBag.__new__(ce.CachedEmbeddingBag)
    fake.table_dtype = torch.float32
    with pytest.raises(ValueError, match="16-bit table"):
        ce.CachedEmbeddingBag.set_weight_rounding(fake, "nearest")
    assert not gpu_asked, "a refusal came after the GPU was asked for"
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    with pytest.raises(NotImplementedError, match="ParallelCachedEmbeddingBag with table_dtype.*on 2 ranks"):
        ParallelCachedEmbeddingBag(100, 8, mode="sum", group="fake", table_dtype=torch.bfloat16)
    assert not gpu_asked


def test_example_parses_the_table_flags_and_refuses_what_it_cannot_do(monkeypatch):
    sys.path.insert(0, str(ROOT / "examples"))
    import importlib
    dm = importlib.import_module("dlrm_main")
    args = dm.parse_args(["--use_cache"])
    assert args.table_dtype == "fp32" and args.weight_rounding == "stochastic"
    args = dm.parse_args(["--use_cache", "--table_dtype", "bf16", "--weight_rounding", "nearest"])
    assert args.table_dtype == "bf16" and args.weight_rounding == "nearest"
    with pytest.raises(NotImplementedError, match="--table_dtype fp16"):
        dm.main(["--use_cache", "--table_dtype", "fp16", "--use_tablewise"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="--table_dtype bf16"):
        dm.main(["--use_cache", "--table_dtype", "bf16"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_stochastic_rounding(dtype):
    """a representable value never moves; the result is always one of the two neighbours; a 0.25 fraction rounds up in
    0.25 +- 6 sigma of 2^18 draws"""
    rng = np.random.default_rng(3)
    k = ref.DROPPED_BITS[dtype]
    n = 1 << 18
    rnd = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    # representable values (the cast of anything), signs and zero included
    x = torch.from_numpy(rng.standard_normal(n).astype(np.float32) * 10).to(dtype).float().numpy()
    x[:2] = [0.0, -0.0]
    got = ref.stochastic_round(x, rnd, dtype)
    assert torch.equal(got.view(torch.int16), torch.from_numpy(x).to(dtype).view(torch.int16))
    # anything in range: one of the two neighbours
    x = (rng.standard_normal(n) * 100).astype(np.float32)
    x = x[np.abs(x) >= 2.0 ** -14]
    lo, hi = ref.neighbours(x, dtype)
    got = ref.stochastic_round(x, rnd[:len(x)], dtype).float().numpy()
    assert np.all((got == lo) | (got == hi))
    assert np.all(np.abs(lo) <= np.abs(x)) and np.all(np.abs(x) <= np.abs(hi))
    # a quarter of the way from 1.0 to the next representable value
    step = 2.0 ** (k - 23)
    for sign in (1.0, -1.0):
        x = np.full(n, sign * (1.0 + 0.25 * step), np.float32)
        got = ref.stochastic_round(x, rnd, dtype).float().numpy()
        assert np.all((got == sign) | (got == sign * (1.0 + step)))
        share = float((got != sign).mean())
        assert abs(share - 0.25) <= 6 * np.sqrt(0.25 * 0.75 / n), share
    # what stochastic rounding leaves to the nearest cast
    special = np.array([np.nan, np.inf, -np.inf, 3.4e38, 70000.0, 65519.0, 2.0 ** -15, 3e-8], np.float32)
    got = ref.stochastic_round(special, np.full(len(special), (1 << 16) - 1, np.uint32), dtype)
    want = torch.from_numpy(special).to(dtype)
    if dtype == torch.float16:
        ref.aref.assert_cast_equal(got, want)
    else:
        ref.aref.assert_cast_equal(got[:4], want[:4])
