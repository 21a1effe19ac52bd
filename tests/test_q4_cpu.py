"""CPU tests of the 4-bit row-wise quantized table format (q4, include/ce_api.h): the host quantizer bit for bit against
a numpy restatement of its formula, the reconstruction bound, the dequantizer against fp64, and every refusal -- in C
and in Python -- before a GPU is asked for.  The q8 file's tests with 15 in place of 255 and two codes per byte.

The formula, in fp32 with one rounding per operation: lo = min, hi = max, scale = (hi - lo) / 15, bias = lo,
q = clamp(rint((x - lo) / scale), 0, 15); a zero scale gives codes 0.  Element i is the low (even i) or high (odd i)
nibble of code byte i / 2.  Element value: fma(q, scale, bias).

Reconstruction bound: |dequantize(quantize(x)) - x| <= scale / 2 + 4 ulp32(max |row|), the q8 bound with the q4 scale:
scale / 2 is the rounding to a code; the ulp term covers the fp32 roundings of x - lo, of the division (together they
can move the quotient across a tie) and of the fma, each at most half an ulp of a value no larger than 2 max |row|."""
import numpy as np
import pytest
import torch

DIMS = [32, 96, 128, 288, 1024]
ROWS = 300
F32 = np.float32
Q4 = torch.quint4x2


def _lib():
    from cachedembedding_amd import _lib
    return _lib


_INPUTS = {}


def _inputs(D):
    """name -> [ROWS, D] fp32, no signed zeros among the row minima (the four kinds of tests/test_q8_cpu.py)"""
    if D in _INPUTS:
        return _INPUTS[D]
    rng = np.random.default_rng(7 + D)
    out = {}
    out["normal"] = rng.standard_normal((ROWS, D)).astype(F32)
    out["criteo_init"] = rng.uniform(-1 / 178e6, 1 / 178e6, (ROWS, D)).astype(F32)
    out["offset"] = (F32(100) + F32(1e-3) * rng.standard_normal((ROWS, D)).astype(F32)).astype(F32)
    edge = rng.standard_normal((ROWS, D)).astype(F32)
    edge[0] = F32(0.375)                                           # a constant row
    edge[1] = np.where(rng.random(D) < 0.5, F32(-2.5), F32(1.25))  # two distinct values
    edge[1, 0], edge[1, 1] = F32(-2.5), F32(1.25)
    edge[2] = (F32(1e-3) + rng.integers(0, 40, D).astype(F32) * F32(1.4e-45)).astype(F32)   # denormal range
    edge[2, 0], edge[2, 1] = F32(1e-3), F32(1e-3) + F32(39 * 1.4e-45)
    edge[3] = rng.integers(0, 200, D).astype(F32) * F32(1.4e-45) + F32(1.4e-45)           # denormal values
    out["edges"] = edge
    _INPUTS[D] = out
    return out


def _formula(x):
    """the quantizer in np.float32, step by step: (codes uint8 [n, D], scale [n], bias [n])"""
    x = np.asarray(x, F32)
    lo, hi = x.min(axis=1), x.max(axis=1)
    rng_ = (hi - lo).astype(F32)
    scale = (rng_ / F32(15)).astype(F32)
    d = (x - lo[:, None]).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (d / scale[:, None]).astype(F32)
    q = np.clip(np.rint(t), 0, 15)
    q[scale == 0] = 0
    scale = np.where(scale == 0, F32(0), scale).astype(F32)
    return q.astype(np.uint8), scale, lo.astype(F32)


def _quantize(x, threads=4, code=0):
    L = _lib()
    x = np.ascontiguousarray(x)
    n, D = x.shape
    out = np.full((n, 16 + D // 2), 0xAB, np.uint8)
    rc = L.lib.ce_host_quantize_q4(x.ctypes.data, code, n, D, out.ctypes.data, threads)
    return rc, out


def _parts(rows):
    """(codes [n, D] with the nibbles unpacked, scale, bias, pad bytes)"""
    scale = np.ascontiguousarray(rows[:, 0:4]).view(F32).reshape(-1)
    bias = np.ascontiguousarray(rows[:, 4:8]).view(F32).reshape(-1)
    packed = rows[:, 16:]
    q = np.empty((rows.shape[0], 2 * packed.shape[1]), np.uint8)
    q[:, 0::2] = packed & 15                                       # even elements: low nibbles
    q[:, 1::2] = packed >> 4                                       # odd elements: high nibbles
    return q, scale, bias, rows[:, 8:16]


def _ulp32(v):
    v = np.abs(np.asarray(v, F32))
    return (np.nextafter(v, F32(np.inf)) - v).astype(np.float64)


@pytest.mark.parametrize("D", DIMS)
def test_quantizer_bit_exact(D):
    L = _lib()
    assert L.lib.ce_q4_row_bytes(D) == 16 + D // 2 == L.q4_row_bytes(D)
    for name, x in _inputs(D).items():
        rc, rows = _quantize(x, threads=1)
        assert rc == L.CE_OK, (name, L.last_error())
        q, scale, bias, pad = _parts(rows)
        wq, wscale, wbias = _formula(x)
        assert np.array_equal(scale.view(np.uint32), wscale.view(np.uint32)), name
        assert np.array_equal(bias, wbias), name                         # (by value: no signed zeros among the minima)
        assert np.array_equal(q, wq), (name, int((q != wq).sum()))       # (both nibbles written: the buffer was 0xAB)
        assert not pad.any(), name
        for threads in (3, 16):
            rc, again = _quantize(x, threads=threads)
            assert rc == L.CE_OK and np.array_equal(again, rows), (name, threads)
    e = _inputs(D)["edges"]
    q, scale, bias, _ = _parts(_quantize(e)[1])
    assert scale[0] == 0 and not q[0].any() and bias[0] == F32(0.375)             # constant row: reproduces lo
    assert set(np.unique(q[1])) == {0, 15}                                        # two values: the two end codes
    assert q[1, 0] == 0 and q[1, 1] == 15                                         # element 0 low nibble, 1 high nibble
    assert scale[2] == 0 and not q[2].any() and bias[2] == F32(1e-3)              # denormal range: quotient 0
    assert not np.signbit(scale).any()                                            # never -0


def test_threads_split_many_rows_the_same():
    """more rows than one thread's share, so the split really happens"""
    x = np.random.default_rng(3).standard_normal((20000, 32)).astype(F32)
    a, b, c = (_quantize(x, threads=t)[1] for t in (1, 3, 16))
    assert np.array_equal(a, b) and np.array_equal(a, c)
    wq, wscale, _ = _formula(x)
    q, scale, _, _ = _parts(a)
    assert np.array_equal(q, wq) and np.array_equal(scale, wscale)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_16bit_source_is_its_exact_upconversion(dt):
    L = _lib()
    from cachedembedding_amd.functional import quantize_rows
    g = torch.Generator().manual_seed(5)
    x = torch.randn(ROWS, 96, generator=g).to(dt)
    x[4] = torch.tensor(6.0e-8 if dt == torch.float16 else 1e-39).to(dt) * torch.arange(96).to(dt)   # subnormals
    rc, rows = _quantize(x.view(torch.int16).numpy(), code=L.ACT_DTYPES[dt])
    assert rc == L.CE_OK
    rc, want = _quantize(x.float().numpy())
    assert rc == L.CE_OK and np.array_equal(rows, want)
    assert np.array_equal(quantize_rows(x, bits=4).numpy(), want)


@pytest.mark.parametrize("D", DIMS)
def test_reconstruction_bound(D):
    from cachedembedding_amd.functional import dequantize_rows, quantize_rows
    for name, x in _inputs(D).items():
        q = quantize_rows(torch.from_numpy(x), bits=4)
        assert q.dtype == torch.uint8 and q.shape == (ROWS, 16 + D // 2)
        back = dequantize_rows(q, D, bits=4)
        assert torch.equal(back, dequantize_rows(q, bits=4))              # dim defaults to 2 * (width - 16)
        back = back.numpy().astype(np.float64)
        _, scale, _, _ = _parts(q.numpy())
        err = np.abs(back - x.astype(np.float64))
        ulp = _ulp32(np.abs(x).max(axis=1))
        bound = scale.astype(np.float64)[:, None] / 2 + 4 * ulp[:, None]
        excess = ((err - scale.astype(np.float64)[:, None] / 2) / ulp[:, None]).max()
        print(f"D={D} {name}: worst error over scale/2, in ulp32(max|row|): {excess:.2f}")
        assert (err <= bound).all(), (name, float((err - bound).max()))


@pytest.mark.parametrize("D", DIMS)
def test_dequantizer_exact(D):
    """fmaf(q, scale, bias) == fp64 q * scale + bias rounded once: the fp64 expression is exact while the exponents of
    q * scale and bias differ by fewer than 25 bits (4 bits of q and 24 of scale: 28 bits of q * scale, 28 + 25 <= 53),
    which these inputs keep"""
    L = _lib()
    for name in ("normal", "criteo_init"):
        x = _inputs(D)[name]
        rows = _quantize(x)[1]
        q, scale, bias, _ = _parts(rows)
        nz = q.astype(np.float64) * scale.astype(np.float64)[:, None]
        with np.errstate(divide="ignore"):
            gap = np.abs(np.log2(np.where(nz > 0, nz, 1)) - np.log2(np.abs(bias.astype(np.float64)))[:, None])
        assert gap[nz > 0].max() < 25, name
        want = (nz + bias.astype(np.float64)[:, None]).astype(F32)
        for threads in (1, 5):
            got = np.empty((ROWS, D), F32)
            assert L.lib.ce_host_dequantize_q4(rows.ctypes.data, ROWS, D, got.ctypes.data, threads) == L.CE_OK
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


def test_c_refusals_without_a_gpu():
    L = _lib()
    lib = L.lib
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    for dim in (0, 16, 48, 1056, -32):
        assert lib.ce_q4_row_bytes(dim) == 0
        assert lib.ce_host_quantize_q4(p, 0, 1, dim, p, 1) == L.CE_ERR_UNSUPPORTED and "q4" in L.last_error()
        assert lib.ce_host_dequantize_q4(p, 1, dim, p, 1) == L.CE_ERR_UNSUPPORTED
        assert lib.ce_bag_forward_q4(p, 4, dim, p, 1, None, 0, 1, 1, None, 0, 0, p, 0, None) == L.CE_ERR_UNSUPPORTED
        assert "q4" in L.last_error()
        assert lib.ce_bag_forward_src_keys_q4(p, 4, dim, 1, p, p, 0, None) == L.CE_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError, match="q4"):
            L.check_q4_dim(dim)
    # null pointers, a negative row count, an unknown source type
    assert lib.ce_host_quantize_q4(None, 0, 1, 32, p, 1) == L.CE_ERR_INVALID and "null" in L.last_error()
    assert lib.ce_host_quantize_q4(p, 0, 1, 32, None, 1) == L.CE_ERR_INVALID
    assert lib.ce_host_dequantize_q4(None, 1, 32, p, 1) == L.CE_ERR_INVALID
    assert lib.ce_host_dequantize_q4(p, 1, 32, None, 1) == L.CE_ERR_INVALID
    assert lib.ce_host_quantize_q4(p, 0, -1, 32, p, 1) == L.CE_ERR_INVALID and "negative" in L.last_error()
    assert lib.ce_host_dequantize_q4(p, -1, 32, p, 1) == L.CE_ERR_INVALID
    assert lib.ce_host_quantize_q4(p, 7, 1, 32, p, 1) == L.CE_ERR_INVALID and "src_dtype" in L.last_error()
    a16 = (p + 15) & ~15
    fwd = lambda w, idx, out, **k: lib.ce_bag_forward_q4(w, k.get("rows", 4), 32, idx, 2, None, 0, 2, 1, None,  # noqa: E731
                                                          k.get("mode", 0), 0, out, k.get("act", 0), None)
    assert fwd(None, a16, a16) == L.CE_ERR_INVALID and "null" in L.last_error()
    assert fwd(a16, None, a16) == L.CE_ERR_INVALID
    assert fwd(a16, a16, None) == L.CE_ERR_INVALID
    assert fwd(a16 + 4, a16, a16) == L.CE_ERR_INVALID and "aligned" in L.last_error()
    assert fwd(a16, a16, a16 + 8) == L.CE_ERR_INVALID                                      # fp32 output: 16 bytes
    assert fwd(a16, a16, a16, act=9) == L.CE_ERR_INVALID
    assert fwd(a16, a16, a16, mode=2) == L.CE_ERR_UNSUPPORTED
    assert fwd(a16, a16, a16, rows=0) == L.CE_ERR_INVALID
    assert lib.ce_bag_forward_q4(a16, 4, 32, a16, 2 ** 31, a16, 0, 2, 1, None, 0, 0, a16, 0, None) == L.CE_ERR_UNSUPPORTED
    assert lib.ce_bag_forward_q4(a16, 4, 32, a16, 3, None, 0, 2, 1, None, 0, 0, a16, 0, None) == L.CE_ERR_INVALID
    keys = lambda w, k, out, nnz=2, act=0: lib.ce_bag_forward_src_keys_q4(w, 4, 32, nnz, k, out, act, None)  # noqa: E731
    assert keys(None, a16, a16) == L.CE_ERR_INVALID
    assert keys(a16, None, a16) == L.CE_ERR_INVALID
    assert keys(a16, a16, None) == L.CE_ERR_INVALID
    assert keys(a16 + 8, a16, a16) == L.CE_ERR_INVALID
    assert keys(a16, a16, a16, nnz=2 ** 31) == L.CE_ERR_UNSUPPORTED
    assert keys(a16, a16, a16, act=5) == L.CE_ERR_INVALID
    # nothing to do is not an error
    assert lib.ce_bag_forward_q4(None, 4, 32, None, 0, None, 0, 0, 1, None, 0, 0, None, 0, None) == L.CE_OK
    assert lib.ce_host_quantize_q4(None, 0, 0, 32, None, 1) == L.CE_OK


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_rows_are_named(bad):
    L = _lib()
    from cachedembedding_amd.functional import quantize_rows
    x = np.random.default_rng(1).standard_normal((9000, 32)).astype(F32)      # several threads' shares
    x[8123, 2] = bad
    x[5017, 9] = bad                                                           # the first one is what is named
    for threads in (1, 16):
        rc, _ = _quantize(x, threads=threads)
        assert rc == L.CE_ERR_INVALID and "row 5017 " in L.last_error(), L.last_error()
    with pytest.raises(L.CeError, match="row 5017 "):
        quantize_rows(torch.from_numpy(x), bits=4)


def test_a_range_that_overflows_fp32_is_refused():
    L = _lib()
    x = np.zeros((3, 32), F32)
    x[1, 0], x[1, 1] = F32(3e38), F32(-3e38)
    rc, _ = _quantize(x)
    assert rc == L.CE_ERR_INVALID and "row 1 " in L.last_error()


def test_python_refusals_before_a_gpu_is_needed(monkeypatch):
    import cachedembedding_amd as ce
    from cachedembedding_amd import _lib
    from cachedembedding_amd.cache_mgr import HostTable
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD, embedding_bag
    from cachedembedding_amd.modules import FusedSparseModules
    from cachedembedding_amd.parallel import (GraphedShardedWindow, ParallelCachedEmbeddingBag,
                                              RowwiseShardedEmbeddingBag)
    from cachedembedding_amd.pipeline import GraphedWindow, PrefetchWindow
    from cachedembedding_amd.tablewise import ParallelCachedEmbeddingBagTablewise
    gpu_asked = []
    monkeypatch.setattr(_lib, "require_gpu", lambda: gpu_asked.append(1) or (_ for _ in ()).throw(RuntimeError("gpu")))
    U8 = torch.uint8
    assert _lib.Q4 is Q4 and _lib.Q8 is U8
    # the neighbouring quantized types stay refused as table dtypes
    for other in (torch.quint8, torch.qint8, torch.quint2x4, "quint4x2"):
        with pytest.raises(NotImplementedError, match="table_dtype"):
            ce.CachedEmbeddingBag(100, 32, cache_ratio=0.1, table_dtype=other)
    for bits in (2, 16, None):
        with pytest.raises(NotImplementedError, match="8 \\(q8\\) and 4 \\(q4\\)"):
            ce.quantize_rows(torch.zeros(4, 32), bits=bits)
        with pytest.raises(NotImplementedError, match="8 \\(q8\\) and 4 \\(q4\\)"):
            ce.dequantize_rows(torch.zeros(4, 32, dtype=U8), bits=bits)
    # a q4 module without rows to quantize
    with pytest.raises(NotImplementedError, match="^a q4 \\(torch.quint4x2\\) table is built from trained rows"):
        ce.CachedEmbeddingBag(100, 32, cache_ratio=0.1, table_dtype=Q4)
    i, o = torch.zeros(2, dtype=torch.long), torch.arange(2)
    for D in (0, 16, 48, 1056):
        with pytest.raises(NotImplementedError, match="q4 \\(torch.quint4x2\\) table needs embedding_dim % 32 == 0"):
            ce.CachedEmbeddingBag(100, D, cache_ratio=0.1, table_dtype=Q4, _weight=torch.zeros(100, D))
        with pytest.raises(NotImplementedError, match="embedding_dim % 32 == 0"):
            HostTable.allocate(100, D, Q4)
        with pytest.raises(NotImplementedError, match="embedding_dim % 32 == 0"):
            HostTable.wrap(torch.zeros(4, 16 + D // 2, dtype=U8), quant_bits=4)
        with pytest.raises(NotImplementedError, match="embedding_dim % 32 == 0"):
            embedding_bag(i, torch.zeros(4, 16 + D // 2, dtype=U8), o, mode="sum", quant_bits=4)
        with pytest.raises(NotImplementedError, match="embedding_dim % 32 == 0"):
            ce.quantize_rows(torch.zeros(4, D), bits=4)
        with pytest.raises(NotImplementedError, match="embedding_dim % 32 == 0"):
            ce.CachedEmbeddingBag.from_pretrained(torch.zeros(100, D), table_dtype=Q4, cache_ratio=0.1)
    with pytest.raises(ValueError, match="q4 rows of dim 64 are 48 bytes wide"):
        ce.dequantize_rows(torch.zeros(4, 80, dtype=U8), 64, bits=4)
    w = torch.zeros(4, 32, dtype=U8)                                 # D = 32 as q4 rows
    for kw, what in ((dict(mode="max"), "mode='max'"), (dict(mode="sum", max_norm=1.0), "max_norm"),
                     (dict(mode="sum", sparse=True), "sparse=True"),
                     (dict(mode="sum", fused_sgd=FusedSGD(0.1)), "fused SGD"),
                     (dict(mode="sum", fused_sgd=FusedRowwiseAdagrad(0.1)), "fused SGD"),
                     (dict(mode="sum", per_sample_weights=torch.ones(2, requires_grad=True)), "per_sample_weights")):
        with pytest.raises(NotImplementedError, match="with a q4 \\(torch.quint4x2\\) table: it is forward only") as e:
            embedding_bag(i, w, o, quant_bits=4, **kw)
        assert what in str(e.value)
    with pytest.raises(NotImplementedError, match="8 \\(q8\\) and 4 \\(q4\\)"):
        embedding_bag(i, w, o, mode="sum", quant_bits=2)
    for kw in (dict(mode="max"), dict(max_norm=1.0), dict(sparse=True)):
        with pytest.raises(NotImplementedError, match="with a q4 \\(torch.quint4x2\\) table: it is forward only"):
            ce.CachedEmbeddingBag(100, 32, cache_ratio=0.1, table_dtype=Q4, _weight=torch.zeros(100, 32), **kw)
    with pytest.raises(NotImplementedError, match="freeze=False\\) with a q4 \\(torch.quint4x2\\)"):
        ce.CachedEmbeddingBag.from_pretrained(torch.zeros(100, 32), freeze=False, table_dtype=Q4, cache_ratio=0.1)
    # a weight that requires grad is detached and quantized like any other; what is refused is training it (freeze=False)
    # the update switches of a q4 module
    fake = ce.CachedEmbeddingBag.__new__(ce.CachedEmbeddingBag)
    fake.table_dtype, fake.mode = Q4, "sum"
    with pytest.raises(NotImplementedError, match="q4 \\(torch.quint4x2\\) table: a quantized table is never updated"):
        ce.CachedEmbeddingBag.set_fused_sgd(fake, 0.1)
    with pytest.raises(NotImplementedError, match="q4 \\(torch.quint4x2\\) table: a quantized table is never updated"):
        ce.CachedEmbeddingBag.set_fused_rowwise_adagrad(fake, 0.1)
    with pytest.raises(ValueError, match="16-bit table"):
        ce.CachedEmbeddingBag.set_weight_rounding(fake, "nearest")
    with pytest.raises(NotImplementedError, match="of a q4 \\(torch.quint4x2\\) module: it is quantized already"):
        ce.CachedEmbeddingBag.quantized(fake)
    with pytest.raises(NotImplementedError, match="of a q4 \\(torch.quint4x2\\) module: it is quantized already"):
        ce.CachedEmbeddingBag.quantized(fake, bits=4)
    # quantized(bits=4) of an fp32 module: what a quantized table does not take, a bad width, several ranks
    src = ce.CachedEmbeddingBag.__new__(ce.CachedEmbeddingBag)
    src.table_dtype, src.mode, src.max_norm, src.embedding_dim = torch.float32, "max", None, 32
    with pytest.raises(NotImplementedError, match="mode='max' with a q4 \\(torch.quint4x2\\) table"):
        ce.CachedEmbeddingBag.quantized(src, bits=4)
    with pytest.raises(NotImplementedError, match="mode='max' with a q8 \\(torch.uint8\\) table"):
        ce.CachedEmbeddingBag.quantized(src)
    with pytest.raises(NotImplementedError, match="8 \\(q8\\) and 4 \\(q4\\)"):
        ce.CachedEmbeddingBag.quantized(src, bits=3)
    src.mode, src.embedding_dim = "sum", 48
    with pytest.raises(NotImplementedError, match="embedding_dim % 32 == 0"):
        ce.CachedEmbeddingBag.quantized(src, bits=4)
    src.world_size = 2
    with pytest.raises(NotImplementedError, match="quantized\\(\\) on 2 ranks with a q4 \\(torch.quint4x2\\) table"):
        ce.CachedEmbeddingBag.quantized(src, bits=4)
    # the classes a q4 table is not wired into: one message each
    with pytest.raises(NotImplementedError, match="^RowwiseShardedEmbeddingBag with a q4 \\(torch.quint4x2\\)"):
        RowwiseShardedEmbeddingBag(100, 32, table_dtype=Q4)
    with pytest.raises(NotImplementedError, match="^GraphedShardedWindow with a q4"):
        GraphedShardedWindow(None, 2, 8, None, None, 8, table_dtype=Q4)
    with pytest.raises(NotImplementedError, match="^ParallelCachedEmbeddingBagTablewise with a q4"):
        ParallelCachedEmbeddingBagTablewise([], 32, table_dtype=Q4)
    with pytest.raises(NotImplementedError, match="^ParallelCachedEmbeddingBag with a q4"):
        ParallelCachedEmbeddingBag(100, 32, table_dtype=Q4)
    with pytest.raises(NotImplementedError, match="^FusedSparseModules with a q4"):
        FusedSparseModules([10, 10], 32, use_cache=True, table_dtype=Q4)
    with pytest.raises(NotImplementedError, match="^PrefetchWindow with a q4"):
        PrefetchWindow(fake, 2)
    with pytest.raises(NotImplementedError, match="^GraphedWindow with a q4"):
        GraphedWindow(fake, 2, 8, None)
    assert not gpu_asked, "a refusal came after the GPU was asked for"


def test_uint8_alone_still_means_q8(monkeypatch):
    """a uint8 tensor's width cannot tell the formats apart ([R, 48] is D = 32 as q8 and D = 64 as q4): without
    quant_bits every entry point takes it for q8 rows, and only quant_bits=4 reaches the q4 entries"""
    import cachedembedding_amd as ce
    from cachedembedding_amd import _lib, functional
    from cachedembedding_amd.cache_mgr import HostTable

    class Reached(Exception):
        pass

    class FakeLib:
        def __getattr__(self, name):
            def entry(*args):
                raise Reached(name, args)
            return entry

    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    monkeypatch.setattr(functional, "lib", FakeLib())
    monkeypatch.setattr(functional, "stream_ptr", lambda: 0)

    class Cuda(torch.Tensor):                                       # a CPU tensor that says it is on the GPU
        is_cuda = True

    w = torch.zeros(4, 48, dtype=torch.uint8).as_subclass(Cuda)
    i, o = torch.zeros(2, dtype=torch.long), torch.arange(3)
    for kw, entry, dim in (({}, "ce_bag_forward_q8", 32), (dict(quant_bits=8), "ce_bag_forward_q8", 32),
                           (dict(quant_bits=4), "ce_bag_forward_q4", 64)):
        with pytest.raises(Reached) as e:
            functional.embedding_bag(i, w, o, mode="sum", include_last_offset=True, **kw)
        name, args = e.value.args
        assert name == entry and args[2] == dim, (kw, name, args[2])
    monkeypatch.undo()
    # the host side, for real: 48-byte rows are D = 32 to dequantize_rows, D = 64 with bits=4
    q8 = ce.quantize_rows(torch.randn(5, 32))
    q4 = ce.quantize_rows(torch.randn(5, 64), bits=4)
    assert q8.shape == q4.shape == (5, 48) and q8.dtype == q4.dtype == torch.uint8
    assert ce.dequantize_rows(q8).shape == (5, 32) and ce.dequantize_rows(q4, bits=4).shape == (5, 64)
    assert torch.equal(ce.quantize_rows(torch.ones(3, 32), 0), ce.quantize_rows(torch.ones(3, 32), threads=0, bits=8))
    t = HostTable.__new__(HostTable)
    HostTable.__init__(t, torch.zeros(4, 48, dtype=torch.uint8), 0, 0, False)
    assert t.quant_bits == 8
    t._fin.detach()


def test_example_parses_eval_q4_and_refuses_what_it_must(monkeypatch):
    import importlib
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "examples"))
    dm = importlib.import_module("dlrm_main")
    a = dm.parse_args(["--use_cache", "--eval_acc"])
    assert not a.eval_q4 and not a.eval_q8
    a = dm.parse_args(["--use_cache", "--eval_acc", "--eval_q4"])
    assert a.eval_q4 and not a.eval_q8
    a = dm.parse_args(["--use_cache", "--eval_acc", "--eval_q4", "--eval_q8"])
    assert a.eval_q4 and a.eval_q8
    with pytest.raises(ValueError, match="--eval_q4 needs --eval_acc"):
        dm.main(["--use_cache", "--eval_q4"])
    with pytest.raises(NotImplementedError, match="--eval_q4"):
        dm.main(["--use_cache", "--eval_acc", "--eval_q4", "--use_tablewise"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="--eval_q4"):
        dm.main(["--use_cache", "--eval_acc", "--eval_q4"])
