"""CPU tests of the row refresh: the three new C entries refuse their arguments before any HIP call,
every Python refusal of refresh_rows / current_rows / refresh_from / quantize_rows_device comes before the GPU is asked
for, and the HOST quantizer -- the reference of tests/test_gpu_refresh.py -- does with the delicate rows of
tests/refresh_cases.py what include/ce_api.h says (so the GPU comparison against it cannot go vacuous)."""
import ctypes
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import refresh_cases as rc  # noqa: E402

F32 = np.float32


def _lib():
    from cachedembedding_amd import _lib
    return _lib


def _entry(bits):
    L = _lib()
    return L.lib.ce_quantize_rows_q4 if bits == 4 else L.lib.ce_quantize_rows_q8


# ---- the C entries ---------------------------------------------------------------------------------------------------

def test_entries_are_declared_and_bound():
    L = _lib()
    for name in ("ce_quantize_rows_q8", "ce_quantize_rows_q4", "ce_cache_install_rows"):
        assert name in L.SIGNATURES and getattr(L.lib, name) is not None
    assert L.lib.ce_version() == 6


@pytest.mark.parametrize("bits,dims", [(8, [8, 24, 1040]), (4, [16, 48])])
def test_quantizer_refuses_the_dim_rule(bits, dims):
    """the host entry's rule and words; no pointer is looked at (they are not even mapped)"""
    L = _lib()
    host = L.lib.ce_host_quantize_q4 if bits == 4 else L.lib.ce_host_quantize_q8
    for dim in dims:
        assert _entry(bits)(0x1000, L.CE_ACT_F32, 4, dim, 0x2000, 0x3000, None) == L.CE_ERR_UNSUPPORTED
        said = L.last_error()
        assert f"got {dim}" in said
        assert host(0x1000, L.CE_ACT_F32, 4, dim, 0x2000, 1) == L.CE_ERR_UNSUPPORTED and L.last_error() == said


@pytest.mark.parametrize("bits", [8, 4])
def test_quantizer_refuses_bad_arguments_before_any_hip_call(bits):
    L = _lib()
    f, dim = _entry(bits), 32
    assert f(0x1000, 3, 4, dim, 0x2000, 0x3000, None) == L.CE_ERR_INVALID and "src_dtype 3" in L.last_error()
    assert f(0x1000, -1, 4, dim, 0x2000, 0x3000, None) == L.CE_ERR_INVALID
    assert f(0x1000, L.CE_ACT_F32, -1, dim, 0x2000, 0x3000, None) == L.CE_ERR_INVALID
    assert "negative n_rows" in L.last_error()
    assert f(None, L.CE_ACT_F32, 0, dim, None, None, None) == L.CE_OK                     # n_rows == 0: nothing to do
    for src, dst, bad in ((None, 0x2000, 0x3000), (0x1000, None, 0x3000), (0x1000, 0x2000, None)):
        assert f(src, L.CE_ACT_F32, 4, dim, dst, bad, None) == L.CE_ERR_INVALID and "null pointer" in L.last_error()
    # misalignment: src 16 bytes for fp32 and 8 for a 16-bit source, dst 16, first_bad 8
    assert f(0x1008, L.CE_ACT_F32, 4, dim, 0x2000, 0x3000, None) == L.CE_ERR_INVALID and "aligned" in L.last_error()
    assert f(0x1004, L.CE_ACT_BF16, 4, dim, 0x2000, 0x3000, None) == L.CE_ERR_INVALID and "aligned" in L.last_error()
    assert f(0x1004, L.CE_ACT_F16, 4, dim, 0x2000, 0x3000, None) == L.CE_ERR_INVALID
    assert f(0x1000, L.CE_ACT_F32, 4, dim, 0x2008, 0x3000, None) == L.CE_ERR_INVALID and "dst" in L.last_error()
    assert f(0x1000, L.CE_ACT_F32, 4, dim, 0x2000, 0x3004, None) == L.CE_ERR_INVALID and "first_bad" in L.last_error()


def test_install_rows_refuses_a_null_handle():
    L = _lib()
    assert L.lib.ce_cache_install_rows(None, 0x1000, 4, 0x2000, None) == L.CE_ERR_INVALID
    assert "null handle" in L.last_error()
    assert L.lib.ce_cache_install_rows(None, None, 0, None, None) == L.CE_ERR_INVALID


# ---- the Python refusals, before the GPU is asked for ------------------------------------------------------------------

def _stub(**kw):
    base = dict(table_dtype=torch.uint8, fused_optimizer=None, num_embeddings=100, embedding_dim=32,
                cache_weight_mgr=SimpleNamespace(_idx_map=None))
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.fixture
def no_gpu(monkeypatch):
    """any request for the GPU fails the test that made it"""
    L = _lib()
    asked = []
    monkeypatch.setattr(L, "require_gpu", lambda: asked.append(1) or (_ for _ in ()).throw(RuntimeError("gpu")))
    yield asked
    assert not asked, "a refusal came after the GPU was asked for"


def test_refresh_rows_refusals(no_gpu):
    import cachedembedding_amd as ce
    refresh = ce.CachedEmbeddingBag.refresh_rows
    ids, rows = torch.arange(4), torch.zeros(4, 32)
    for layout in ("adam", "partial_rowwise_adam", "adagrad"):
        with pytest.raises(NotImplementedError, match=f"in-row layout \\(fused_optimizer='{layout}'\\)"):
            refresh(_stub(table_dtype=torch.float32, fused_optimizer=layout), ids, rows)
    with pytest.raises(NotImplementedError, match="^refresh_rows on SimpleNamespace \\(2 ranks\\): rows are refreshed in"):
        refresh(_stub(world_size=2), ids, rows)
    with pytest.raises(NotImplementedError, match="^refresh_rows on ParallelCachedEmbeddingBag \\(2 ranks\\): rows are"):
        refresh(_stub(_no_weight_decay="ParallelCachedEmbeddingBag", world_size=2), ids, rows)
    who = "ParallelCachedEmbeddingBagTablewise"                 # a shard module of the table-wise class: no world_size
    with pytest.raises(NotImplementedError, match=f"^refresh_rows on {who} \\(1 rank\\): rows are refreshed in"):
        refresh(_stub(_no_weight_decay=who), ids, rows)
    # the column-wise class on one rank is a single-process module: its checks go on to the rows
    with pytest.raises(ValueError, match=r"needs \[4, 32\] rows"):
        refresh(_stub(_no_weight_decay="ParallelCachedEmbeddingBag", world_size=1), ids, torch.zeros(4, 16))
    for bad_ids in (torch.arange(4, dtype=torch.int32), torch.arange(4).view(2, 2), [0, 1, 2, 3]):
        with pytest.raises(ValueError, match="ids as a 1-D torch.int64 tensor"):
            refresh(_stub(), bad_ids, rows)
    with pytest.raises(NotImplementedError, match="torch.float32, torch.bfloat16 or torch.float16"):
        refresh(_stub(), ids, torch.zeros(4, 32, dtype=torch.float64))
    for bad_rows in (torch.zeros(3, 32), torch.zeros(4, 16), torch.zeros(4 * 32), torch.zeros(4, 32, 1)):
        with pytest.raises(ValueError, match=r"needs \[4, 32\] rows"):
            refresh(_stub(), ids, bad_rows)
    # n == 0 is a no-op: it never reaches the GPU either
    assert refresh(_stub(), torch.zeros(0, dtype=torch.int64), torch.zeros(0, 32)) is None


def test_current_rows_and_refresh_from_refusals(no_gpu):
    import cachedembedding_amd as ce
    current, refresh_from = ce.CachedEmbeddingBag.current_rows, ce.CachedEmbeddingBag.refresh_from
    ids = torch.arange(4)
    with pytest.raises(NotImplementedError, match="^current_rows with a q8 \\(torch.uint8\\) table"):
        current(_stub(), ids)
    with pytest.raises(NotImplementedError, match="^current_rows with a q4 \\(torch.quint4x2\\) table"):
        current(_stub(table_dtype=torch.quint4x2), ids)
    with pytest.raises(NotImplementedError, match="^current_rows on SimpleNamespace \\(4 ranks\\)"):
        current(_stub(table_dtype=torch.float32, world_size=4), ids)
    with pytest.raises(ValueError, match="ids as a 1-D torch.int64 tensor"):
        current(_stub(table_dtype=torch.float32), ids.float())
    served, trainer = _stub(), _stub(table_dtype=torch.float32)
    with pytest.raises(ValueError, match="same num_embeddings \\(100; the source has 99\\)"):
        refresh_from(served, _stub(table_dtype=torch.float32, num_embeddings=99), ids)
    with pytest.raises(ValueError, match="same embedding_dim \\(32; the source has 64\\)"):
        refresh_from(served, _stub(table_dtype=torch.float32, embedding_dim=64), ids)
    with pytest.raises(NotImplementedError, match="in-row layout"):
        refresh_from(_stub(table_dtype=torch.float32, fused_optimizer="adam"), trainer, ids)
    with pytest.raises(NotImplementedError, match="^current_rows with a q8"):
        refresh_from(served, _stub(), ids)                      # a quantized source has no current_rows
    with pytest.raises(ValueError, match="ids as a 1-D torch.int64 tensor"):
        refresh_from(served, trainer, ids.int())


def test_quantize_rows_device_refusals(no_gpu):
    from cachedembedding_amd.functional import quantize_rows_device
    with pytest.raises(NotImplementedError, match="2-D torch.float32, torch.bfloat16 or torch.float16"):
        quantize_rows_device(torch.zeros(4, 32, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="2-D"):
        quantize_rows_device(torch.zeros(32))
    with pytest.raises(NotImplementedError, match="8 \\(q8\\) and 4 \\(q4\\)"):
        quantize_rows_device(torch.zeros(4, 32), bits=2)
    with pytest.raises(NotImplementedError, match="q8 \\(torch.uint8\\) table needs embedding_dim % 16"):
        quantize_rows_device(torch.zeros(4, 24))
    with pytest.raises(NotImplementedError, match="q4 \\(torch.quint4x2\\) table needs embedding_dim % 32"):
        quantize_rows_device(torch.zeros(4, 48), bits=4)
    with pytest.raises(ValueError, match="rows that are on the GPU"):
        quantize_rows_device(torch.zeros(4, 32))


# ---- the reference of the GPU tests ----------------------------------------------------------------------------------

def _host(x, bits):
    from cachedembedding_amd.functional import quantize_rows
    return quantize_rows(torch.from_numpy(np.ascontiguousarray(x, F32)), bits=bits).numpy()


def _words(rows):
    return np.ascontiguousarray(rows[:, :8]).view(np.uint32)           # [n, 2]: scale, bias


@pytest.mark.parametrize("bits,D", [(8, 16), (8, 128), (4, 32)])
def test_host_bias_is_the_first_zero(bits, D):
    """[1, +0, -0, 4, ...] stores bias 0x00000000, [1, -0, +0, 4, ...] 0x80000000, with the same codes"""
    rows = _host(rc.zero_sign_rows(D), bits)
    w = _words(rows)
    assert w[0, 1] == 0x00000000 and w[1, 1] == 0x80000000
    assert w[0, 0] == w[1, 0] and np.array_equal(rows[0, 16:], rows[1, 16:])


def test_host_subnormal_quotient():
    """i * 1e-40f at D = 16: scale 0x00001066 and codes 0, 17, 34, ...; i * 1e-44f: a zero quotient, scale 0, codes 0"""
    rows = _host(rc.subnormal_rows(16), 8)
    w = _words(rows)
    assert w[0, 0] == 0x00001066 and np.array_equal(rows[0, 16:], (17 * np.arange(16)).astype(np.uint8))
    assert w[1, 0] == 0 and not rows[1, 16:].any()
    # q4 at D = 32 divides by 15: both quotients are subnormal and not zero, and the codes reach 15
    rows4 = _host(rc.subnormal_rows(32), 4)
    assert all(0 < int(_words(rows4)[r, 0]) < 0x00800000 and int((rows4[r, 16:] >> 4).max()) == 15 for r in (0, 1))


def test_fixture_builder_places_every_special_row():
    for D, n in ((16, 257), (128, 9000), (1024, 257)):
        x = rc.quantizer_input(D, n)
        assert x.shape == (n, D) and x.dtype == F32 and np.isfinite(x).all()
        special = np.concatenate(list(rc.special_rows(D).values()))
        bits = {r.tobytes() for r in x}
        assert all(s.tobytes() in bits for s in special), "a special row is missing from the input"
        assert x[n - 1].tobytes() == special[-1].tobytes()               # one sits in the ragged last workgroup
    assert rc.quantizer_input(32, 1)[0].tobytes() == rc.zero_sign_rows(32)[1].tobytes()
    bad = rc.bad_rows_input(32, 50, {3: "nan", 9: "+inf", 11: "-inf", 20: "range"})
    assert np.isnan(bad[3]).sum() == 1 and np.isposinf(bad[9]).sum() == 1 and np.isneginf(bad[11]).sum() == 1
    with np.errstate(over="ignore"):
        assert np.isfinite(bad[20]).all() and not np.isfinite(bad[20].max() - bad[20].min())
    from cachedembedding_amd import CeError
    from cachedembedding_amd.functional import quantize_rows
    with pytest.raises(CeError, match="row 3 holds a NaN or an infinity"):
        quantize_rows(torch.from_numpy(bad))
