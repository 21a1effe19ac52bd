"""CPU tests of the half-precision activations: the reference helper against known answers, the C ABI of the new entry
points, and every refusal that can be reached without a device."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

import activation_dtype_ref as ref  # noqa: E402

ENTRY_POINTS = ["ce_bag_forward_act", "ce_bag_forward_src_keys_act", "ce_bag_backward_dense_act",
                "ce_bag_backward_sgd_act", "ce_bag_backward_sgd_src_act", "ce_bag_backward_dense_src_act",
                "ce_bag_backward_rowwise_adagrad_act", "ce_bag_backward_rowwise_adagrad_src_act"]
DTYPES = [torch.bfloat16, torch.float16]


def _bits(t):
    return [x & 0xffff for x in t.view(torch.int16).tolist()]


def test_reference_cast_of_special_values_has_the_known_answers():
    f = lambda *v: torch.tensor(v, dtype=torch.float32)                       # noqa: E731
    # bf16: 8 bits of significand, ties to even; a value above 65504 stays finite
    assert _bits(ref.cast(f(1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -0.0, 70000.0),
                          torch.bfloat16)) == [0x3f80, 0x3f82, 0x3f81, 0x8000, 0x4789]
    # fp16: 11 bits, ties to even, inf from 65520 on, subnormals in steps of 2^-24 (2^-25 is a tie -> 0)
    assert _bits(ref.cast(f(1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 70000.0, -70000.0, 65504.0, 65519.9, 65520.0,
                            2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, -0.0), torch.float16)) == \
        [0x3c00, 0x3c02, 0x7c00, 0xfc00, 0x7bff, 0x7bff, 0x7c00, 0x0001, 0x0003, 0x0000, 0x0001, 0x8000]
    sv = ref.special_values()
    assert torch.isnan(sv[:4]).all() and torch.isinf(sv[4:6]).all()
    for dt in DTYPES:
        c = ref.cast(sv, dt)
        assert torch.isnan(c[:4]).all(), "NaN must stay NaN, quiet or signalling, either sign"
        assert _bits(c[4:6]) == ([0x7f80, 0xff80] if dt == torch.bfloat16 else [0x7c00, 0xfc00])
        ref.assert_cast_equal(c, c.clone())
    assert torch.isinf(ref.cast(sv, torch.float16)[6]) and torch.isfinite(ref.cast(sv, torch.bfloat16)[6])
    # the comparison: any NaN matches any NaN; -0.0 is not +0.0; one ulp is a difference
    a = torch.tensor([float("nan"), -0.0, 1.0], dtype=torch.bfloat16)
    ref.assert_cast_equal(a, torch.tensor([-float("nan"), -0.0, 1.0], dtype=torch.bfloat16))
    for other in ([float("nan"), 0.0, 1.0], [float("nan"), -0.0, 1.0078125], [0.0, -0.0, 1.0]):
        with pytest.raises(AssertionError):
            ref.assert_cast_equal(a, torch.tensor(other, dtype=torch.bfloat16))


def test_reference_bag_and_hook_order():
    W = np.arange(12, dtype=float).reshape(4, 3)
    r, s, L = ref.bag_ref64(W, [0, 1, 3, 9, 2], [0, 2, 4, 5], mode="sum")
    np.testing.assert_array_equal(r, [W[0] + W[1], W[3], W[2]])                # 9 is out of range: ignored
    np.testing.assert_array_equal(L, [2, 2, 1])
    r, s, _ = ref.bag_ref64(W, [0, 1, 3, 2], [0, 2, 4], mode="mean")
    np.testing.assert_array_equal(r, [(W[0] + W[1]) / 2, (W[3] + W[2]) / 2])
    r, s, _ = ref.bag_ref64(-W, [1, 2], [0, 2], psw=[2.0, 0.5])
    np.testing.assert_array_equal(r, [-(2 * W[1] + 0.5 * W[2])])
    np.testing.assert_array_equal(s, [2 * W[1] + 0.5 * W[2]])
    # F = 2, B = 2: bags 0, 1 = feature 0 of samples 0, 1; output row b * F + f
    r, _, _ = ref.bag_ref64(W, [0, 1, 2, 3], np.arange(5), hook_features=2)
    np.testing.assert_array_equal(r, [W[0], W[2], W[1], W[3]])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_bound_holds_for_two_summation_orders_that_round_differently(dtype):
    """bags of 40 ids, D = 128, uniform(-0.5, 0.5) rows: 262,144 elements.  Both fp32 summation orders are inside the
    bound, while they do NOT agree with each other after rounding -- which is why equality with the cast of one fp32
    result is not what the GPU tests assert."""
    rng = np.random.default_rng(0)
    nb, L, D, N = 2048, 40, 128, 5000
    W = (rng.random((N, D), dtype=np.float32) - 0.5)
    idx = rng.integers(0, N, nb * L)
    off = np.arange(0, nb * L + 1, L)
    r64, asum, Ls = ref.bag_ref64(W, idx, off)
    rows = W[idx].reshape(nb, L, D)
    fwd = np.zeros((nb, D), np.float32)
    bwd = np.zeros((nb, D), np.float32)
    for j in range(L):
        fwd += rows[:, j]
        bwd += rows[:, L - 1 - j]
    outs = [ref.cast(torch.from_numpy(x), dtype) for x in (fwd, bwd)]
    assert r64.size == 262144
    for o in outs:
        assert ref.violations(o, r64, asum, Ls) == 0
    differ = int((outs[0].view(torch.int16) != outs[1].view(torch.int16)).sum())
    assert differ > 0, "the two orders were expected to round some elements differently"
    # and the bound is a bound: two 16-bit ulps off is caught everywhere the value is not tiny
    off2 = (outs[0].float() * (1 + 4 * ref.UNIT_ROUNDOFF[dtype])).to(dtype)
    assert ref.violations(off2, r64, asum, Ls) > 0.9 * r64.size


def test_header_library_and_binding_agree_on_the_new_names_and_constants():
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    text = (ROOT / "include" / "ce_api.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", body), name
        assert re.search(rf" T {name}\b", out), name
        assert name in _lib.SIGNATURES
    for name, val in (("CE_ACT_F32", 0), ("CE_ACT_BF16", 1), ("CE_ACT_F16", 2)):
        assert re.search(rf"#define {name} {val}\b", body), name
        assert getattr(_lib, name) == val
    assert _lib.ACT_DTYPES == {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
    assert _lib.lib.ce_version() == 6 and re.search(r"#define CE_API_VERSION 6\b", body)


def test_unknown_activation_dtype_is_refused_without_a_gpu():
    """host-side check in front of everything else: no pointer is looked at, nothing is launched"""
    from cachedembedding_amd import _lib
    lib = _lib.lib
    bad = 3
    calls = [
        lambda a: lib.ce_bag_forward_act(None, 10, 8, None, 4, None, 0, 4, 1, None, 0, 0, None, a, None),
        lambda a: lib.ce_bag_forward_src_keys_act(None, 10, 8, 4, None, None, a, None),
        lambda a: lib.ce_bag_backward_dense_act(None, 10, 8, None, 4, None, 0, 4, 1, None, 0, 0, None, a, None, None),
        lambda a: lib.ce_bag_backward_sgd_act(None, 10, 8, None, 4, None, 0, 4, 1, None, 0, 0, None, a, 0.1, None, None),
        lambda a: lib.ce_bag_backward_sgd_src_act(None, 10, 8, 4, None, a, 0.1, None, None, None),
        lambda a: lib.ce_bag_backward_dense_src_act(None, 10, 8, 4, None, a, None, None),
        lambda a: lib.ce_bag_backward_rowwise_adagrad_act(None, 10, 8, None, 4, None, 0, 4, 1, None, 0, 0, None, a, None,
                                                          None, None, 10, 0.1, 1e-8, None, 0, None),
        lambda a: lib.ce_bag_backward_rowwise_adagrad_src_act(None, 10, 8, 4, None, a, None, None, None, 10, 0.1, 1e-8,
                                                              None, 0, None),
    ]
    for call in calls:
        for a in (bad, -1):
            assert call(a) == _lib.CE_ERR_INVALID
            assert "unknown activation dtype" in _lib.last_error()
        # a known dtype gets past that check and is stopped by the next one
        for a in (_lib.CE_ACT_F32, _lib.CE_ACT_BF16, _lib.CE_ACT_F16):
            assert call(a) == _lib.CE_ERR_INVALID
            assert "null pointer" in _lib.last_error()


def test_python_refusals_before_a_gpu_is_needed(monkeypatch):
    import torch.distributed as dist

    import cachedembedding_amd as ce
    from cachedembedding_amd import _lib
    from cachedembedding_amd.functional import embedding_bag
    from cachedembedding_amd.modules import FusedSparseModules
    from cachedembedding_amd.parallel import (GraphedShardedWindow, ParallelCachedEmbeddingBag,
                                              RowwiseShardedEmbeddingBag)
    from cachedembedding_amd.tablewise import ParallelCachedEmbeddingBagTablewise
    gpu_asked = []
    monkeypatch.setattr(_lib, "require_gpu", lambda: gpu_asked.append(1) or (_ for _ in ()).throw(RuntimeError("gpu")))
    w = torch.zeros(4, 2)
    i, o = torch.zeros(2, dtype=torch.long), torch.arange(2)
    for bad in (torch.float64, torch.int8, "bf16"):
        with pytest.raises(NotImplementedError, match="output_dtype"):
            embedding_bag(i, w, o, mode="sum", output_dtype=bad)
        with pytest.raises(NotImplementedError, match="output_dtype"):
            ce.CachedEmbeddingBag(100, 8, cache_ratio=0.1, output_dtype=bad)
    # dtype= keeps meaning the table's dtype
    with pytest.raises(NotImplementedError, match="fp32 tables"):
        ce.CachedEmbeddingBag(100, 8, cache_ratio=0.1, dtype=torch.bfloat16)
    for dt in DTYPES:
        with pytest.raises(NotImplementedError, match="RowwiseShardedEmbeddingBag.*exchange buffers are fp32"):
            RowwiseShardedEmbeddingBag(100, 8, output_dtype=dt)
        with pytest.raises(NotImplementedError, match="GraphedShardedWindow.*exchange buffers are fp32"):
            GraphedShardedWindow(None, 2, 8, None, None, 8, output_dtype=dt)
        with pytest.raises(NotImplementedError, match="ParallelCachedEmbeddingBagTablewise.*all-to-all"):
            ParallelCachedEmbeddingBagTablewise([], 8, output_dtype=dt)
        with pytest.raises(NotImplementedError, match="use_tablewise_parallel=True.*all-to-all"):
            FusedSparseModules([10, 10], 8, use_cache=True, use_tablewise_parallel=True, output_dtype=dt)
    assert not gpu_asked, "a refusal came after the GPU was asked for"
    # the column-wise module on more than one rank: refused in the constructor and in set_output_dtype
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    with pytest.raises(NotImplementedError, match="ParallelCachedEmbeddingBag.*on 2 ranks"):
        ParallelCachedEmbeddingBag(100, 8, mode="sum", group="fake", output_dtype=torch.bfloat16)
    assert not gpu_asked
    fake = ParallelCachedEmbeddingBag.__new__(ParallelCachedEmbeddingBag)
    fake.world_size = 2
    with pytest.raises(NotImplementedError, match="on 2 ranks"):
        ParallelCachedEmbeddingBag.set_output_dtype(fake, torch.float16)
    fake.world_size = 1                       # one rank (what FusedSparseModules builds on one device): accepted
    ParallelCachedEmbeddingBag.set_output_dtype(fake, torch.float16)
    assert fake.output_dtype == torch.float16
    ParallelCachedEmbeddingBag.set_output_dtype(fake, None)
    assert fake.output_dtype == torch.float32
    # with the dtype accepted, the next thing the constructors want is the GPU
    with pytest.raises(RuntimeError, match="gpu"):
        ce.CachedEmbeddingBag(100, 8, cache_ratio=0.1, output_dtype=torch.bfloat16)
    assert gpu_asked


def _dlrm():
    sys.path.insert(0, str(ROOT / "examples"))
    import importlib
    return importlib.import_module("dlrm_main")


def test_example_parses_the_flag_and_refuses_what_it_must(monkeypatch):
    dm = _dlrm()
    assert dm.parse_args(["--use_cache"]).embedding_output_dtype == "fp32"
    args = dm.parse_args(["--use_cache", "--embedding_output_dtype", "bf16", "--fused_sgd", "--window_keys",
                          "--fold_hook", "--graph_step", "--eval_acc"])
    assert args.embedding_output_dtype == "bf16"
    assert dm.parse_args(["--use_cache", "--embedding_output_dtype", "bf16", "--adagrad"]).adagrad
    with pytest.raises(SystemExit):                                           # fp16 is a library option only
        dm.parse_args(["--use_cache", "--embedding_output_dtype", "fp16"])
    with pytest.raises(NotImplementedError, match="--embedding_output_dtype bf16"):
        dm.main(["--use_cache", "--embedding_output_dtype", "bf16", "--use_tablewise"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="--embedding_output_dtype bf16"):
        dm.main(["--use_cache", "--embedding_output_dtype", "bf16", "--fused_sgd"])


def test_benchmark_fails_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([sys.executable, str(ROOT / "benchmarks" / "bench_activation_dtype.py"), "--table_scale", "0.001"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert r.returncode != 0 and "{" not in r.stdout
