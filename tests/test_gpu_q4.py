"""GPU tests of the 4-bit row-wise quantized table (q4: rows of 16 + D / 2 bytes, two codes per byte, element =
fma(code, scale, bias)): the general and the key-driven forward against the host dequantizer, q4 as a row type of the
fp32 kernels, the cache while it evicts (every strategy and transport), CachedEmbeddingBag.quantized(bits=4) of a
trained module, and the example's --eval_q4.  The reference table of every forward test is ce_host_dequantize_q4 of the
quantized rows, which tests/test_q4_cpu.py pins to the formula.  R = 257 rows and 130 bags reach every lane arrangement:
D = 32 (8 lanes a row, 8 rows a wave), 96 (32 lanes, 8 of them masked), 128 (32 lanes), 288 (64 lanes, two chunks, the
second masked for 56 lanes), 1024 (four chunks).  The kernels only ever see in-range slots and the documented ignored
slot -1."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))

from activation_dtype_ref import assert_cast_equal, bag_ref64, forward_bound  # noqa: E402
from table_dtype_ref import U32  # noqa: E402

pytestmark = pytest.mark.gpu
OUT = [torch.float32, torch.bfloat16, torch.float16]
NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
Q4 = torch.quint4x2


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _equal_cast(got: torch.Tensor, want32: torch.Tensor) -> None:
    """got == the cast of the fp32 values want32 to got's dtype, bit for bit"""
    if got.dtype == torch.float32:
        assert torch.equal(_bits(got), _bits(want32))
    else:
        assert_cast_equal(got.detach().cpu(), want32.to(got.dtype))


# ---- general forward -------------------------------------------------------------------------------------------------

_FWD = {}


def _fwd_case(D):
    """shared inputs of one D: the quantized table, its dequantized rows, one-id bags and a multi-id layout, built once"""
    if D not in _FWD:
        from cachedembedding_amd.functional import dequantize_rows, quantize_rows
        rng = np.random.default_rng(400 + D)
        R, nb = 257, 130
        q = quantize_rows(torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)), bits=4)
        assert q.shape == (R, 16 + D // 2) and q.dtype == torch.uint8
        single = rng.integers(0, R, nb)
        lens = rng.integers(0, 21, nb)
        lens[3], lens[7] = 0, 9                                   # an empty bag, a 9-id bag
        off = np.concatenate([[0], np.cumsum(lens)])
        idx = rng.integers(0, R, int(off[-1]))
        idx[int(off[7]) + 2] = -1                                 # one ignored lookup
        psw = rng.random(len(idx)).astype(np.float32) + 0.5
        _FWD[D] = dict(R=R, nb=nb, q=q, deq=dequantize_rows(q, D, bits=4), single=single, off=off, idx=idx, psw=psw,
                       refs={})
    return _FWD[D]


@pytest.mark.parametrize("ot", OUT, ids=lambda d: "out_" + NAMES[d])
@pytest.mark.parametrize("D", [32, 96, 128, 288, 1024])
def test_general_forward(D, ot):
    from cachedembedding_amd.functional import embedding_bag
    c = _fwd_case(D)
    w = c["q"].cuda()
    nb = c["nb"]
    # (a) one id per bag, sum: the cast of the dequantized row, bit for bit
    ids = torch.from_numpy(c["single"]).cuda()
    for hook in (0, 5):
        out = embedding_bag(ids, w, torch.arange(nb + 1, device="cuda"), mode="sum", include_last_offset=True,
                            hook_features=hook, output_dtype=ot, quant_bits=4)
        assert out.dtype == ot and not out.requires_grad
        rows = c["deq"][torch.from_numpy(c["single"])]
        if hook:
            rows = rows.view(hook, nb // hook, D).transpose(0, 1).contiguous()       # bag f * B + b -> [b, f]
        _equal_cast(out.view(-1, D), rows.reshape(-1, D))
    # (b) bags of 0..20 ids
    idx = torch.from_numpy(c["idx"]).cuda()
    t32 = c["deq"].numpy()
    for mode, use_psw in (("sum", False), ("sum", True), ("mean", False)):
        for hook in (0, 5):
            rk = (mode, use_psw, hook)
            if rk not in c["refs"]:
                c["refs"][rk] = bag_ref64(t32, c["idx"], c["off"], c["psw"] if use_psw else None, mode, True, hook)
            r64, asum, L = c["refs"][rk]
            for odt in (torch.int32, torch.int64):
                out = embedding_bag(idx, w, torch.from_numpy(c["off"]).to(odt).cuda(), mode=mode,
                                    include_last_offset=True, hook_features=hook, output_dtype=ot,
                                    per_sample_weights=torch.from_numpy(c["psw"]).cuda() if use_psw else None,
                                    masked_indices=mode == "sum", quant_bits=4)
                assert out.dtype == ot
                got = out.detach().cpu().double().numpy().reshape(r64.shape)
                if ot == torch.float32:
                    bound = np.asarray(L, np.float64).reshape(-1, 1) * U32 * asum        # the fp32 term alone
                else:
                    bound = forward_bound(r64, asum, L, ot)
                bad = int((np.abs(got - r64) > bound).sum())
                assert bad == 0, (mode, use_psw, hook, odt, bad)


# ---- key-driven forward ----------------------------------------------------------------------------------------------

def _key_slots(D):
    """two batches of 1000 slots into the R = 257 rows of _fwd_case(D)"""
    rng = np.random.default_rng(3000 + D)
    slots = rng.integers(0, 257, (2, 1000))
    slots[:, :8] = [5, 6, 5, 5, 6, 0, 256, 5]                    # runs of equal rows, the first and the last row
    slots[1, 11] = -1                                            # an ignored lookup: a zero row
    return slots


@pytest.mark.parametrize("D", [32, 128, 288])
def test_key_driven_forward(D):
    """nnz = 1000: not a whole segment; two batches; keys from the window presort, with and without hook_features; one
    ignored lookup, whose output row is zero.  The outputs are 16-byte aligned."""
    from cachedembedding_amd.functional import embedding_bag, presort_window
    c = _fwd_case(D)
    R, nnz, P = c["R"], 1000, 2
    w = c["q"].cuda()
    slots = _key_slots(D)
    sl = torch.from_numpy(slots).cuda()
    off = torch.arange(nnz + 1, dtype=torch.int32, device="cuda")
    for hook in (0, 4):
        keys = presort_window(sl, R, offsets=off, include_last_offset=True, hook_features=hook, identity_bags=True)
        for b in range(P):
            rows = c["deq"][torch.from_numpy(np.maximum(slots[b], 0))].clone()
            rows[torch.from_numpy(slots[b] < 0)] = 0
            if hook:
                rows = rows.view(hook, nnz // hook, D).transpose(0, 1).contiguous()
            rows = rows.reshape(-1, D)
            for ot in OUT:
                out = embedding_bag(sl[b], w, off, mode="sum", include_last_offset=True, hook_features=hook,
                                    presorted=keys[b], output_dtype=ot, quant_bits=4)
                assert out.data_ptr() % 16 == 0
                _equal_cast(out.view(-1, D), rows)
                if b == 1:
                    zero = out.view(-1, D)[(11 % (nnz // hook)) * hook + 11 // (nnz // hook) if hook else 11]
                    assert not _bits(zero).any()


@pytest.mark.parametrize("D", [32, 288])
def test_q4_forward_is_the_fp32_forward_over_the_dequantized_rows(D):
    """q4 is a row type of the two forward kernels, not kernels of its own: an fp32 table that holds
    dequantize_rows(q, bits=4) gives the same output, bit for bit, in every output type.  One id per bag: the general
    forward, with and without hook_features, and the key-driven forward over the window presort's keys (nnz = 1000, one
    ignored lookup)."""
    from cachedembedding_amd.functional import embedding_bag, presort_window
    c = _fwd_case(D)
    nb, R = c["nb"], c["R"]
    tables = ((c["q"].cuda(), 4), (c["deq"].cuda(), 8))

    def same(ids, off, **kw):
        for ot in OUT:
            o4, o32 = (embedding_bag(ids, w, off, include_last_offset=True, output_dtype=ot, quant_bits=bits, **kw)
                       for w, bits in tables)
            assert o4.dtype == ot and o32.dtype == ot and o4.shape == o32.shape
            assert torch.equal(_bits(o4), _bits(o32)), (NAMES[ot], kw.get("mode"), kw.get("hook_features"))

    ids = torch.from_numpy(c["single"]).cuda()
    for hook in (0, 5):
        same(ids, torch.arange(nb + 1, device="cuda"), mode="sum", hook_features=hook)
    slots = _key_slots(D)
    sl = torch.from_numpy(slots).cuda()
    nnz = slots.shape[1]
    off = torch.arange(nnz + 1, dtype=torch.int32, device="cuda")
    for hook in (0, 4):
        keys = presort_window(sl, R, offsets=off, include_last_offset=True, hook_features=hook, identity_bags=True)
        for b in range(len(slots)):
            same(sl[b], off, mode="sum", hook_features=hook, presorted=keys[b])


# ---- through the cache -----------------------------------------------------------------------------------------------

N_C, C_C, STEPS_C = 2000, 64, 20
_CACHE = {}


def _cache_batches():
    """20 batches of 96 ids, 48 bags of 2: 48 distinct ids a batch (24 of 40 hot ids, 24 of the rest), each twice -- a
    64-row cache evicts from the second batch on (the stream of tests/test_gpu_q8.py)"""
    rng = np.random.default_rng(19)
    out = []
    for _ in range(STEPS_C):
        u = np.concatenate([rng.choice(40, 24, replace=False), 40 + rng.choice(N_C - 40, 24, replace=False)])
        out.append(rng.permutation(np.concatenate([u, u])))
    return out


def _cache_case(D):
    """the fp32 rows, their q4 rows, the dequantized host table and every step's expected output: a bag is two ids, and
    0 + a + b in fp32 is one rounding whatever adds it, so the CPU's a + b is the kernel's sum bit for bit"""
    if D not in _CACHE:
        from cachedembedding_amd.functional import dequantize_rows, quantize_rows
        x = torch.from_numpy(np.random.default_rng(D).standard_normal((N_C, D)).astype(np.float32))
        q = quantize_rows(x, bits=4)
        deq = dequantize_rows(q, D, bits=4)
        batches = _cache_batches()
        want = [deq[torch.from_numpy(ids[0::2])] + deq[torch.from_numpy(ids[1::2])] for ids in batches]
        _CACHE[D] = dict(x=x, q=q, batches=batches, want=want)
    return _CACHE[D]


@pytest.mark.parametrize("transport", ["zerocopy", "staged", "worker"])
@pytest.mark.parametrize("strategy", ["DATASET", "LFU", "LRU"])
@pytest.mark.parametrize("D", [32, 128, 1024])
def test_through_the_cache(D, strategy, transport):
    """the cache op moves 32-byte (D = 32), 80-byte (D = 128) and 528-byte (D = 1024: 33 of a 64-lane group's lanes)
    rows intact while it evicts"""
    import cachedembedding_amd as ce
    c = _cache_case(D)
    W = 16 + D // 2
    emb = ce.CachedEmbeddingBag.from_pretrained(c["x"], table_dtype=Q4, mode="sum", include_last_offset=True,
                                                cuda_row_num=C_C, warmup_ratio=0.0,
                                                evict_strategy=ce.EvictionStrategy[strategy])
    emb.cache_weight_mgr.set_transport(transport)
    mgr = emb.cache_weight_mgr
    assert emb.table_dtype == Q4 and mgr.table_dtype == Q4 and mgr.quant_bits == 4
    assert emb.embedding_dim == D and mgr.embedding_dim == D and mgr._lib_dim == W // 4
    assert emb.weight.dtype == torch.uint8 and emb.weight.shape == (N_C, W) and emb.element_size() == 1
    p = mgr.cuda_cached_weight
    assert p.dtype == torch.uint8 and p.shape == (C_C, W) and p.requires_grad is False
    assert next(emb.parameters()) is p and not emb.training
    before = emb.weight.clone()
    assert torch.equal(before, c["q"])
    off = torch.arange(0, 97, 2, device="cuda")
    scale = torch.randn(48, D, device="cuda", requires_grad=True)
    for ids, want in zip(c["batches"], c["want"]):
        out = emb(torch.from_numpy(ids).cuda(), off)
        assert out.dtype == torch.float32 and not out.requires_grad
        assert torch.equal(_bits(out), _bits(want))
    # a loss over the output: its backward reaches the other leaves and leaves the table alone
    loss = (out * scale).sum()
    loss.backward()
    assert scale.grad is not None and p.grad is None
    torch.cuda.synchronize()
    assert sum(emb.num_write_back_history) > 0 and sum(emb.num_miss_history) > C_C, "the cache never evicted"
    emb.flush()
    assert torch.equal(emb.weight, before), "a quantized table is never written"


def test_ready_q4_rows_are_taken_as_they_are():
    """from_pretrained(uint8 rows, table_dtype=torch.quint4x2): columns are 2 * (width - 16)"""
    import cachedembedding_amd as ce
    c = _cache_case(32)
    emb = ce.CachedEmbeddingBag.from_pretrained(c["q"].clone(), table_dtype=Q4, mode="sum", include_last_offset=True,
                                                cuda_row_num=C_C, warmup_ratio=0.0)
    assert emb.embedding_dim == 32 and emb.table_dtype == Q4 and torch.equal(emb.weight, c["q"])
    out = emb(torch.from_numpy(c["batches"][0]).cuda(), torch.arange(0, 97, 2, device="cuda"))
    assert torch.equal(_bits(out), _bits(c["want"][0]))


# ---- quantized(bits=4) -----------------------------------------------------------------------------------------------

def test_quantized_bits4_of_a_trained_module():
    """A DATASET module with ids_freq_mapping (so ids are re-ranked: idx_map), a few fused-SGD steps, quantized(bits=4).
    One id per bag: the q4 module's output is the row of dequantize_rows(quantize_rows(flushed table, bits=4)), bit for
    bit.  Bags of L = 4 ids: within L * 2^-24 * sum |terms| of the fp64 sum over those rows, the fp32 sum's bound."""
    import cachedembedding_amd as ce
    N, D, C, B, L, lr = 2000, 32, 400, 64, 4, 2.0 ** -3
    rng = np.random.default_rng(43)
    freq = rng.integers(1, 1000, N)
    emb = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, ids_freq_mapping=freq,
                                evict_strategy=ce.EvictionStrategy.DATASET, init_seed=5)
    emb.set_fused_sgd(lr)
    off = torch.arange(0, B * L + 1, L, device="cuda")
    batches = [rng.choice(N, B * L, replace=False) for _ in range(5)]
    for ids in batches[:4]:
        out = emb(torch.from_numpy(ids).cuda(), off)
        out.backward(torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).cuda())
    q = emb.quantized(bits=4)
    assert q.table_dtype == Q4 and q.weight.dtype == torch.uint8 and q.weight.shape == (N, 16 + D // 2)
    assert not q.training
    assert (q.mode, q.include_last_offset, q.padding_idx, q.evict_strategy, q.cuda_row_num, q.output_dtype) == \
        (emb.mode, emb.include_last_offset, emb.padding_idx, emb.evict_strategy, emb.cuda_row_num, emb.output_dtype)
    imap = emb.cache_weight_mgr.idx_map
    assert not torch.equal(imap.cpu(), torch.arange(N, dtype=torch.int32)), "the test needs a re-ranked module"
    assert torch.equal(q.cache_weight_mgr.idx_map, imap)
    assert q.cache_weight_mgr.cuda_cached_weight.requires_grad is False
    big = emb.quantized(bits=4, cuda_row_num=3 * C)
    assert big.cuda_row_num == 3 * C and big.cache_weight_mgr.cuda_cached_weight.shape == (3 * C, 16 + D // 2)
    q8 = emb.quantized()
    assert q8.table_dtype == torch.uint8 and q8.weight.shape == (N, 16 + D)     # without bits: still q8
    table = emb.weight.clone()                                      # flushed by quantized(); rows in row space
    want_q = ce.quantize_rows(table, bits=4)
    assert torch.equal(q.weight, want_q)
    deq = ce.dequantize_rows(want_q, D, bits=4)
    rows_of = imap.cpu().long()
    off1 = torch.arange(B * L + 1, device="cuda")
    for ids in batches:
        i = torch.from_numpy(ids).cuda()
        r = rows_of[torch.from_numpy(ids)]
        one, ob = q(i, off1), big(i, off1)
        assert torch.equal(_bits(one), _bits(deq[r])) and torch.equal(_bits(ob), _bits(one))
        terms = deq[r].view(B, L, D).double()
        err = (q(i, off).cpu().double() - terms.sum(dim=1)).abs()
        assert bool((err <= L * U32 * terms.abs().sum(dim=1)).all())
    with pytest.raises(NotImplementedError, match="quantized already"):
        q.quantized(bits=4)
    with pytest.raises(NotImplementedError, match="never updated"):
        q.set_fused_sgd(0.1)


# ---- the example -----------------------------------------------------------------------------------------------------

def test_dlrm_example_eval_q4(capsys):
    """--eval_q4 beside --eval_q8 on the toy data: both run and report; the AUROC differences are printed, not bounded
    (nobody has measured what 4-bit rows cost this toy model: profiles/q4_table.md records what this prints)"""
    import importlib
    sys.path.insert(0, str(ROOT / "examples"))
    dm = importlib.import_module("dlrm_main")
    D = 32
    dm.main(["--dataset", "avazu", "--table_scale", "0.01", "--batch_size", "256", "--embedding_dim", str(D),
             "--dense_arch_layer_sizes", "64,32", "--over_arch_layer_sizes", "64,1", "--use_cache", "--cache_ratio", "0.03",
             "--use_freq", "--prefetch_num", "4", "--use_overlap", "--use_sparse_embed_grad", "--overlap_cache_op", "--fused_sgd",
             "--fold_hook", "--limit_train_batches", "16", "--learning_rate", "0.2", "--eval_acc", "--eval_q8", "--eval_q4",
             "--limit_val_batches", "2", "--limit_test_batches", "4"])
    out = capsys.readouterr().out
    assert out.count("AUROC over test set") == 1 and out.count("AUROC over test (q4 table) set") == 1
    assert out.count("AUROC over test (q8 table) set") == 1
    line = [ln for ln in out.splitlines() if ln.startswith("{") and "test_auroc_q4" in ln]
    assert len(line) == 1
    res = json.loads(line[0])
    N = dm.main.model.sparse_modules.embed.num_embeddings
    assert res["table_bytes_q4"] == N * (16 + D // 2) and res["table_bytes"] == N * D * 4
    assert np.isfinite(res["test_auroc_q4"]) and 0.0 <= res["test_accuracy_q4"] <= 1.0
    assert np.isfinite(res["test_auroc"])
    r = dm.main.results
    assert r["test_auroc_q4"] == res["test_auroc_q4"] and np.isfinite(r["test_auroc_q8"])
    with capsys.disabled():
        print(f"\nAUROC fp32 {r['test_auroc']:.6f}; q4 - fp32 {r['test_auroc_q4'] - r['test_auroc']:+.6f}; "
              f"q8 - fp32 {r['test_auroc_q8'] - r['test_auroc']:+.6f}")
    assert dm.main.model.sparse_modules.embed.table_dtype == torch.float32        # the trained module is put back
