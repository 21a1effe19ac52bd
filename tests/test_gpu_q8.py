"""GPU tests of the 8-bit row-wise quantized table (q8: rows of 16 + D bytes, element = fma(code, scale, bias)): the
general and the key-driven forward against the host dequantizer, the cache while it evicts (every strategy and
transport), CachedEmbeddingBag.quantized() of a trained module, and the example's --eval_q8.  The reference table of
every forward test is ce_host_dequantize_q8 of the quantized rows, which tests/test_q8_cpu.py pins to the formula.  The
kernels only ever see in-range slots and the documented ignored slot -1."""
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


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _equal_cast(got: torch.Tensor, want32: torch.Tensor) -> None:
    """got == the cast of the fp32 values want32 to got's dtype, bit for bit"""
    if got.dtype == torch.float32:
        assert torch.equal(_bits(got), _bits(want32))
    else:
        assert_cast_equal(got.detach().cpu(), want32.to(got.dtype))


# ---- 5. general forward ----------------------------------------------------------------------------------------------

_FWD = {}


def _fwd_case(D):
    """shared inputs of one D: the quantized table, its dequantized rows, one-id bags and a multi-id layout, built once"""
    if D not in _FWD:
        from cachedembedding_amd.functional import dequantize_rows, quantize_rows
        rng = np.random.default_rng(200 + D)
        R, nb = 257, 130
        q = quantize_rows(torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)))
        assert q.shape == (R, 16 + D) and q.dtype == torch.uint8
        single = rng.integers(0, R, nb)
        lens = rng.integers(0, 21, nb)
        lens[3], lens[7] = 0, 9                                   # an empty bag, a 9-id bag
        off = np.concatenate([[0], np.cumsum(lens)])
        idx = rng.integers(0, R, int(off[-1]))
        idx[int(off[7]) + 2] = -1                                 # one ignored lookup
        psw = rng.random(len(idx)).astype(np.float32) + 0.5
        _FWD[D] = dict(R=R, nb=nb, q=q, deq=dequantize_rows(q, D), single=single, off=off, idx=idx, psw=psw, refs={})
    return _FWD[D]


@pytest.mark.parametrize("ot", OUT, ids=lambda d: "out_" + NAMES[d])
@pytest.mark.parametrize("D", [16, 48, 128, 272, 1024])
def test_general_forward(D, ot):
    from cachedembedding_amd.functional import embedding_bag
    c = _fwd_case(D)
    w = c["q"].cuda()
    nb = c["nb"]
    # (a) one id per bag, sum: the cast of the dequantized row, bit for bit
    ids = torch.from_numpy(c["single"]).cuda()
    for hook in (0, 5):
        out = embedding_bag(ids, w, torch.arange(nb + 1, device="cuda"), mode="sum", include_last_offset=True,
                            hook_features=hook, output_dtype=ot)
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
                                    masked_indices=mode == "sum")
                assert out.dtype == ot
                got = out.detach().cpu().double().numpy().reshape(r64.shape)
                if ot == torch.float32:
                    bound = np.asarray(L, np.float64).reshape(-1, 1) * U32 * asum        # the fp32 term alone
                else:
                    bound = forward_bound(r64, asum, L, ot)
                bad = int((np.abs(got - r64) > bound).sum())
                assert bad == 0, (mode, use_psw, hook, odt, bad)


def test_forward_defaults_to_fp32_and_takes_out():
    from cachedembedding_amd.functional import embedding_bag
    c = _fwd_case(16)
    ids, off = torch.from_numpy(c["single"]).cuda(), torch.arange(c["nb"] + 1, device="cuda")
    out = embedding_bag(ids, c["q"].cuda(), off, mode="sum", include_last_offset=True)
    assert out.dtype == torch.float32
    buf = torch.empty(c["nb"], 16, device="cuda", dtype=torch.bfloat16)
    got = embedding_bag(ids, c["q"].cuda(), off, mode="sum", include_last_offset=True, out=buf,
                        output_dtype=torch.bfloat16)
    assert got is buf
    _equal_cast(buf, out.cpu())


# ---- 6. key-driven forward -------------------------------------------------------------------------------------------

def _key_slots(D):
    """two batches of 1000 slots into the R = 257 rows of _fwd_case(D)"""
    rng = np.random.default_rng(1000 + D)
    slots = rng.integers(0, 257, (2, 1000))
    slots[:, :8] = [5, 6, 5, 5, 6, 0, 256, 5]                    # runs of equal rows, the first and the last row
    slots[1, 11] = -1                                            # an ignored lookup: a zero row
    return slots


@pytest.mark.parametrize("D", [16, 128, 272])
def test_key_driven_forward(D):
    """nnz = 1000: not a whole segment; two batches; keys from the window presort, with and without hook_features; one
    ignored lookup, whose output row is zero.  The 16-bit outputs are 16-byte aligned and D % 8 == 0."""
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
                                    presorted=keys[b], output_dtype=ot)
                assert out.data_ptr() % 16 == 0
                _equal_cast(out.view(-1, D), rows)
                if b == 1:
                    zero = out.view(-1, D)[(11 % (nnz // hook)) * hook + 11 // (nnz // hook) if hook else 11]
                    assert not _bits(zero).any()


@pytest.mark.parametrize("D", [16, 272])
def test_q8_forward_is_the_fp32_forward_over_the_dequantized_rows(D):
    """q8 is a row type of the two forward kernels, not kernels of its own: an fp32 table that holds dequantize_rows(q)
    gives the same output, bit for bit, in every output type.  D = 16: one chunk per lane; D = 272: two, the lanes' third
    masked.  One id per bag: the general forward, with and without hook_features, and the key-driven forward over the
    window presort's keys (nnz = 1000, one ignored lookup).  (Bags of several ids are not compared bit for bit: with
    per-sample weights the compiler contracts `sum + value * weight` differently for the two row types, in the separate
    q8 kernels before this as well -- profiles/q8_row_type_refactor.md; test_general_forward bounds those.)"""
    from cachedembedding_amd.functional import embedding_bag, presort_window
    c = _fwd_case(D)
    nb, R = c["nb"], c["R"]
    tables = (c["q"].cuda(), c["deq"].cuda())

    def same(ids, off, **kw):
        for ot in OUT:
            o8, o32 = (embedding_bag(ids, w, off, include_last_offset=True, output_dtype=ot, **kw) for w in tables)
            assert o8.dtype == ot and o32.dtype == ot and o8.shape == o32.shape
            assert torch.equal(_bits(o8), _bits(o32)), (NAMES[ot], kw.get("mode"), kw.get("hook_features"))

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


# ---- 7. through the cache --------------------------------------------------------------------------------------------

N_C, C_C, STEPS_C = 2000, 64, 20


def _cache_batches():
    """20 batches of 96 ids, 48 bags of 2: 48 distinct ids a batch (24 of 40 hot ids, 24 of the rest), each twice -- a
    64-row cache evicts from the second batch on"""
    rng = np.random.default_rng(19)
    out = []
    for _ in range(STEPS_C):
        u = np.concatenate([rng.choice(40, 24, replace=False), 40 + rng.choice(N_C - 40, 24, replace=False)])
        out.append(rng.permutation(np.concatenate([u, u])))
    return out


@pytest.mark.parametrize("transport", ["zerocopy", "staged", "worker"])
@pytest.mark.parametrize("strategy", ["DATASET", "LFU", "LRU"])
@pytest.mark.parametrize("D", [16, 128, 1024])      # 1024: rows of 65 16-byte units, one past the movers' 64-lane group
def test_through_the_cache(D, strategy, transport):
    import cachedembedding_amd as ce
    from cachedembedding_amd.functional import embedding_bag, quantize_rows
    x = torch.from_numpy(np.random.default_rng(D).standard_normal((N_C, D)).astype(np.float32))
    want_table = quantize_rows(x)
    emb = ce.CachedEmbeddingBag.from_pretrained(x, table_dtype=torch.uint8, mode="sum", include_last_offset=True,
                                                cuda_row_num=C_C, warmup_ratio=0.0,
                                                evict_strategy=ce.EvictionStrategy[strategy])
    emb.cache_weight_mgr.set_transport(transport)
    mgr = emb.cache_weight_mgr
    assert emb.table_dtype == torch.uint8 and emb.embedding_dim == D and mgr.embedding_dim == D
    assert emb.weight.dtype == torch.uint8 and emb.weight.shape == (N_C, 16 + D) and emb.element_size() == 1
    p = mgr.cuda_cached_weight
    assert p.dtype == torch.uint8 and p.shape == (C_C, 16 + D) and p.requires_grad is False
    assert next(emb.parameters()) is p and not emb.training
    before = emb.weight.clone()
    assert torch.equal(before, want_table)
    full = want_table.cuda()
    off = torch.arange(0, 97, 2, device="cuda")
    scale = torch.randn(48, D, device="cuda", requires_grad=True)
    for ids in _cache_batches():
        i = torch.from_numpy(ids).cuda()
        out = emb(i, off)
        assert out.dtype == torch.float32 and not out.requires_grad
        want = embedding_bag(i, full, off, mode="sum", include_last_offset=True)
        assert torch.equal(_bits(out), _bits(want))
    # a loss over the output: its backward reaches the other leaves and leaves the table alone
    loss = (out * scale).sum()
    loss.backward()
    assert scale.grad is not None and p.grad is None
    torch.cuda.synchronize()
    assert sum(emb.num_write_back_history) > 0 and sum(emb.num_miss_history) > C_C, "the cache never evicted"
    emb.flush()
    assert torch.equal(emb.weight, before), "a quantized table is never written"


# ---- 8. quantized() --------------------------------------------------------------------------------------------------

def test_quantized_of_a_trained_module():
    """A DATASET module with ids_freq_mapping (so ids are re-ranked: idx_map), a few fused-SGD steps, quantized().
    Bound on |q8 output - fp32 output| of a bag of L ids r: sum_r (scale_r / 2 + 4 ulp32(max |row_r|)) -- the
    reconstruction bound of tests/test_q8_cpu.py per lookup -- plus L * 2^-24 * (sum |fp32 terms| + sum |q8 terms|) for
    the two fp32 sums of L terms."""
    import cachedembedding_amd as ce
    N, D, C, B, L, lr = 2000, 32, 400, 64, 4, 2.0 ** -3
    rng = np.random.default_rng(41)
    freq = rng.integers(1, 1000, N)
    emb = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, ids_freq_mapping=freq,
                                evict_strategy=ce.EvictionStrategy.DATASET, init_seed=5)
    emb.set_fused_sgd(lr)
    off = torch.arange(0, B * L + 1, L, device="cuda")
    batches = [rng.choice(N, B * L, replace=False) for _ in range(5)]
    for ids in batches[:4]:
        out = emb(torch.from_numpy(ids).cuda(), off)
        out.backward(torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).cuda())
    q = emb.quantized()
    assert q.table_dtype == torch.uint8 and q.weight.shape == (N, 16 + D) and not q.training
    assert (q.mode, q.include_last_offset, q.padding_idx, q.evict_strategy, q.cuda_row_num) == \
        (emb.mode, emb.include_last_offset, emb.padding_idx, emb.evict_strategy, emb.cuda_row_num)
    imap = emb.cache_weight_mgr.idx_map
    assert not torch.equal(imap.cpu(), torch.arange(N, dtype=torch.int32)), "the test needs a re-ranked module"
    assert torch.equal(q.cache_weight_mgr.idx_map, imap)
    assert q.cache_weight_mgr.cuda_cached_weight.requires_grad is False
    big = emb.quantized(cuda_row_num=3 * C)
    assert big.cuda_row_num == 3 * C and big.cache_weight_mgr.cuda_cached_weight.shape == (3 * C, 16 + D)
    table = emb.weight.clone()                                      # flushed by quantized(); rows in row space
    qt = q.weight
    sc = qt[:, :4].contiguous().view(torch.float32).view(-1).double()
    amax = table.abs().max(dim=1).values
    ulp = (torch.nextafter(amax, torch.full_like(amax, float("inf"))) - amax).double()
    per_row = sc / 2 + 4 * ulp                                      # the reconstruction bound, by table row
    rows_of = imap.cpu().long()
    for ids in batches:
        i = torch.from_numpy(ids).cuda()
        with torch.no_grad():
            o32, o8, ob = emb(i, off).cpu().double(), q(i, off).cpu().double(), big(i, off)
        assert torch.equal(_bits(ob), _bits(q(i, off)))
        r = rows_of[torch.from_numpy(ids)].view(B, L)
        bound = per_row[r].sum(dim=1, keepdim=True) + L * U32 * (
            table[r].abs().double().sum(dim=1) + ce.dequantize_rows(qt[r.view(-1)], D).view(B, L, D).abs().double().sum(dim=1))
        err = (o8 - o32).abs()
        assert bool((err <= bound).all()), float((err - bound).max())
        assert float(err.max()) > 0                                 # (it IS another table)
    # the source module still trains, and the quantized copy does not follow it
    q_before = q.weight.clone()
    out = emb(torch.from_numpy(batches[4]).cuda(), off)
    out.backward(torch.ones_like(out))
    emb.flush()
    touched = rows_of[torch.from_numpy(batches[4])]
    assert not torch.equal(emb.weight[touched], table[touched])
    q.flush()
    assert torch.equal(q.weight, q_before)


# ---- 9. the example --------------------------------------------------------------------------------------------------

def test_dlrm_example_eval_q8(capsys):
    import importlib
    sys.path.insert(0, str(ROOT / "examples"))
    dm = importlib.import_module("dlrm_main")
    D = 32
    dm.main(["--dataset", "avazu", "--table_scale", "0.01", "--batch_size", "256", "--embedding_dim", str(D),
             "--dense_arch_layer_sizes", "64,32", "--over_arch_layer_sizes", "64,1", "--use_cache", "--cache_ratio", "0.03",
             "--use_freq", "--prefetch_num", "4", "--use_overlap", "--use_sparse_embed_grad", "--overlap_cache_op", "--fused_sgd",
             "--fold_hook", "--limit_train_batches", "16",
             "--learning_rate", "0.2", "--eval_acc", "--eval_q8", "--limit_val_batches", "2", "--limit_test_batches", "4"])
    out = capsys.readouterr().out
    assert out.count("AUROC over test set") == 1 and out.count("AUROC over test (q8 table) set") == 1
    line = [ln for ln in out.splitlines() if ln.startswith("{") and "test_auroc_q8" in ln]
    assert len(line) == 1
    res = json.loads(line[0])
    N = dm.main.model.sparse_modules.embed.num_embeddings
    assert res["table_bytes_q8"] == N * (16 + D) and res["table_bytes"] == N * D * 4
    assert np.isfinite(res["test_auroc_q8"]) and 0.0 <= res["test_accuracy_q8"] <= 1.0
    assert np.isfinite(res["test_auroc"])
    assert dm.main.results["test_auroc_q8"] == res["test_auroc_q8"]
    assert dm.main.model.sparse_modules.embed.table_dtype == torch.float32        # the trained module is put back
