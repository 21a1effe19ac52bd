"""GPU tests of the row refresh: the device quantizer against the host quantizer byte for byte,
CachedEmbeddingBag.refresh_rows through a cache that has evicted (every transport; the rows a write-back may still carry
and the rows the previous job's staging buffer still holds included), plain tables, current_rows / refresh_from without a
flush, and the refusals that need the device.  The reference of every quantizer test is ce_host_quantize_q8 / _q4
(functional.quantize_rows), which tests/test_q8_cpu.py, tests/test_q4_cpu.py and tests/test_refresh_cpu.py pin to the
formula and to the delicate rows; comparisons are torch.equal on bytes, nowhere a tolerance."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import refresh_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu
Q4 = torch.quint4x2
SRC = [torch.float32, torch.bfloat16, torch.float16]
NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
SHAPES = [(8, D) for D in rc.Q8_DIMS] + [(4, D) for D in rc.Q4_DIMS]


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


# ---- 1. the quantizer against the host, byte for byte ------------------------------------------------------------------

@pytest.mark.parametrize("src", SRC, ids=lambda d: "src_" + NAMES[d])
@pytest.mark.parametrize("bits,D", SHAPES, ids=lambda v: str(v))
def test_device_quantizer_writes_the_hosts_bytes(bits, D, src):
    from cachedembedding_amd.functional import quantize_rows, quantize_rows_device
    for n in rc.ROW_COUNTS:
        x = rc.as_source(rc.quantizer_input(D, n), src)
        want = quantize_rows(x, bits=bits)
        if src == torch.float32 and n > 1:
            # the case is not vacuous: on the HOST the two zero-sign rows differ in their bias word alone
            z = quantize_rows(torch.from_numpy(rc.zero_sign_rows(D)), bits=bits)
            assert z[0, 4:8].tolist() == [0, 0, 0, 0] and z[1, 4:8].tolist() == [0, 0, 0, 0x80]
            assert torch.equal(z[0, :4], z[1, :4]) and torch.equal(z[0, 8:], z[1, 8:])
        got = quantize_rows_device(x.cuda(), bits=bits)
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == want.shape
        same = (got.cpu() == want).all(dim=1)
        if not bool(same.all()):
            r = int((~same).nonzero()[0])
            print(f"\nrow {r} of {n}, D={D}, q{bits}, {NAMES[src]}:\n device {got[r].cpu().tolist()}\n host   "
                  f"{want[r].tolist()}\n input  {x[r].float().tolist()}")
        assert torch.equal(got.cpu(), want), (n, int((~same).sum()))
    # out=: written in place and handed back
    out = torch.full((n, want.shape[1]), 0xAB, dtype=torch.uint8, device="cuda")
    assert quantize_rows_device(x.cuda(), bits=bits, out=out) is out and torch.equal(out.cpu(), want)
    assert quantize_rows_device(x[:0].cuda(), bits=bits).shape == (0, want.shape[1])


# ---- 2. bad rows -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", [{31: "nan", 100: "+inf", 200: "-inf", 250: "range"}, {5: "range", 6: "nan"},
                                   {256: "-inf"}, {0: "+inf", 255: "nan"}], ids=lambda w: "_".join(map(str, w)))
@pytest.mark.parametrize("bits,D", [(8, 48), (8, 272), (4, 128)], ids=lambda v: str(v))
def test_bad_rows_raise_what_the_host_raises(bits, D, where):
    from cachedembedding_amd import CeError
    from cachedembedding_amd.functional import quantize_rows, quantize_rows_device
    n = 257
    x = rc.bad_rows_input(D, n, where)
    t = torch.from_numpy(x)
    with pytest.raises(CeError) as host:
        quantize_rows(t, bits=bits)
    assert f"row {min(where)} holds" in str(host.value)
    out = torch.full((n, 16 + (D if bits == 8 else D // 2)), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(CeError) as dev:
        quantize_rows_device(t.cuda(), bits=bits, out=out)
    assert type(dev.value) is type(host.value) and str(dev.value) == str(host.value) and dev.value.code == host.value.code
    good = np.ones(n, bool)
    good[list(where)] = False
    x[~good] = 0
    want = quantize_rows(torch.from_numpy(x), bits=bits)
    assert torch.equal(out.cpu()[good], want[good]), "a good row beside a bad one differs from the host's"


# ---- 3. refresh_rows through the cache -------------------------------------------------------------------------------

N_C, C_C = 600, 64
_CASE = {}


def _case(bits, D):
    """the rows, their quantized form and the batches, built once per (bits, D)"""
    if (bits, D) not in _CASE:
        from cachedembedding_amd.functional import quantize_rows
        g = np.random.default_rng(100 * bits + D)
        x = torch.from_numpy(g.standard_normal((N_C, D)).astype(np.float32))
        new = torch.from_numpy((3.0 * g.standard_normal((N_C, D))).astype(np.float32))      # a new value for ANY row
        _CASE[(bits, D)] = dict(x=x, q=quantize_rows(x, bits=bits), new=new, qnew=quantize_rows(new, bits=bits),
                                batches=rc.cache_batches(N_C, 8))
    return _CASE[(bits, D)]


def _served(bits, D, strategy, transport):
    """a quantized module whose 64-row cache is full and has evicted; the rows the LAST call evicted"""
    import cachedembedding_amd as ce
    c = _case(bits, D)
    emb = ce.CachedEmbeddingBag.from_pretrained(c["x"], table_dtype=Q4 if bits == 4 else torch.uint8, mode="sum",
                                                include_last_offset=True, cuda_row_num=C_C, warmup_ratio=0.0,
                                                evict_strategy=ce.EvictionStrategy[strategy])
    mgr = emb.cache_weight_mgr
    mgr.set_transport(transport)
    off = torch.arange(0, 97, 2, device="cuda")
    for ids in c["batches"][:-1]:
        emb(torch.from_numpy(ids).cuda(), off)
    before = set(mgr.cached_idx_map.cpu().tolist()) - {-1}
    emb(torch.from_numpy(c["batches"][-1]).cuda(), off)
    after = set(mgr.cached_idx_map.cpu().tolist()) - {-1}
    assert sum(emb.num_write_back_history) > 0 and len(after) == C_C, "the cache is not full or never evicted"
    return emb, off, sorted(before - after), sorted(after)


def _state(emb):
    mgr = emb.cache_weight_mgr
    torch.cuda.synchronize()
    return dict(cached_idx_map=mgr.cached_idx_map.clone(), inverted=mgr.inverted_cached_idx.clone(),
                freq=None if mgr.freq_cnter is None else mgr.freq_cnter.clone(), hits=list(emb.num_hits_history),
                miss=list(emb.num_miss_history), wb=list(emb.num_write_back_history), totals=mgr.totals())


def _assert_state(emb, was):
    now = _state(emb)
    assert torch.equal(now["cached_idx_map"], was["cached_idx_map"]) and torch.equal(now["inverted"], was["inverted"])
    assert (was["freq"] is None and now["freq"] is None) or torch.equal(now["freq"], was["freq"])
    assert (now["hits"], now["miss"], now["wb"], now["totals"]) == (was["hits"], was["miss"], was["wb"], was["totals"])


def _refresh_ids(evicted_last, resident):
    """ids of the three groups (ids are rows here: no idx_map): resident now, never admitted, evicted by the last call"""
    seen = set(np.concatenate(_case(8, 16)["batches"]).tolist())         # (the batches do not depend on bits / D)
    never = [i for i in range(N_C) if i not in seen]
    assert resident and never and evicted_last, (len(resident), len(never), len(evicted_last))
    groups = dict(resident=resident[:12], never=never[:12], evicted_last=evicted_last[:12])
    ids = np.array(groups["evicted_last"] + groups["resident"] + groups["never"], np.int64)
    return groups, np.random.default_rng(5).permutation(ids)


@pytest.mark.parametrize("strategy", ["DATASET", "LFU"])
@pytest.mark.parametrize("transport", ["zerocopy", "staged", "worker"])
@pytest.mark.parametrize("bits,D", [(8, 16), (8, 128), (4, 32), (4, 128)], ids=lambda v: str(v))
def test_refresh_rows_through_the_cache(bits, D, transport, strategy):
    from cachedembedding_amd.functional import dequantize_rows
    c = _case(bits, D)
    emb, off, evicted_last, resident = _served(bits, D, strategy, transport)
    mgr = emb.cache_weight_mgr
    groups, ids = _refresh_ids(evicted_last, resident)
    was = _state(emb)
    tid = torch.from_numpy(ids)
    emb.refresh_rows(tid, c["new"][tid])
    # straight after the call: the host rows, the slots of the resident ones, and nothing else
    assert torch.equal(mgr._weight[tid], c["qnew"][tid]), "a host row does not hold the new value"
    slots = was["inverted"][torch.from_numpy(np.array(groups["resident"])).cuda()].long()
    assert bool((slots >= 0).all())
    assert torch.equal(mgr.cuda_cached_weight.data[slots].cpu(), c["qnew"][groups["resident"]])
    _assert_state(emb, was)
    # further batches; the first re-admits the rows the last call evicted (the worker transport would find their OLD
    # payload in the previous write-back job's staging buffer)
    table = c["q"].clone()
    table[tid] = c["qnew"][tid]
    deq = dequantize_rows(table, D, bits=bits)
    rng = np.random.default_rng(11)
    pool = np.setdiff1d(np.arange(N_C), ids)
    for k in range(3):
        first = np.concatenate([groups["evicted_last"], groups["never"][:6], groups["resident"][:6]]) if k == 0 else \
            rng.choice(ids, 24, replace=False)
        u = np.concatenate([first, rng.choice(pool, 48 - len(first), replace=False)]).astype(np.int64)
        b = rng.permutation(np.concatenate([u, u]))
        out = emb(torch.from_numpy(b).cuda(), off)
        want = deq[torch.from_numpy(b[0::2])] + deq[torch.from_numpy(b[1::2])]
        assert torch.equal(_bits(out), _bits(want)), (k, "an output still shows an old row")
    emb.flush()
    assert torch.equal(emb.weight, table), "after flush(): a refreshed row lost its value or another row changed"


# ---- 4. a bad row installs nothing -----------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,D,transport,strategy", [(8, 16, "worker", "LFU"), (4, 32, "zerocopy", "DATASET")])
def test_a_bad_row_installs_nothing(bits, D, transport, strategy):
    from cachedembedding_amd import CeError
    c = _case(bits, D)
    emb, off, evicted_last, resident = _served(bits, D, strategy, transport)
    mgr = emb.cache_weight_mgr
    _, ids = _refresh_ids(evicted_last, resident)
    tid = torch.from_numpy(ids)
    rows = c["new"][tid].clone()
    rows[7, 3] = float("nan")
    mgr.writeback_wait()
    was, table, cache = _state(emb), mgr._weight.clone(), mgr.cuda_cached_weight.data.clone()
    with pytest.raises(CeError, match="row 7 holds a NaN or an infinity"):
        emb.refresh_rows(tid, rows)
    _assert_state(emb, was)
    assert torch.equal(mgr._weight, table) and torch.equal(mgr.cuda_cached_weight.data, cache)


# ---- 5. plain tables -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", [(torch.float32, 20), (torch.bfloat16, 24)], ids=["fp32_20", "bf16_24"])
def test_refresh_rows_of_a_plain_table(dtype, D):
    import cachedembedding_amd as ce
    N, C = 300, 64
    emb = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, table_dtype=dtype, init_seed=3)
    mgr = emb.cache_weight_mgr
    mgr.set_transport("worker")
    emb.set_fused_rowwise_adagrad(0.1)                               # state outside the rows: left alone
    mgr.momentum1.fill_(0.25)
    off1 = torch.arange(49, device="cuda")
    with torch.no_grad():
        emb(torch.arange(100, 148, device="cuda"), off1)             # 48 rows beside the 45 preloaded ones: evictions
    resident = sorted(set(mgr.cached_idx_map.cpu().tolist()) - {-1})
    absent = [i for i in range(N) if i not in set(resident)]
    assert resident and absent
    ids = torch.tensor(resident[:9] + absent[:9])
    new = torch.from_numpy(np.random.default_rng(2).standard_normal((18, D)).astype(np.float32))
    before = emb.weight.clone()
    was = _state(emb)
    emb.refresh_rows(ids, new)
    want = new.to(dtype)                                             # (round to nearest)
    _assert_state(emb, was)
    assert torch.equal(_bits(mgr._weight[ids]), _bits(want))
    slots = mgr.inverted_cached_idx[ids[:9].cuda()].long()
    assert torch.equal(_bits(mgr.cuda_cached_weight.data[slots]), _bits(want[:9]))
    assert bool((mgr.momentum1 == 0.25).all())
    with torch.no_grad():
        out = emb(ids.cuda(), torch.arange(19, device="cuda"))       # one id per bag: the row itself
    assert torch.equal(_bits(out), _bits(want.to(out.dtype)))
    emb.flush()
    other = torch.ones(N, dtype=torch.bool)
    other[ids] = False
    assert torch.equal(_bits(emb.weight[ids]), _bits(want)) and torch.equal(_bits(emb.weight[other]), _bits(before[other]))


# ---- 6. current_rows / refresh_from without a flush ------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 4])
def test_refresh_from_a_trainer_without_a_flush(bits):
    import cachedembedding_amd as ce
    N, D, C, B, lr = 2000, 32, 400, 256, 2.0 ** -3
    rng = np.random.default_rng(43 + bits)
    freq = rng.integers(1, 1000, N)
    trainer = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, ids_freq_mapping=freq,
                                    evict_strategy=ce.EvictionStrategy.DATASET, init_seed=5)
    trainer.cache_weight_mgr.set_transport("worker")
    trainer.set_fused_sgd(lr)
    off = torch.arange(B + 1, device="cuda")

    def step(ids):
        out = trainer(torch.from_numpy(ids).cuda(), off)
        out.backward(torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).cuda())

    for _ in range(3):
        step(rng.choice(N, B, replace=False))
    served = trainer.quantized(bits=bits)
    imap = trainer.cache_weight_mgr.idx_map
    assert not torch.equal(imap.cpu(), torch.arange(N, dtype=torch.int32)), "the test needs a re-ranked module"
    probe = torch.from_numpy(rng.choice(N, 300, replace=False)).cuda()
    served(probe, torch.arange(301, device="cuda"))                  # the served cache is warm
    touched = [rng.choice(N, B, replace=False) for _ in range(4)]
    for ids in touched:
        step(ids)
    T = torch.from_numpy(np.unique(np.concatenate(touched)))
    assert trainer.cache_weight_mgr.cuda_available_row_num < C       # nothing below flushes the trainer
    cur = trainer.current_rows(T)
    assert cur.is_cuda and cur.dtype == torch.float32 and cur.shape == (len(T), D)
    cur = cur.clone()
    served.refresh_from(trainer, T)
    assert trainer.cache_weight_mgr.cuda_available_row_num < C, "current_rows / refresh_from flushed the trainer"
    trainer.flush()
    table = trainer.weight.clone()                                   # row space
    assert torch.equal(_bits(cur), _bits(table[imap.cpu().long()[T]])), "current_rows is not the flushed table's rows"
    assert torch.equal(served.weight, ce.quantize_rows(table, bits=bits)), "the served table is not the rebuilt one"
    fresh = trainer.quantized(bits=bits)
    for ids in touched + [probe.cpu().numpy()]:
        i = torch.from_numpy(np.asarray(ids)).cuda()
        o = torch.arange(len(ids) + 1, device="cuda")
        assert torch.equal(_bits(served(i, o)), _bits(fresh(i, o)))


@pytest.mark.parametrize("dtype,D,layout", [(torch.bfloat16, 24, None), (torch.float32, 20, "adam"),
                                            (torch.float32, 20, "adagrad")], ids=["bf16_24", "adam_20", "adagrad_20"])
def test_current_rows_of_16bit_and_in_row_tables(dtype, D, layout):
    """a 16-bit table is read as D / 2 floats, an in-row table gives the w part of its 3 D / 2 D wide rows; the slots are
    doubled in place (exact), so a resident row's value is in the cache alone until the flush"""
    import cachedembedding_amd as ce
    N, C = 300, 64
    emb = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, table_dtype=dtype,
                                fused_optimizer=layout, init_seed=3,
                                initial_accumulator_value=0.5 if layout == "adagrad" else 0.0)
    mgr = emb.cache_weight_mgr
    mgr.set_transport("worker")
    init = emb.weight.clone()
    mgr.prepare_ids(torch.arange(100, 148, device="cuda"))           # 48 rows beside the 45 preloaded ones: evictions
    mgr.cuda_cached_weight.data.mul_(2)
    resident = sorted(set(mgr.cached_idx_map.cpu().tolist()) - {-1})
    absent = [i for i in range(N) if i not in set(resident)]
    ids = torch.tensor(resident[:9] + absent[:9])
    cur = emb.current_rows(ids)
    assert cur.is_cuda and cur.dtype == dtype and cur.shape == (18, D) and cur.is_contiguous()
    cur = cur.clone()
    assert mgr.cuda_available_row_num < C, "current_rows flushed the module"
    assert torch.equal(_bits(cur[:9]), _bits(2 * init[ids[:9]])) and torch.equal(_bits(cur[9:]), _bits(init[ids[9:]]))
    emb.flush()
    assert torch.equal(_bits(cur), _bits(emb.weight[ids]))


# ---- the example -----------------------------------------------------------------------------------------------------

def test_dlrm_example_eval_refresh(capsys):
    """--eval_q8_refresh --eval_q4_refresh on the toy data, the overlapped window with the worker transport: the served
    copies are built before training and only ever refreshed from the bitmap of looked-up rows -- after the last
    evaluation each is byte-equal to a rebuild from the flushed trainer, so the bitmap missed no row that moved"""
    import importlib
    import json
    import cachedembedding_amd as ce
    sys.path.insert(0, str(HERE.parent / "examples"))
    dm = importlib.import_module("dlrm_main")
    D = 32
    dm.main(["--dataset", "avazu", "--table_scale", "0.01", "--batch_size", "256", "--embedding_dim", str(D),
             "--dense_arch_layer_sizes", "64,32", "--over_arch_layer_sizes", "64,1", "--use_cache", "--cache_ratio", "0.03",
             "--use_freq", "--prefetch_num", "4", "--use_overlap", "--use_sparse_embed_grad", "--overlap_cache_op",
             "--fused_sgd", "--fold_hook", "--limit_train_batches", "16", "--learning_rate", "0.2", "--epochs", "2",
             "--eval_acc", "--eval_q8_refresh", "--eval_q4_refresh", "--limit_val_batches", "2",
             "--limit_test_batches", "4"])
    out = capsys.readouterr().out
    assert out.count("AUROC over val (q8 table, refreshed) set") == 2
    assert out.count("AUROC over test (q4 table, refreshed) set") == 1
    line = [ln for ln in out.splitlines() if ln.startswith("{") and "test_auroc_q8_refresh" in ln]
    assert len(line) == 1
    res, r = json.loads(line[0]), dm.main.results
    embed = dm.main.model.sparse_modules.embed
    for bits in (8, 4):
        assert np.isfinite(res[f"test_auroc_q{bits}_refresh"]) and len(r[f"val_aurocs_q{bits}_refresh"]) == 2
        n = r[f"refreshed_rows_q{bits}"]
        assert len(n) == 3 and 0 < n[0] <= embed.num_embeddings and n[2] == 0      # (nothing trains before the test set)
    embed.flush()
    table = embed.weight.clone()
    for bits, served in dm.main.served.items():
        assert torch.equal(served.weight, ce.quantize_rows(table, bits=bits)), bits


# ---- 7. refusals that need the device --------------------------------------------------------------------------------

def test_refusals_on_the_device():
    import cachedembedding_amd as ce
    from cachedembedding_amd import _lib
    c = _case(8, 16)
    emb, off, evicted_last, resident = _served(8, 16, "DATASET", "zerocopy")
    mgr = emb.cache_weight_mgr
    mgr.writeback_wait()
    was, table, cache = _state(emb), mgr._weight.clone(), mgr.cuda_cached_weight.data.clone()

    def untouched():
        _assert_state(emb, was)
        assert torch.equal(mgr._weight, table) and torch.equal(mgr.cuda_cached_weight.data, cache)

    rows = c["new"][:4]
    with pytest.raises(ValueError, match="distinct ids"):
        emb.refresh_rows(torch.tensor([3, 9, 3, 11]), rows)
    untouched()
    with pytest.raises(IndexError, match=r"1 of the 4 ids are outside \[0, 600\)"):
        emb.refresh_rows(torch.tensor([3, 9, N_C, 11]), rows)
    untouched()
    with pytest.raises(IndexError, match="outside"):
        emb.refresh_rows(torch.tensor([3, -1, 5, 11]), rows)
    untouched()
    # a cache op begun and not finished: CE_ERR_INVALID, nothing written
    ids2 = torch.from_numpy(c["batches"][0]).cuda().view(1, -1)
    slots = torch.empty_like(ids2)
    mgr.prepare_ids_begin(ids2, slots)
    with pytest.raises(ce.CeError) as e:
        emb.refresh_rows(torch.tensor([3, 9, 5, 11]), rows)
    assert e.value.code == _lib.CE_ERR_INVALID and "has not been finished" in str(e.value)
    mgr.prepare_ids_finish()
    torch.cuda.synchronize()
    assert torch.equal(mgr._weight[torch.tensor([3, 9, 5, 11])], c["q"][torch.tensor([3, 9, 5, 11])])
    # a source with another id -> row map, and one of another size
    plain = ce.CachedEmbeddingBag(N_C, 16, mode="sum", include_last_offset=True, cuda_row_num=C_C, init_seed=1)
    ranked = ce.CachedEmbeddingBag(N_C, 16, mode="sum", include_last_offset=True, cuda_row_num=C_C, init_seed=1,
                                   ids_freq_mapping=np.arange(N_C))
    small = ce.CachedEmbeddingBag(N_C - 1, 16, mode="sum", include_last_offset=True, cuda_row_num=C_C)
    with pytest.raises(ValueError, match="same id -> row map"):
        emb.refresh_from(ranked, torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="same num_embeddings"):
        emb.refresh_from(small, torch.tensor([1, 2]))
    with pytest.raises(IndexError):
        plain.current_rows(torch.tensor([0, N_C]))
    emb.refresh_from(plain, torch.tensor([1, 2]))                    # the same (identity) map: taken
    assert torch.equal(emb.weight[1:3], ce.quantize_rows(plain.weight[1:3].contiguous()))
