"""fp32 / bf16 / fp16 pooled output and incoming gradient on the same windows (one process, device events).

The package's synthetic Criteo-shaped tables (configs[2] = criteo_1tb at --table_scale 1.0; default 0.1), B = 16384,
F = 26, D = 128, a 1 % cache, prefetch window P = 8 with source-row keys: the forward from the window's keys
(k_bag_fwd_keys) + the fused SGD streaming backward (k_bag_bwd_stream), the cache op outside the timed range.  Three
modules -- one per activation dtype -- share nothing but the generator's windows; the dtypes alternate window by window.
Prints ONE JSON line: ms per step and lookups/s of each dtype and the algorithmic bytes of the two kernels from the
shapes; ends by checking, per 16-bit dtype, one step on sampled rows: the output bit for bit against the cast of the
cache rows, the updated rows against the fp32 module's arithmetic on the upcast gradient."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import cachedembedding_amd as ce  # noqa: E402
from cachedembedding_amd import synthetic  # noqa: E402
from cachedembedding_amd.pipeline import PrefetchWindow  # noqa: E402

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def algorithmic_bytes(nnz: int, D: int, act_bytes: int, unique_rows: int) -> dict:
    """compulsory traffic of the two kernels at this shape: keys read once (8 B per lookup); forward = a row load per
    unique row + the output; backward = the gradient rows + a read-modify-write per unique row"""
    return {"fwd_keys": nnz * 8 + unique_rows * D * 4 + nnz * D * act_bytes,
            "bwd_stream": nnz * 8 + nnz * D * act_bytes + 2 * unique_rows * D * 4}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--dataset", default="criteo_1tb", choices=list(synthetic.TABLES))
    # three host tables are pinned (one per dtype): 273 GB at 1.0, so the default is a tenth
    p.add_argument("--table_scale", type=float, default=0.1)
    p.add_argument("--batch_size", type=int, default=16384)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--cache_ratio", type=float, default=0.01)
    p.add_argument("--prefetch_num", type=int, default=8)
    p.add_argument("--windows", type=int, default=9, help="timed windows per dtype")
    p.add_argument("--warmup_windows", type=int, default=3)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--check_rows", type=int, default=4096)
    p.add_argument("--seed", type=int, default=1024)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("bench_activation_dtype needs a HIP device (MI355X): there is no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sizes = synthetic.scale_tables(synthetic.TABLES[a.dataset], a.table_scale)
    N, D, B, F, P = int(sum(sizes)), a.dim, a.batch_size, len(sizes), a.prefetch_num
    C = int(N * a.cache_ratio)
    nnz = F * B
    gen = synthetic.SyntheticKJT(sizes, B, 1, "power_law", 0.25, seed=a.seed, device=dev)
    off = torch.arange(nnz + 1, dtype=torch.int32, device=dev)
    layout = (off, True, F)
    g32 = torch.randn(B, F, D, device=dev) * 1e-2
    # every module gets the gradient in its own dtype; the fp32 one is what a trainer without autocast hands back
    grads = {n: g32.to(dt) for n, dt in DTYPES.items()}

    def module(dt):
        emb = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, strict=False,
                                    init_seed=a.seed, output_dtype=dt)
        emb.set_cache_op(False)
        emb.set_fused_sgd(a.lr)
        return emb, PrefetchWindow(emb, P, overlap=False, presort=True, bag_layout=layout)

    mods = {n: module(dt) for n, dt in DTYPES.items()}
    ms = {n: [] for n in mods}
    names = list(mods)
    uniq = []
    for w in range(a.warmup_windows + a.windows):
        values = gen.next_values(P)
        if w >= a.warmup_windows:
            uniq.append(float(np.mean([int(torch.unique(values[i]).numel()) for i in range(P)])))
        order = names[w % 3:] + names[:w % 3]
        for n in order:
            emb, win = mods[n]
            slots = win.prepare([values[i] for i in range(P)])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(P):
                out = emb(slots[i], off, hook_features=F, presorted=win.keys[i])
                out.backward(grads[n])
            e1.record()
            e1.synchronize()
            assert out.dtype == DTYPES[n]
            if w >= a.warmup_windows:
                ms[n].append(e0.elapsed_time(e1) / P)
    # the value check: one more window, its first batch, one step per 16-bit dtype on sampled lookups
    values = gen.next_values(P)
    checks = {}
    ok = True
    for n in ("bf16", "fp16"):
        emb, win = mods[n]
        mgr = emb.cache_weight_mgr
        slots = win.prepare([values[i] for i in range(P)])
        s0 = slots[0].reshape(-1)
        valid = (s0 >= 0).nonzero().view(-1)                               # (strict=False: an overflowing id has slot -1)
        pick = valid[torch.randperm(valid.numel(), device=dev)[:a.check_rows]]
        before = mgr.cuda_cached_weight.detach()[s0[pick]].clone()
        out = emb(slots[0], off, hook_features=F, presorted=win.keys[0])
        f, b = pick // B, pick % B                                          # lookup j = f * B + b -> out[b, f]
        got = out.detach()[b, f]
        want = before.to(DTYPES[n])
        fwd_ok = bool(torch.equal(got.view(torch.int16), want.view(torch.int16)))
        out.backward(grads[n])
        # rows looked up once in the batch: ONE fp32 update with the upcast gradient, bit for bit
        cnt = torch.bincount(s0[valid], minlength=C)
        once = cnt[s0[pick]] == 1
        gup = grads[n].float()[b, f]
        after = mgr.cuda_cached_weight.detach()[s0[pick]]
        two = before + gup * (-a.lr)
        one = (before.double() + gup.double() * float(torch.tensor(-a.lr, dtype=torch.float32))).float()
        same = ((after == two) | (after == one)).all(dim=1)
        bwd_ok = bool(same[once].all()) and int(once.sum()) > 0
        checks[n] = {"lookups": int(pick.numel()), "rows_looked_up_once": int(once.sum()), "forward_bit_equal": fwd_ok,
                     "single_lookup_update_bit_equal": bwd_ok}
        ok = ok and fwd_ok and bwd_ok
    U = int(np.mean(uniq)) if uniq else 0
    res = {"bench": "bench_activation_dtype", "dataset": a.dataset, "table_scale": a.table_scale, "num_embeddings": N,
           "cuda_row_num": C, "batch_size": B, "features": F, "dim": D, "prefetch_num": P, "windows": a.windows,
           "unique_rows_per_batch": U,
           "scope": "per step: forward from the window's keys + fused SGD backward (cache op outside the timed range)"}
    for n in ms:
        t = float(np.median(ms[n]))
        res[f"{n}_ms_per_step"] = round(t, 4)
        res[f"{n}_ms_per_step_min_max"] = [round(float(min(ms[n])), 4), round(float(max(ms[n])), 4)]
        res[f"{n}_lookups_per_s"] = nnz / (t * 1e-3)
        res[f"{n}_algorithmic_bytes"] = algorithmic_bytes(nnz, D, 4 if n == "fp32" else 2, U)
    for n in ("bf16", "fp16"):
        res[f"{n}_over_fp32_step"] = round(res[f"{n}_ms_per_step"] / res["fp32_ms_per_step"], 3)
    res["check"] = {**checks, "ok": bool(ok)}
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
