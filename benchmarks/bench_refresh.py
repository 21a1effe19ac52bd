"""Refreshing rows of a served (quantized) table in place, against what there was before (one process).

(a) The device quantizer: ce_quantize_rows_q8 / _q4 on --rows rows (1 Mi) of D = 128, fp32 and bf16 source, held
    against ce_host_quantize_* on the SAME rows at ce_cpu_budget() threads and against the bytes-moved bound: per row
    4 D (2 D) bytes read and 16 + D (16 + D / 2) written, at 6.3 TB/s -- the HBM rate a streaming copy achieves on this
    part (8.0 TB/s is the specification's peak; both fractions are printed).  One device timing = --inner launches back
    to back between two device events; the variants alternate from repetition to repetition.
(b) refresh_rows of 64 Ki and of 1 Mi distinct rows into a --table_rows (4 Mi) q8 table behind a 10 % cache, held
    against quantized() of the same trainer -- the only way to bring a served copy up to date without refresh_rows --,
    host clock around work that ends in a device synchronise.  And what the served cache is worth afterwards: the
    misses of the next 20 batches (8192 x 26 ids each, long-tailed: --skew) on the refreshed module (warm) and on the
    rebuilt one (cold).

Every figure is the median of --reps repetitions (at least five) with its min and max.  Prints ONE JSON line."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import cachedembedding_amd as ce  # noqa: E402
from cachedembedding_amd import _lib  # noqa: E402

HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])


def quantizer_speed(a, dev):
    R, D = a.rows, a.dim
    g = torch.Generator().manual_seed(a.seed)
    host32 = torch.randn(R, D, generator=g) * 0.01
    srcs = {"fp32": host32, "bf16": host32.to(torch.bfloat16)}
    variants = [(bits, s) for bits in (8, 4) for s in srcs]
    dsrc = {s: t.to(dev) for s, t in srcs.items()}
    width = {8: 16 + D, 4: 16 + D // 2}
    outs = {bits: torch.empty(R, width[bits], dtype=torch.uint8, device=dev) for bits in (8, 4)}
    first_bad = torch.empty(1, dtype=torch.int64, device=dev)
    entry = {8: _lib.lib.ce_quantize_rows_q8, 4: _lib.lib.ce_quantize_rows_q4}
    host_entry = {8: _lib.lib.ce_host_quantize_q8, 4: _lib.lib.ce_host_quantize_q4}
    threads = int(_lib.lib.ce_cpu_budget())

    def launch(bits, s):
        t = dsrc[s]
        _lib.check(entry[bits](_lib.ptr(t), _lib.ACT_DTYPES[t.dtype], R, D, _lib.ptr(outs[bits]), _lib.ptr(first_bad),
                               _lib.stream_ptr()))

    dev_ms = {v: [] for v in variants}
    host_ms = {v: [] for v in variants}
    hout = {bits: torch.empty(R, width[bits], dtype=torch.uint8) for bits in (8, 4)}
    for v in variants:                                       # warm-up, and the results agree before anything is timed
        launch(*v)
        _lib.check(host_entry[v[0]](_lib.ptr(srcs[v[1]]), _lib.ACT_DTYPES[srcs[v[1]].dtype], R, D, _lib.ptr(hout[v[0]]),
                                    threads))
        torch.cuda.synchronize()
        if not torch.equal(outs[v[0]].cpu(), hout[v[0]]):
            raise RuntimeError(f"device and host quantizer disagree on {v}")
    for rep in range(a.reps):
        order = variants[rep % len(variants):] + variants[:rep % len(variants)]
        for v in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                launch(*v)
            e1.record()
            e1.synchronize()
            dev_ms[v].append(e0.elapsed_time(e1) / a.inner)
            t0 = time.perf_counter()
            _lib.check(host_entry[v[0]](_lib.ptr(srcs[v[1]]), _lib.ACT_DTYPES[srcs[v[1]].dtype], R, D,
                                        _lib.ptr(hout[v[0]]), threads))
            host_ms[v].append((time.perf_counter() - t0) * 1e3)
    res = {}
    for bits, s in variants:
        nbytes = R * ((4 if s == "fp32" else 2) * D + width[bits])
        d, h = stats(dev_ms[(bits, s)]), stats(host_ms[(bits, s)])
        res[f"q{bits}_{s}"] = dict(device_ms=d, host_ms=h, host_threads=threads, bytes=nbytes,
                                   bound_ms=nbytes / HBM_ACHIEVABLE * 1e3,
                                   fraction_of_achievable_hbm=nbytes / HBM_ACHIEVABLE * 1e3 / d["median"],
                                   fraction_of_hbm_peak=nbytes / HBM_PEAK * 1e3 / d["median"],
                                   host_over_device=h["median"] / d["median"])
    return res


def refresh_against_rebuild(a, dev):
    N, D = a.table_rows, a.dim
    C = N // 10
    trainer = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, init_seed=a.seed)
    t0 = time.perf_counter()
    served = trainer.quantized()
    torch.cuda.synchronize()
    rebuild_s = [time.perf_counter() - t0]
    g = torch.Generator().manual_seed(a.seed + 1)
    B = 8192 * 26
    # --skew 1: uniform ids (a 10 % cache then holds 10 % of the lookups, warm or cold); --skew k > 1: id = N u^k for
    # uniform u, a long tail with the low ids hot, as recommendation ids are (k = 4: 56 % of the lookups in 10 % of the rows)
    batches = [(N * torch.rand(B, generator=g, dtype=torch.float64) ** a.skew).long().clamp_(max=N - 1).to(dev)
               for _ in range(20)]
    off = torch.arange(B + 1, dtype=torch.int32, device=dev)

    def misses(module):
        before = sum(module.num_miss_history)
        for ids in batches:
            module(ids, off)
        torch.cuda.synchronize()
        return sum(module.num_miss_history) - before

    misses(served)                                           # the served cache warms up on the stream it will see again
    out = {"table_rows": N, "cache_rows": C, "skew": a.skew, "rebuild_quantized_s": None}
    for n in a.refresh_rows:
        ids = torch.randperm(N, generator=g)[:n].to(dev)
        rows = (torch.randn(n, D, generator=g) * 0.01).to(dev)
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            served.refresh_rows(ids, rows)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        out[f"refresh_rows_{n}_s"] = stats(times)
    out["misses_next_20_batches_refreshed"] = misses(served)
    for _ in range(a.reps - 1):
        del served
        t0 = time.perf_counter()
        served = trainer.quantized()
        torch.cuda.synchronize()
        rebuild_s.append(time.perf_counter() - t0)
    out["rebuild_quantized_s"] = stats(rebuild_s)
    out["misses_next_20_batches_rebuilt"] = misses(served)
    out["lookups_next_20_batches"] = 20 * B
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1 << 20)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--table_rows", type=int, default=1 << 22)
    p.add_argument("--refresh_rows", type=int, nargs="+", default=[1 << 16, 1 << 20])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--seed", type=int, default=1024)
    p.add_argument("--skew", type=float, default=4.0, help="ids of part (b): N * u ** skew (1: uniform)")
    p.add_argument("--only", choices=["quantizer", "refresh"], default=None)
    a = p.parse_args(argv)
    if a.reps < 5:
        raise ValueError("--reps: at least five timed repetitions")
    if not torch.cuda.is_available():
        raise RuntimeError("bench_refresh needs a HIP device (MI355X): there is no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"bench": "refresh", "dim": a.dim, "rows": a.rows, "reps": a.reps, "inner": a.inner}
    if a.only != "refresh":
        res["quantizer"] = quantizer_speed(a, dev)
    if a.only != "quantizer":
        res["refresh"] = refresh_against_rebuild(a, dev)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
