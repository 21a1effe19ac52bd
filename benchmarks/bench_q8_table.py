"""The two bag forwards over an fp32, a bf16 and a q8 (8-bit row-wise quantized) table (one process, device events).

B = 16384, F = 26, D = 128: the general forward with one id per bag (nnz = 425,984) and with 20 ids per bag
(nnz = 8,519,680), and the key-driven forward over the window presort's source-row keys (one id per bag), each with an
fp32 and a bf16 output.  The table has --rows rows (1 Mi by default: 512 MiB of fp32 rows, beyond L2 and Infinity
Cache), the lookups are uniform over it, so nearly every lookup of the one-id shapes is a row of its own from HBM.

Method: every (kernel, shape, table, output) variant is warmed up, then timed --reps times (at least five) in an order
that rotates from repetition to repetition; one timing = --inner launches back to back between two device events.
Reported per variant: the median, min and max of the per-launch time, the bytes the algorithm needs (row bytes per
lookup -- per run of equal rows for the key-driven form -- plus the output) and that over the median as a fraction of
the 8.0 TB/s HBM peak.  `*_over_fp32`: the variant's median over the fp32 table's at the same kernel, shape and output,
beside the fp32 baseline's own (max - min) / median spread.  Prints ONE JSON line."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from cachedembedding_amd.functional import embedding_bag, presort_window, quantize_rows  # noqa: E402

HBM_PEAK = 8.0e12
OUTS = {"fp32": torch.float32, "bf16": torch.bfloat16}
ROW_BYTES = {"fp32": lambda D: 4 * D, "bf16": lambda D: 2 * D, "q8": lambda D: 16 + D}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batch_size", type=int, default=16384)
    p.add_argument("--features", type=int, default=26)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--rows", type=int, default=1 << 20)
    p.add_argument("--bag", type=int, default=20, help="ids per bag of the multi-id shape")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--seed", type=int, default=1024)
    a = p.parse_args(argv)
    if a.reps < 5:
        raise ValueError("--reps: at least five timed repetitions")
    if not torch.cuda.is_available():
        raise RuntimeError("bench_q8_table needs a HIP device (MI355X): there is no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, F, D, R = a.batch_size, a.features, a.dim, a.rows
    nb = B * F
    g = torch.Generator().manual_seed(a.seed)
    host = torch.randn(R, D, generator=g) * 0.01
    tables = {"fp32": host.to(dev), "bf16": host.to(torch.bfloat16).to(dev), "q8": quantize_rows(host).to(dev)}
    del host
    # shapes: (name, indices, offsets, number of lookups)
    idx1 = torch.randint(0, R, (nb,), generator=g).to(dev)
    off1 = torch.arange(nb + 1, dtype=torch.int32, device=dev)
    idxL = torch.randint(0, R, (nb * a.bag,), generator=g).to(dev)
    offL = torch.arange(0, nb * a.bag + 1, a.bag, dtype=torch.int32, device=dev)
    keys = presort_window(idx1.view(1, -1), R, offsets=off1, include_last_offset=True, hook_features=F,
                          identity_bags=True)[0]
    k = keys.keys.cpu().numpy().view(np.uint64)
    k = k[k != np.uint64(0xFFFFFFFFFFFFFFFF)] >> np.uint64(32)
    runs = int(1 + np.count_nonzero(k[1:] != k[:-1]))                 # row loads of the key-driven form (upper bound:
    shapes = {"fwd_1id": (idx1, off1, nb, None), "fwd_20id": (idxL, offL, nb * a.bag, None),      # shares cut runs)
              "fwd_keys_1id": (idx1, off1, runs, keys)}
    variants = [(s, t, o) for s in shapes for t in tables for o in OUTS]
    bufs = {o: torch.empty(B, F, D, device=dev, dtype=dt) for o, dt in OUTS.items()}

    def launch(s, t, o):
        idx, off, _, pre = shapes[s]
        embedding_bag(idx, tables[t], off, mode="sum", include_last_offset=True, hook_features=F, presorted=pre,
                      out=bufs[o], output_dtype=OUTS[o])

    with torch.no_grad():
        for v in variants:                                             # warm-up: code objects, first touch
            for _ in range(3):
                launch(*v)
        torch.cuda.synchronize()
        ms = {v: [] for v in variants}
        for r in range(a.reps):
            order = variants[r % len(variants):] + variants[:r % len(variants)]
            if r % 2:
                order = order[::-1]
            for v in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    launch(*v)
                e1.record()
                e1.synchronize()
                ms[v].append(e0.elapsed_time(e1) / a.inner)
        # the value check: every table's outputs at the one-id shape against a torch gather of sampled bags
        pick = torch.randint(0, nb, (4096,), generator=g).to(dev)
        f, b = pick // B, pick % B                                     # bag j = f * B + b -> out[b, f]
        from cachedembedding_amd.functional import dequantize_rows
        ok = True
        for t in tables:
            for s in ("fwd_1id", "fwd_keys_1id"):
                launch(s, t, "fp32")
                rows = tables[t][idx1[pick]]
                want = dequantize_rows(rows.cpu(), D).to(dev) if t == "q8" else rows.float()
                ok = ok and bool(torch.equal(bufs["fp32"][b, f], want))

    res = {"bench": "bench_q8_table", "batch_size": B, "features": F, "dim": D, "table_rows": R, "ids_per_bag": a.bag,
           "reps": a.reps, "launches_per_timing": a.inner, "hbm_peak_bytes_per_s": HBM_PEAK,
           "key_driven_row_loads": runs, "values_ok": ok,
           "scope": "one launch of the forward kernel through functional.embedding_bag(out=...), device events"}
    for s, t, o in variants:
        med = float(np.median(ms[(s, t, o)]))
        lo, hi = float(min(ms[(s, t, o)])), float(max(ms[(s, t, o)]))
        nbytes = shapes[s][2] * ROW_BYTES[t](D) + nb * D * (4 if o == "fp32" else 2)
        res[f"{s}_{t}_out_{o}"] = {"us": round(med * 1e3, 2), "us_min_max": [round(lo * 1e3, 2), round(hi * 1e3, 2)],
                                   "spread": round((hi - lo) / med, 3), "bytes": nbytes,
                                   "hbm_peak_fraction": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}
    for s in shapes:
        for o in OUTS:
            base = res[f"{s}_fp32_out_{o}"]["us"]
            for t in ("bf16", "q8"):
                res[f"{s}_{t}_out_{o}_over_fp32"] = round(res[f"{s}_{t}_out_{o}"]["us"] / base, 3)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
