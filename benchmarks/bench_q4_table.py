"""The two bag forwards over an fp32, a q8 and a q4 (8-bit / 4-bit row-wise quantized) table (one process, device
events): is the q4 forward slower than the q8 forward of the same process by more than q8's own spread?

B = 16384, F = 26, D = 128: the general forward with one id per bag (nnz = 425,984) and with 20 ids per bag
(nnz = 8,519,680), and the key-driven forward over the window presort's source-row keys (one id per bag), each with an
fp32 and a bf16 output.  The table has --rows rows (1 Mi by default: 512 MiB of fp32 rows, 144 MiB of q8 rows, 80 MiB
of q4 rows), the lookups are uniform over it.

Method, as in bench_q8_table.py: every (kernel, shape, table, output) variant is warmed up, then timed --reps times (at
least five) in an order that rotates from repetition to repetition, so the three tables alternate inside every
repetition; one timing = --inner launches back to back between two device events.  Reported per variant: the median,
min and max of the per-launch time, the bytes the algorithm needs and that over the median as a fraction of the 8.0 TB/s
HBM peak, and the 128-byte lines its row loads touch (a q8 row of D = 128 spans 2, a q4 row 1 or 2 by its offset, an
fp32 row 4).  `*_q4_over_q8`: the q4 median over the q8 median of the same kernel, shape and output, beside
`*_q8_spread`, the q8 variant's own (max - min) / median over its repetitions; `q4_not_slower_than_q8` is true when no
q4 median exceeds its q8 median by more than that spread.  Prints ONE JSON line."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from cachedembedding_amd.functional import dequantize_rows, embedding_bag, presort_window, quantize_rows  # noqa: E402

HBM_PEAK = 8.0e12
OUTS = {"fp32": torch.float32, "bf16": torch.bfloat16}
ROW_BYTES = {"fp32": lambda D: 4 * D, "q8": lambda D: 16 + D, "q4": lambda D: 16 + D // 2}
BITS = {"fp32": 8, "q8": 8, "q4": 4}                 # quant_bits is looked at for a uint8 table only


def lines_per_row(row_bytes: int) -> float:
    """128-byte lines a row of row_bytes spans, averaged over the offsets in a line that rows lying back to back from an
    aligned base start at (a 512-byte row: always 0; a 144- or 80-byte row: all 8 multiples of 16)"""
    return float(np.mean([((k * row_bytes) % 128 + row_bytes - 1) // 128 + 1 for k in range(8)]))


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
        raise RuntimeError("bench_q4_table needs a HIP device (MI355X): there is no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, F, D, R = a.batch_size, a.features, a.dim, a.rows
    nb = B * F
    g = torch.Generator().manual_seed(a.seed)
    host = torch.randn(R, D, generator=g) * 0.01
    tables = {"fp32": host.to(dev), "q8": quantize_rows(host).to(dev), "q4": quantize_rows(host, bits=4).to(dev)}
    del host
    # shapes: (name, indices, offsets, number of row loads)
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
                      out=bufs[o], output_dtype=OUTS[o], quant_bits=BITS[t])

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
        ok = True
        for t in tables:
            for s in ("fwd_1id", "fwd_keys_1id"):
                launch(s, t, "fp32")
                rows = tables[t][idx1[pick]]
                want = rows.float() if t == "fp32" else dequantize_rows(rows.cpu(), D, bits=BITS[t]).to(dev)
                ok = ok and bool(torch.equal(bufs["fp32"][b, f], want))

    res = {"bench": "bench_q4_table", "batch_size": B, "features": F, "dim": D, "table_rows": R, "ids_per_bag": a.bag,
           "reps": a.reps, "launches_per_timing": a.inner, "hbm_peak_bytes_per_s": HBM_PEAK,
           "key_driven_row_loads": runs, "values_ok": ok,
           "lines_per_row": {t: lines_per_row(ROW_BYTES[t](D)) for t in tables},
           "scope": "one launch of the forward kernel through functional.embedding_bag(out=...), device events"}
    for s, t, o in variants:
        med = float(np.median(ms[(s, t, o)]))
        lo, hi = float(min(ms[(s, t, o)])), float(max(ms[(s, t, o)]))
        out_bytes = nb * D * (4 if o == "fp32" else 2)
        nbytes = shapes[s][2] * ROW_BYTES[t](D) + out_bytes
        res[f"{s}_{t}_out_{o}"] = {"us": round(med * 1e3, 2), "us_min_max": [round(lo * 1e3, 2), round(hi * 1e3, 2)],
                                   "spread": round((hi - lo) / med, 3), "bytes": nbytes,
                                   "hbm_peak_fraction": round(nbytes / (med * 1e-3) / HBM_PEAK, 3),
                                   "row_lines": int(shapes[s][2] * lines_per_row(ROW_BYTES[t](D))),
                                   "output_lines": out_bytes // 128}
    not_slower = True
    for s in shapes:
        for o in OUTS:
            base, q8, q4 = (res[f"{s}_{t}_out_{o}"] for t in ("fp32", "q8", "q4"))
            res[f"{s}_q8_out_{o}_over_fp32"] = round(q8["us"] / base["us"], 3)
            res[f"{s}_q4_out_{o}_over_fp32"] = round(q4["us"] / base["us"], 3)
            res[f"{s}_out_{o}_q4_over_q8"] = round(q4["us"] / q8["us"], 3)
            res[f"{s}_out_{o}_q8_spread"] = q8["spread"]
            not_slower = not_slower and q4["us"] <= q8["us"] * (1 + q8["spread"])
    res["q4_not_slower_than_q8"] = not_slower
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
