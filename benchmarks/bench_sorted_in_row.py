"""The sorted (deterministic) fold of the in-row fused optimizers beside the atomic fold with the
step-sized accumulator, in one process with device events: what does run-to-run equality cost per call, per layout --
Adam (rows w | m | v), partial row-wise Adam (rows w | m, v per row), element-wise Adagrad (rows w | h) -- and what does
each path's workspace weigh?

B = 16384, F = 26, D = 128, one id per bag (nnz = 425,984), from slots + offsets (the only form the sorted entries have),
over --rows rows (1 Mi by default), for two id distributions: `uniform` (nearly every lookup a row of its own) and `zipf`
(exponent 1.2: hot rows, runs of many chunks).  The whole call is timed: the atomic one's mark, compaction, rewrite, dense
backward and apply pass; the sorted one's step count, sort, fold and apply pass.

Method, as in bench_partial_rowwise_adam.py: every variant is warmed up, then timed --reps times (at least five) in an
order that rotates from repetition to repetition; one timing = --inner calls back to back between two device events.
Reported per variant: the median, min and max of the per-call time, the spread (max - min) / median and the workspace's
bytes; `*_sorted_over_step`: ratios of medians.  Nothing here is a gate.  Prints ONE JSON line."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from cachedembedding_amd import _lib  # noqa: E402
from cachedembedding_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402

SPAN = {"adam": 3, "partial": 2, "adagrad": 2}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batch_size", type=int, default=16384)
    p.add_argument("--features", type=int, default=26)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--rows", type=int, default=1 << 20)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--seed", type=int, default=1024)
    a = p.parse_args(argv)
    if a.reps < 5:
        raise ValueError("--reps: at least five timed repetitions")
    if not torch.cuda.is_available():
        raise RuntimeError("bench_sorted_in_row needs a HIP device (MI355X): there is no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, F, D, R = a.batch_size, a.features, a.dim, a.rows
    nb = B * F
    g = torch.Generator().manual_seed(a.seed)
    rng = np.random.default_rng(a.seed)
    w0 = torch.randn(R, D, generator=g) * 0.01
    tables = {}
    for layout, span in SPAN.items():
        t = torch.zeros(R, span * D)
        t[:, :D] = w0
        tables[layout] = t.to(dev)
    del w0
    ids = {"uniform": torch.randint(0, R, (nb,), generator=g).to(dev),
           "zipf": torch.from_numpy(np.minimum(rng.zipf(1.2, nb) - 1, R - 1).astype(np.int64)).to(dev)}
    stats = {}
    for dist, idx in ids.items():
        counts = torch.bincount(idx, minlength=1)
        stats[dist] = {"unique_rows": int((counts > 0).sum().item()), "longest_run": int(counts.max().item())}
    off = torch.arange(nb + 1, dtype=torch.int32, device=dev)
    go = (torch.randn(B, F, D, generator=g) * 1e-3).to(dev)
    lr, eps = 1e-4, 1e-8
    v_rows = torch.zeros(R, device=dev)
    steps = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in SPAN}
    ws_bytes = {"step": lib.ce_bag_backward_adam_workspace(R, nb, D, _lib.CE_ACC_STEP),
                "sorted": lib.ce_bag_backward_in_row_sorted_workspace(R, nb, D)}
    ws = {"step": torch.zeros(ws_bytes["step"], dtype=torch.uint8, device=dev),
          "sorted": torch.empty(ws_bytes["sorted"], dtype=torch.uint8, device=dev)}

    def upd(layout, path, dist):
        idx, w, t = ids[dist], ws[path], tables[layout]
        head = (ptr(t), R, D, ptr(idx), nb, ptr(off), 0, nb, 1, None, _lib.CE_MODE_SUM, F, ptr(go), _lib.CE_ACT_F32)
        keys = (None,) if path == "step" else ()
        acc = (_lib.CE_ACC_STEP,) if path == "step" else ()
        tail = (lr, None, eps, 0.0, _lib.CE_WD_NONE, 0.0, _lib.CE_CLIP_NONE, ptr(steps[layout])) + acc + \
            (ptr(w), w.numel(), stream_ptr())
        if layout == "adam":
            fn = lib.ce_bag_backward_adam_clip if path == "step" else lib.ce_bag_backward_adam_sorted
            args = head + keys + (0.9, 0.999) + tail
        elif layout == "partial":
            fn = lib.ce_bag_backward_pradam_clip if path == "step" else lib.ce_bag_backward_pradam_sorted
            args = head + keys + (None, ptr(v_rows), R, 0.9, 0.999) + tail
        else:
            fn = lib.ce_bag_backward_adagrad if path == "step" else lib.ce_bag_backward_adagrad_sorted
            args = head + keys + (0.0,) + tail

        def run():
            check(fn(*args))
        return run

    variants = {f"{layout}_{path}_{dist}": upd(layout, path, dist)
                for dist in ids for layout in SPAN for path in ("step", "sorted")}
    names = list(variants)
    for n in names:                                                    # warm-up: code objects, first touch
        for _ in range(3):
            variants[n]()
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    for r in range(a.reps):
        order = names[r % len(names):] + names[:r % len(names)]
        if r % 2:
            order = order[::-1]
        for n in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                variants[n]()
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1) / a.inner)
    calls = 2 * len(ids) * (3 + a.reps * a.inner)
    ok = all(int(s.item()) == calls for s in steps.values())
    ok = ok and all(bool(torch.isfinite(t).all()) for t in tables.values()) and bool(torch.isfinite(v_rows).all())

    res = {"bench": "bench_sorted_in_row", "batch_size": B, "features": F, "dim": D, "table_rows": R, "nnz": nb,
           "reps": a.reps, "launches_per_timing": a.inner, "values_ok": ok, "lookups": stats,
           "workspace_bytes": ws_bytes,
           "scope": "one call of the C entry from slots + offsets (atomic: mark, compaction, rewrite, dense backward, "
                    "apply; sorted: step count, sort, fold, apply); device events"}
    for n in names:
        med = float(np.median(ms[n]))
        lo, hi = float(min(ms[n])), float(max(ms[n]))
        res[n] = {"us": round(med * 1e3, 2), "us_min_max": [round(lo * 1e3, 2), round(hi * 1e3, 2)],
                  "spread": round((hi - lo) / med, 3)}
    for dist in ids:
        for layout in SPAN:
            res[f"{layout}_{dist}_sorted_over_step"] = round(res[f"{layout}_sorted_{dist}"]["us"] /
                                                             res[f"{layout}_step_{dist}"]["us"], 3)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
