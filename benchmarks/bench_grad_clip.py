"""Gradient clipping in the fused updates beside the same updates without it, in one process with device
events: what does the clip cost?  "value" is a clamp per element of a gradient the apply pass holds in registers anyway;
"row_norm" adds a second reduction across the row's lane group (sum of squares, square root, one division) in front of
the one row-wise Adagrad / partial row-wise Adam already run.  Both act between the accumulator's load and the row's
store, on a pass that is bound by memory, so the expectation is that the clipped lines sit within the run-to-run spread
of the unclipped ones.

B = 16384, F = 26, D = 128, one id per bag (nnz = 425,984), lookups uniform over --rows rows (1 Mi by default).  The
whole backward + update from the source-row keys (what a window step runs): mark, (compaction, rewrite,) the dense
backward into the accumulator, the apply pass --
  * exact row-wise Adagrad with the cache-sized and with the step-sized accumulator, on an fp32 and on a bf16 table
    (rounded to nearest);
  * Adam on an Adam-layout table and partial row-wise Adam on its layout, with the step-sized accumulator;
each unclipped (the entry from before the clip), with CE_CLIP_VALUE and with CE_CLIP_ROW_NORM (the ce_*_clip entries; no
decay).  The thresholds sit in the middle of the gradients' distribution (--clip_sigma gradient standard deviations per
element), so both branches of either clip are taken.

Method, as in bench_weight_decay.py: every variant is warmed up, then timed --reps times (at least five) in an order
that rotates from repetition to repetition; one timing = --inner calls back to back between two device events.  Reported
per variant: the median, min and max of the per-call time and the spread (max - min) / median; per update `*_over_none`:
the clipped median over the unclipped one, beside the unclipped variant's own spread.  Nothing here is a gate.  Prints
ONE JSON line."""
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
from cachedembedding_amd.functional import presort_window  # noqa: E402

MODES = {"none": _lib.CE_CLIP_NONE, "value": _lib.CE_CLIP_VALUE, "row_norm": _lib.CE_CLIP_ROW_NORM}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batch_size", type=int, default=16384)
    p.add_argument("--features", type=int, default=26)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--rows", type=int, default=1 << 20)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--clip_sigma", type=float, default=1.0)
    p.add_argument("--seed", type=int, default=1024)
    a = p.parse_args(argv)
    if a.reps < 5:
        raise ValueError("--reps: at least five timed repetitions")
    if not torch.cuda.is_available():
        raise RuntimeError("bench_grad_clip needs a HIP device (MI355X): there is no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, F, D, R = a.batch_size, a.features, a.dim, a.rows
    nb = B * F
    g = torch.Generator().manual_seed(a.seed)
    host = torch.randn(R, D, generator=g) * 0.01
    tables = {"fp32": host.to(dev), "bf16": host.to(torch.bfloat16).to(dev)}
    adam = torch.zeros(R, 3 * D, device=dev)
    adam[:, :D] = tables["fp32"]
    pradam = torch.zeros(R, 2 * D, device=dev)
    pradam[:, :D] = tables["fp32"]
    del host
    idx = torch.randint(0, R, (nb,), generator=g).to(dev)
    off = torch.arange(nb + 1, dtype=torch.int32, device=dev)
    keys = presort_window(idx.view(1, -1), R, offsets=off, include_last_offset=True, hook_features=F,
                          identity_bags=True)[0]
    unique = int(torch.unique(idx).numel())
    sigma = 1e-3
    go = (torch.randn(B, F, D, generator=g) * sigma).to(dev)
    lr, eps = 1e-4, 1e-8
    clip = {"none": 0.0, "value": a.clip_sigma * sigma, "row_norm": a.clip_sigma * sigma * float(np.sqrt(D))}
    mom = {t: torch.zeros(R, device=dev) for t in tables}
    v_row = torch.zeros(R, device=dev)
    steps = {"adam": torch.zeros(1, dtype=torch.int64, device=dev), "pradam": torch.zeros(1, dtype=torch.int64, device=dev)}
    F32, NEAREST, ADAGRAD = _lib.CE_ACT_F32, _lib.CE_ROUND_NEAREST, _lib.CE_OPT_ROWWISE_ADAGRAD

    def zeros(n):
        return torch.zeros(n, dtype=torch.uint8, device=dev)

    def adagrad(table, acc, mode):
        w = tables[table]
        wdt = _lib.ACT_DTYPES[w.dtype]
        code = _lib.CE_ACC_STEP if acc == "step" else _lib.CE_ACC_CACHE
        if acc == "step":
            ws = zeros(lib.ce_bag_backward_update_compact_workspace(R, nb, D))
        elif table == "fp32":
            ws = zeros(lib.ce_bag_backward_rowwise_adagrad_workspace(R, D))
        else:
            ws = zeros(lib.ce_bag_backward_w16_workspace(R, D))
        head = (ptr(w), wdt, R, D, nb, ptr(go), F32, ptr(keys.keys), None, ptr(mom[table]), R)

        def run():
            if mode != "none":
                check(lib.ce_bag_backward_update_src_clip(*head, lr, None, eps, 0.0, _lib.CE_WD_NONE, clip[mode],
                                                          MODES[mode], ADAGRAD, NEAREST, 0, code, ptr(ws), ws.numel(),
                                                          stream_ptr()))
            elif acc == "step":
                check(lib.ce_bag_backward_update_compact_src(*head, lr, eps, ADAGRAD, NEAREST, 0, ptr(ws), ws.numel(),
                                                             stream_ptr()))
            elif table == "fp32":
                check(lib.ce_bag_backward_rowwise_adagrad_src_act(ptr(w), R, D, nb, ptr(go), F32, ptr(keys.keys), None,
                                                                  ptr(mom[table]), R, lr, eps, ptr(ws), ws.numel(),
                                                                  stream_ptr()))
            else:
                check(lib.ce_bag_backward_update_src_w16(*head, lr, eps, ADAGRAD, NEAREST, 0, ptr(ws), ws.numel(),
                                                         stream_ptr()))
        return run

    def adam_step(which, mode):
        ws = zeros(lib.ce_bag_backward_adam_workspace(R, nb, D, _lib.CE_ACC_STEP))
        table = adam if which == "adam" else pradam
        head = (ptr(table), R, D, nb, ptr(go), F32, ptr(keys.keys))
        if which == "pradam":
            head += (None, ptr(v_row), R)
        head += (0.9, 0.999, lr, None, eps)
        tail = (ptr(steps[which]), _lib.CE_ACC_STEP, ptr(ws), ws.numel(), stream_ptr())

        def run():
            if mode != "none":
                fn = lib.ce_bag_backward_adam_src_clip if which == "adam" else lib.ce_bag_backward_pradam_src_clip
                check(fn(*head, 0.0, _lib.CE_WD_NONE, clip[mode], MODES[mode], *tail))
            elif which == "adam":
                check(lib.ce_bag_backward_adam_src(*head, *tail))
            else:
                check(lib.ce_bag_backward_pradam_src(*head, 0.0, _lib.CE_WD_NONE, *tail))
        return run

    groups = [f"adagrad_{t}_{acc}" for t in ("fp32", "bf16") for acc in ("cache", "step")] + ["adam_step", "pradam_step"]
    variants = {}
    for t in ("fp32", "bf16"):
        for acc in ("cache", "step"):
            for mode in MODES:
                variants[f"adagrad_{t}_{acc}_{mode}"] = adagrad(t, acc, mode)
    for which in ("adam", "pradam"):
        for mode in MODES:
            variants[f"{which}_step_{mode}"] = adam_step(which, mode)
    names = list(variants)
    with torch.no_grad():
        for n in names:                                                # warm-up: code objects, first touch
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
        calls = 3 * (3 + a.reps * a.inner)
        ok = all(int(s.item()) == calls for s in steps.values()) and bool(torch.isfinite(adam).all()) and \
            bool(torch.isfinite(pradam).all()) and all(bool(torch.isfinite(t.float()).all()) for t in tables.values())

    res = {"bench": "bench_grad_clip", "batch_size": B, "features": F, "dim": D, "table_rows": R, "reps": a.reps,
           "launches_per_timing": a.inner, "unique_rows": unique, "grad_clip": {k: v for k, v in clip.items() if v},
           "values_ok": ok,
           "scope": "one call of the C entry from source-row keys (mark, compaction, dense backward, apply); device events"}
    for n in names:
        med = float(np.median(ms[n]))
        lo, hi = float(min(ms[n])), float(max(ms[n]))
        res[n] = {"us": round(med * 1e3, 2), "us_min_max": [round(lo * 1e3, 2), round(hi * 1e3, 2)],
                  "spread": round((hi - lo) / med, 3)}
    for grp in groups:
        base = res[f"{grp}_none"]
        for mode in ("value", "row_norm"):
            res[f"{grp}_{mode}_over_none"] = round(res[f"{grp}_{mode}"]["us"] / base["us"], 3)
        res[f"{grp}_none_spread"] = base["spread"]
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
