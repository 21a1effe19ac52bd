"""Weight decay in the fused updates beside the same updates without it, in one process with device
events: does the decay cost anything?  It reads nothing the update does not read already -- the row is loaded before
the reduction instead of after it --, so the expectation is that the weight_decay != 0 lines sit within the run-to-run
spread of the weight_decay = 0 lines.

B = 16384, F = 26, D = 128, one id per bag (nnz = 425,984), lookups uniform over --rows rows (1 Mi by default).  The
whole backward + update from the source-row keys (what a window step runs): mark, (compaction, rewrite,) the dense
backward into the accumulator, the apply pass --
  * exact row-wise Adagrad with the cache-sized and with the step-sized accumulator, on an fp32 and on a bf16 table
    (rounded to nearest);
  * Adam on an Adam-layout table with the step-sized accumulator;
each with weight_decay = 0 (the entry from before the decay), CE_WD_L2 and CE_WD_DECOUPLED (the ce_*_wd entries).

Method, as in bench_adam.py: every variant is warmed up, then timed --reps times (at least five) in an order that
rotates from repetition to repetition; one timing = --inner calls back to back between two device events.  Reported per
variant: the median, min and max of the per-call time and the spread (max - min) / median; per update `*_over_none`:
the decayed median over the undecayed one, beside the undecayed variant's own spread.  Nothing here is a gate.  Prints
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

MODES = {"none": _lib.CE_WD_NONE, "l2": _lib.CE_WD_L2, "decoupled": _lib.CE_WD_DECOUPLED}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batch_size", type=int, default=16384)
    p.add_argument("--features", type=int, default=26)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--rows", type=int, default=1 << 20)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--weight_decay", type=float, default=1e-4)
    p.add_argument("--seed", type=int, default=1024)
    a = p.parse_args(argv)
    if a.reps < 5:
        raise ValueError("--reps: at least five timed repetitions")
    if not torch.cuda.is_available():
        raise RuntimeError("bench_weight_decay needs a HIP device (MI355X): there is no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, F, D, R = a.batch_size, a.features, a.dim, a.rows
    nb = B * F
    g = torch.Generator().manual_seed(a.seed)
    host = torch.randn(R, D, generator=g) * 0.01
    tables = {"fp32": host.to(dev), "bf16": host.to(torch.bfloat16).to(dev)}
    adam = torch.zeros(R, 3 * D, device=dev)
    adam[:, :D] = tables["fp32"]
    del host
    idx = torch.randint(0, R, (nb,), generator=g).to(dev)
    off = torch.arange(nb + 1, dtype=torch.int32, device=dev)
    keys = presort_window(idx.view(1, -1), R, offsets=off, include_last_offset=True, hook_features=F,
                          identity_bags=True)[0]
    unique = int(torch.unique(idx).numel())
    go = (torch.randn(B, F, D, generator=g) * 1e-3).to(dev)
    lr, eps, wd = 1e-4, 1e-8, float(a.weight_decay)
    mom = {t: torch.zeros(R, device=dev) for t in tables}
    step = torch.zeros(1, dtype=torch.int64, device=dev)
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
                check(lib.ce_bag_backward_update_src_wd(*head, lr, None, eps, wd, MODES[mode], ADAGRAD, NEAREST, 0, code,
                                                        ptr(ws), ws.numel(), stream_ptr()))
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

    def adam_step(mode):
        ws = zeros(lib.ce_bag_backward_adam_workspace(R, nb, D, _lib.CE_ACC_STEP))
        head = (ptr(adam), R, D, nb, ptr(go), F32, ptr(keys.keys), 0.9, 0.999, lr, None, eps)
        tail = (ptr(step), _lib.CE_ACC_STEP, ptr(ws), ws.numel(), stream_ptr())

        def run():
            if mode == "none":
                check(lib.ce_bag_backward_adam_src(*head, *tail))
            else:
                check(lib.ce_bag_backward_adam_src_wd(*head, wd, MODES[mode], *tail))
        return run

    groups = [f"adagrad_{t}_{acc}" for t in ("fp32", "bf16") for acc in ("cache", "step")] + ["adam_step"]
    variants = {}
    for t in ("fp32", "bf16"):
        for acc in ("cache", "step"):
            for mode in MODES:
                variants[f"adagrad_{t}_{acc}_{mode}"] = adagrad(t, acc, mode)
    for mode in MODES:
        variants[f"adam_step_{mode}"] = adam_step(mode)
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
        ok = int(step.item()) == 3 * (3 + a.reps * a.inner) and bool(torch.isfinite(adam).all()) and \
            all(bool(torch.isfinite(t.float()).all()) for t in tables.values())

    res = {"bench": "bench_weight_decay", "batch_size": B, "features": F, "dim": D, "table_rows": R, "reps": a.reps,
           "launches_per_timing": a.inner, "unique_rows": unique, "weight_decay": wd, "values_ok": ok,
           "scope": "one call of the C entry from source-row keys (mark, compaction, dense backward, apply); device events"}
    for n in names:
        med = float(np.median(ms[n]))
        lo, hi = float(min(ms[n])), float(max(ms[n]))
        res[n] = {"us": round(med * 1e3, 2), "us_min_max": [round(lo * 1e3, 2), round(hi * 1e3, 2)],
                  "spread": round((hi - lo) / med, 3)}
    for grp in groups:
        base = res[f"{grp}_none"]
        for mode in ("l2", "decoupled"):
            res[f"{grp}_{mode}_over_none"] = round(res[f"{grp}_{mode}"]["us"] / base["us"], 3)
        res[f"{grp}_none_spread"] = base["spread"]
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
