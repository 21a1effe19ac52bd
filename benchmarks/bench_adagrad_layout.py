"""Element-wise Adagrad with its state in the row (rows w | h of 2 * D fp32) beside row-wise Adagrad on
the plain fp32 table, partial row-wise Adam (rows w | m, the same row width) and the Adam layout (rows w | m | v), in one
process with device events: where does the new update land -- by the bytes a row moves it should lie near partial
row-wise Adam and clearly under Adam -- and does its forward cost what the partial layout's does (it runs those kernels)?

B = 16384, F = 26, D = 128, one id per bag (nnz = 425,984), lookups uniform over --rows rows (1 Mi by default: 512 MiB
of fp32 rows, 1 GiB each of Adagrad-layout and partial rows, 1.5 GiB of Adam-layout rows): bench_partial_rowwise_adam's
shape.
  * the key-driven forward (the window presort's source-row keys), fp32 output, over the four tables.
  * backward + update, from the source-row keys (what a window step runs), each with the cache-sized and with the
    step-sized accumulator -- the whole call: mark, (compaction, rewrite,) the dense backward into the accumulator, the
    apply pass.  `apply_bytes`: what the apply pass alone moves per call, U unique rows times 4 * D bytes times 4
    (row-wise Adagrad: acc, w read and written), 6 (element-wise Adagrad: acc, w, h; partial: acc, w, m) or 8 (Adam: acc,
    w, m, v) row-parts, the 4 bytes per row of row-wise Adagrad's momentum and of the partial layout's second moment
    apart.

Method, as in bench_adam.py: every variant is warmed up, then timed --reps times (at least five) in an order that
rotates from repetition to repetition; one timing = --inner calls back to back between two device events.  Reported per
variant: the median, min and max of the per-call time and the spread (max - min) / median.  `*_elementwise_over_*`:
ratios of medians.  Nothing here is a gate.  Prints ONE JSON line."""
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
from cachedembedding_amd.functional import FusedAdagrad, FusedAdam, embedding_bag, presort_window  # noqa: E402

HBM_PEAK = 8.0e12
PARTS = {"adagrad": 4, "elementwise": 6, "partial": 6, "adam": 8}                     # row-parts the apply pass moves per distinct row


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
        raise RuntimeError("bench_adagrad_layout needs a HIP device (MI355X): there is no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, F, D, R = a.batch_size, a.features, a.dim, a.rows
    nb = B * F
    g = torch.Generator().manual_seed(a.seed)
    host = torch.randn(R, D, generator=g) * 0.01
    tables = {"fp32": host.to(dev), "elementwise": torch.zeros(R, 2 * D, device=dev),
              "partial": torch.zeros(R, 2 * D, device=dev), "adam": torch.zeros(R, 3 * D, device=dev)}
    for t in ("elementwise", "partial", "adam"):
        tables[t][:, :D] = tables["fp32"]
    del host
    idx = torch.randint(0, R, (nb,), generator=g).to(dev)
    off = torch.arange(nb + 1, dtype=torch.int32, device=dev)
    keys = presort_window(idx.view(1, -1), R, offsets=off, include_last_offset=True, hook_features=F,
                          identity_bags=True)[0]
    unique = int(torch.unique(idx).numel())
    k = keys.keys.cpu().numpy().view(np.uint64)
    k = k[k != np.uint64(0xFFFFFFFFFFFFFFFF)] >> np.uint64(32)
    runs = int(1 + np.count_nonzero(k[1:] != k[:-1]))
    out = torch.empty(B, F, D, device=dev)
    go = (torch.randn(B, F, D, generator=g) * 1e-3).to(dev)
    # the objects that say which layout a weight has
    tags = {"fp32": None, "elementwise": FusedAdagrad(None), "adam": FusedAdam(None),
            "partial": FusedAdam(None, layout="partial_rowwise_adam")}

    def fwd(table, pre):
        def run():
            embedding_bag(idx, tables[table], off, mode="sum", include_last_offset=True, hook_features=F, presorted=pre,
                          out=out, fused_sgd=tags[table])
        return run

    # the updates, through the C entries (no autograd node between the launches)
    lr, eps = 1e-4, 1e-8                                               # (element-wise Adagrad: torch's 1e-10)
    mom = torch.zeros(R, device=dev)
    v_rows = torch.zeros(R, device=dev)
    steps = {o: torch.zeros(1, dtype=torch.int64, device=dev) for o in ("elementwise", "partial", "adam")}
    codes = {"cache": _lib.CE_ACC_CACHE, "step": _lib.CE_ACC_STEP}
    ws = {("adagrad", "cache"): lib.ce_bag_backward_rowwise_adagrad_workspace(R, D),
          ("adagrad", "step"): lib.ce_bag_backward_update_compact_workspace(R, nb, D)}
    for acc, code in codes.items():
        ws[("adam", acc)] = lib.ce_bag_backward_adam_workspace(R, nb, D, code)
        ws[("partial", acc)] = lib.ce_bag_backward_pradam_workspace(R, nb, D, code)
        ws[("elementwise", acc)] = lib.ce_bag_backward_adagrad_workspace(R, nb, D, code)
    ws = {kk: torch.zeros(n, dtype=torch.uint8, device=dev) for kk, n in ws.items()}

    def upd(opt, acc):
        w = ws[(opt, acc)]
        plain = tables["fp32"]

        def run():
            if opt == "adam":
                check(lib.ce_bag_backward_adam_src(ptr(tables["adam"]), R, D, nb, ptr(go), _lib.CE_ACT_F32, ptr(keys.keys),
                                                   0.9, 0.999, lr, None, eps, ptr(steps["adam"]), codes[acc], ptr(w),
                                                   w.numel(), stream_ptr()))
            elif opt == "elementwise":
                check(lib.ce_bag_backward_adagrad_src(ptr(tables["elementwise"]), R, D, nb, ptr(go), _lib.CE_ACT_F32,
                                                      ptr(keys.keys), 0.0, lr, None, 1e-10, 0.0, 0, 0.0, 0,
                                                      ptr(steps["elementwise"]), codes[acc], ptr(w), w.numel(),
                                                      stream_ptr()))
            elif opt == "partial":
                check(lib.ce_bag_backward_pradam_src(ptr(tables["partial"]), R, D, nb, ptr(go), _lib.CE_ACT_F32,
                                                     ptr(keys.keys), None, ptr(v_rows), R, 0.9, 0.999, lr, None, eps, 0.0,
                                                     0, ptr(steps["partial"]), codes[acc], ptr(w), w.numel(),
                                                     stream_ptr()))
            elif acc == "cache":
                check(lib.ce_bag_backward_rowwise_adagrad_src_act(ptr(plain), R, D, nb, ptr(go), _lib.CE_ACT_F32,
                                                                  ptr(keys.keys), None, ptr(mom), R, lr, eps, ptr(w),
                                                                  w.numel(), stream_ptr()))
            else:
                check(lib.ce_bag_backward_update_compact_src(ptr(plain), _lib.CE_ACT_F32, R, D, nb, ptr(go), _lib.CE_ACT_F32,
                                                             ptr(keys.keys), None, ptr(mom), R, lr, eps,
                                                             _lib.CE_OPT_ROWWISE_ADAGRAD, _lib.CE_ROUND_NEAREST, 0, ptr(w),
                                                             w.numel(), stream_ptr()))
        return run

    variants = {}
    for t in ("fp32", "elementwise", "partial", "adam"):
        variants[f"fwd_keys_1id_{t}"] = fwd(t, keys)
    for acc in ("cache", "step"):
        for opt in ("adagrad", "elementwise", "partial", "adam"):
            variants[f"update_{opt}_{acc}"] = upd(opt, acc)
    names = list(variants)
    with torch.no_grad():
        # the value check first, on untrained tables: the strided forwards against the fp32 ones, bit for bit
        ok = True
        fwd("fp32", keys)()
        want = out.clone()
        for t in ("elementwise", "partial", "adam"):
            out.zero_()
            fwd(t, keys)()
            ok = ok and bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
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
        calls = 2 * (3 + a.reps * a.inner)
        ok = ok and all(int(s.item()) == calls for s in steps.values())
        ok = ok and bool(torch.isfinite(tables["elementwise"]).all()) and bool(torch.isfinite(tables["partial"]).all())
        # a sum of squares behind every row the calls named, and behind no other
        ok = ok and int((tables["elementwise"][:, D:] != 0).any(dim=1).sum().item()) == unique

    res = {"bench": "bench_adagrad_layout", "batch_size": B, "features": F, "dim": D, "table_rows": R,
           "reps": a.reps, "launches_per_timing": a.inner, "hbm_peak_bytes_per_s": HBM_PEAK, "unique_rows": unique,
           "key_driven_row_loads": runs, "values_ok": ok,
           "row_stride_bytes": {"fp32": 4 * D, "elementwise": 8 * D, "partial": 8 * D, "adam": 12 * D},
           "scope": "forwards: one launch through functional.embedding_bag(out=...); updates: one call of the C entry "
                    "(mark, compaction, dense backward, apply); device events"}
    fwd_bytes = {"fwd_keys_1id": runs * 4 * D + nb * 4 * D}
    for n in names:
        med = float(np.median(ms[n]))
        lo, hi = float(min(ms[n])), float(max(ms[n]))
        e = {"us": round(med * 1e3, 2), "us_min_max": [round(lo * 1e3, 2), round(hi * 1e3, 2)],
             "spread": round((hi - lo) / med, 3)}
        if n.startswith("fwd"):
            e["bytes"] = fwd_bytes[n.rsplit("_", 1)[0]]
            e["hbm_peak_fraction"] = round(e["bytes"] / (med * 1e-3) / HBM_PEAK, 3)
        else:
            e["apply_bytes"] = unique * PARTS[n.split("_")[1]] * 4 * D
        res[n] = e
    s = "fwd_keys_1id"
    for t in ("elementwise", "partial", "adam"):
        res[f"{s}_{t}_over_fp32"] = round(res[f"{s}_{t}"]["us"] / res[f"{s}_fp32"]["us"], 3)
    res[f"{s}_fp32_spread"] = res[f"{s}_fp32"]["spread"]
    for acc in ("cache", "step"):
        eu, pu, au, gu = (res[f"update_{o}_{acc}"]["us"] for o in ("elementwise", "partial", "adam", "adagrad"))
        res[f"update_{acc}_elementwise_over_rowwise_adagrad"] = round(eu / gu, 3)
        res[f"update_{acc}_elementwise_over_partial"] = round(eu / pu, 3)
        res[f"update_{acc}_elementwise_over_adam"] = round(eu / au, 3)
        res[f"update_{acc}_partial_over_adam"] = round(pu / au, 3)
        res[f"update_{acc}_adagrad_spread"] = res[f"update_adagrad_{acc}"]["spread"]
        # where between row-wise Adagrad (0) and Adam (1) the element-wise update lands
        res[f"update_{acc}_elementwise_between"] = round((eu - gu) / (au - gu), 3) if au != gu else None
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
