"""Which C entry `_BagFn.backward` calls, and with which arguments: the cases of tests/golden/update_dispatch.json, the
driver that runs one of them on the CPU, and the fixture's column form.

Nothing here needs a GPU and no kernel runs: `functional.lib` is replaced by a stand-in that hands the host-only
`*_workspace` / `ce_bag_presort_len` functions on to the real library and, for every other entry, notes (name, args)
and returns CE_OK; `functional.stream_ptr` is a constant; `_BagFn.backward(ctx, grad_out)` is called directly on CPU
tensors with a SimpleNamespace for ctx.  A noted call is then turned into data: an address becomes the name of the
tensor it belongs to, a float its repr.

tests/golden/record_update_dispatch.py wrote the fixture from the commit named in it; tests/test_update_dispatch_cpu.py
holds the code of the checkout to it.  A new optimizer: add its cases to base_cases() and record only those
(record_update_dispatch.py --only)."""
import itertools
import types
from typing import NamedTuple, Optional

import torch

ROWS, DIM, BAGS, NNZ = 8, 8, 4, 6               # nothing runs: the smallest shapes that keep every length distinct
STREAM = 0x5EED00000000                         # what stream_ptr() answers here
LR, EPS, WEIGHT_DECAY, GRAD_CLIP, BETAS, LR_DECAY, SEED = 0.05, 1e-6, 0.01, 0.5, (0.9, 0.98), 0.25, 12345
WORKSPACES = ("_ws", "_ws16", "_ws_step", "_ws_sorted")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
IN_ROW = ("adam", "partial_rowwise_adam", "adagrad")
VARIANTS = ("grad_bf16", "grad_fp16", "mean", "psw", "hook2", "last_offset", "off32", "ranges")


class Case(NamedTuple):
    optimizer: str                  # "none", "sgd", "rowwise_adagrad", "adam", "partial_rowwise_adam", "adagrad"
    table: str                      # "fp32", "bf16", "fp16"
    lookups: str                    # "slots", "keys" (slots + a presorted key tensor), "src" (SrcKeys)
    path: str                       # "cache", "step", "sorted" (deterministic=True for SGD and row-wise Adagrad)
    lr: str                         # "float", "tensor"
    decay: str                      # "0", "l2", "decoupled"
    clip: str                       # "none", "value", "row_norm"
    rounding: str                   # "stochastic", "nearest"; "-": the switch has none
    row_of_slot: str                # "none", "tensor"
    variant: str = ""               # one of VARIANTS: what the smaller sweep changes


AXES = Case._fields


def base_cases():
    """the full product of the axes, what the pre-forward checks refuse included (build() sorts it out)"""
    for table, lookups in itertools.product(DTYPES, ("slots", "keys", "src")):
        yield Case("none", table, lookups, "cache", "float", "0", "none", "-", "none")
    tail = list(itertools.product(("float", "tensor"), ("0", "l2", "decoupled"), ("none", "value", "row_norm")))
    for opt, table, lookups, path in itertools.product(("sgd", "rowwise_adagrad"), DTYPES, ("slots", "keys", "src"),
                                                       ("cache", "step", "sorted")):
        for (lr, decay, clip), rounding, ros in itertools.product(tail, ("stochastic", "nearest"), ("none", "tensor")):
            yield Case(opt, table, lookups, path, lr, decay, clip, rounding, ros)
    for opt, lookups, path in itertools.product(IN_ROW, ("slots", "keys", "src"), ("cache", "step", "sorted")):
        for (lr, decay, clip), ros in itertools.product(tail, ("none",) if opt == "adagrad" else ("none", "tensor")):
            yield Case(opt, "fp32", lookups, path, lr, decay, clip, "-", ros)


def variants(case: Case):
    """the smaller sweep over one case"""
    return [case._replace(variant=v) for v in VARIANTS]


class Call(NamedTuple):
    """what one case must hand to a driver: everything _BagFn.backward reads, and the tensors by name"""
    ctx: types.SimpleNamespace
    grad_out: torch.Tensor
    fused: object
    named: dict


def build(case: Case, F) -> Optional[Call]:
    """the inputs of `case` for the `functional` module F, or None where embedding_bag refuses the combination before
    its forward (the switches' constructors, then F.check_front: the front of embedding_bag itself; the source-row
    keys' refusals)"""
    v = case.variant
    src, det = case.lookups == "src", case.path == "sorted"
    mode = "mean" if v == "mean" else "sum"
    if (v == "ranges" and not src) or (src and v in ("mean", "psw")):
        return None
    t = {"lr": torch.full((1,), LR)} if case.lr == "tensor" else {}
    if case.row_of_slot == "tensor":
        t["row_of_slot"] = torch.arange(ROWS, dtype=torch.int32)
    kw = dict(weight_decay=0.0 if case.decay == "0" else WEIGHT_DECAY,
              weight_decay_mode="l2" if case.decay == "0" else case.decay,
              grad_clip=None if case.clip == "none" else GRAD_CLIP,
              grad_clip_mode="value" if case.clip == "none" else case.clip)
    lr = t.get("lr", LR)
    span = 1
    try:
        if case.optimizer == "none":
            fused = None
        elif case.optimizer in ("sgd", "rowwise_adagrad"):
            if case.optimizer == "sgd":
                fused = F.FusedSGD(lr, deterministic=det, accumulator="cache" if det else case.path, **kw)
                fused.row_of_slot = t.get("row_of_slot")
            else:
                t["momentum"] = torch.zeros(ROWS)
                fused = F.FusedRowwiseAdagrad(lr, EPS, t["momentum"], t.get("row_of_slot"), deterministic=det,
                                              accumulator="cache" if det else case.path, **kw)
            fused.rounding, fused.seed = case.rounding, SEED
            # (the switch's own state would have to be on a GPU: FusedRowwiseAdagrad.check is not what is asked here)
            fused.check = lambda weight: None
            F.check_front(fused, torch.empty(ROWS, DIM, dtype=DTYPES[case.table]), mode, None, False, None, None)
            del fused.check
        else:
            t["step"] = torch.zeros(1, dtype=torch.int64)
            if case.optimizer == "adagrad":
                fused = F.FusedAdagrad(lr, EPS, LR_DECAY, case.path, t["step"], **kw)
            else:
                if case.optimizer == "partial_rowwise_adam":
                    t["exp_avg_sq"] = torch.zeros(ROWS)
                fused = F.FusedAdam(lr, BETAS, EPS, case.path, t["step"], layout=case.optimizer,
                                    exp_avg_sq=t.get("exp_avg_sq"), row_of_slot=t.get("row_of_slot"), **kw)
            span = fused.span
    except NotImplementedError:
        return None
    hook = 2 if v == "hook2" else 0
    last = v == "last_offset"
    t["weight"] = torch.zeros(ROWS, span * DIM, dtype=DTYPES[case.table])
    t["indices"] = torch.tensor([0, 3, 3, 7, 1, 5])
    t["offsets"] = torch.tensor([0, 2, 3, 5] + [NNZ] * last, dtype=torch.int32 if v == "off32" else torch.int64)
    if v == "psw":
        t["psw"] = torch.ones(NNZ)
    g = torch.zeros((BAGS // 2, 2, DIM) if hook else (BAGS, DIM),
                    dtype=DTYPES[v[5:]] if v.startswith("grad_") else torch.float32)
    t["grad_out"] = g
    pre = None
    if case.lookups != "slots":
        t["keys"] = pre = torch.zeros(F.presort_len(NNZ), dtype=torch.int64)
    if src:
        if v == "ranges":
            t["ranges"] = torch.zeros(pre.numel() // 16384, 2, dtype=torch.int64)
        pre = F.SrcKeys(pre, BAGS, last, hook, t.get("ranges"))
    ctx = types.SimpleNamespace(saved_tensors=(t["indices"], t["offsets"], t.get("psw")), weight=t["weight"],
                                args=(F._MODES[mode], last, hook, False, fused, BAGS), presorted=pre, masked=False,
                                needs_input_grad=(True,) + (False,) * 13)
    return Call(ctx, g, fused, t)


class RecordingLib:
    """stands in for functional.lib: the host-only size functions are the real library's, every other entry notes its
    call and answers CE_OK"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith("_workspace") or name == "ce_bag_presort_len":
            fn = getattr(self.real, name)
        else:
            def fn(*args, _name=name, _calls=self.calls):
                _calls.append((_name, args))
                return 0
        setattr(self, name, fn)                  # (asked once per name)
        return fn


class patched:
    """with patched(F) as rec: F.lib is a RecordingLib, F.stream_ptr a constant"""

    def __init__(self, F):
        self.F = F

    def __enter__(self):
        self.saved = (self.F.lib, self.F.stream_ptr)
        self.F.lib, self.F.stream_ptr = RecordingLib(self.F.lib), lambda: STREAM
        return self.F.lib

    def __exit__(self, *exc):
        self.F.lib, self.F.stream_ptr = self.saved


def normalise(args, call: Call) -> list:
    """the arguments as data: the name of the tensor (or of the workspace attribute) an address belongs to, "stream",
    "fresh" for any other address, the repr of a float; an int and None stay"""
    names = {t.data_ptr(): n for n, t in call.named.items()}
    for a in WORKSPACES:
        ws = getattr(call.fused, a, None)
        if ws is not None:
            names[ws.data_ptr()] = a
    names[STREAM] = "stream"
    out = []
    for a in args:
        if isinstance(a, float):
            out.append(repr(a))
        elif a is None:
            out.append(None)
        else:
            assert type(a) is int, (type(a), a)
            out.append(names.get(a, "fresh" if a >= 1 << 32 else a))
    return out


def run(case: Case, F, rec: RecordingLib):
    """(entry, normalised arguments, allocated workspaces) of `case` under the patched module F, or None where the
    combination is refused before the forward"""
    call = build(case, F)
    if call is None:
        return None
    del rec.calls[:]
    F._BagFn.backward(call.ctx, call.grad_out)
    assert len(rec.calls) == 1, (case, [n for n, _ in rec.calls])
    name, args = rec.calls[0]
    allocated = ",".join(a for a in WORKSPACES if getattr(call.fused, a, None) is not None)
    return name, normalise(args, call), allocated


# ---- the fixture's column form: per entry a table, one row per case, whose columns are the case's axes, the arguments by
# position and the allocated workspaces; a column is {"all": value} or {"values": [...], "rows": which value per row}
_DIGITS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def pack_column(column: list):
    values = []                                  # (ints, strings and None: equal means the same)
    for v in column:
        if v not in values:
            values.append(v)
    if len(values) == 1:
        return {"all": values[0]}
    index = [values.index(v) for v in column]
    return {"values": values, "rows": "".join(_DIGITS[i] for i in index) if len(values) <= len(_DIGITS) else index}


def unpack_column(col: dict, n: int) -> list:
    if "all" in col:
        return [col["all"]] * n
    rows = col["rows"]
    return [col["values"][_DIGITS.index(r) if isinstance(r, str) else r] for r in rows]


def pack(records: list) -> dict:
    """records: [(Case, entry, args, allocated)] -> {entry: table}"""
    out = {}
    for entry in sorted({r[1] for r in records}):
        rows = [r for r in records if r[1] == entry]
        width = {len(r[2]) for r in rows}
        assert len(width) == 1, (entry, width)
        out[entry] = {"n": len(rows),
                      "case": {ax: pack_column([getattr(r[0], ax) for r in rows]) for ax in AXES},
                      "args": [pack_column([r[2][i] for r in rows]) for i in range(width.pop())],
                      "allocated": pack_column([r[3] for r in rows])}
    return out


def unpack(entries: dict) -> list:
    records = []
    for entry, tab in entries.items():
        n = tab["n"]
        axes = [unpack_column(tab["case"][ax], n) for ax in AXES]
        args = [unpack_column(c, n) for c in tab["args"]]
        allocated = unpack_column(tab["allocated"], n)
        for i in range(n):
            records.append((Case(*(a[i] for a in axes)), entry, [a[i] for a in args], allocated[i]))
    return records
