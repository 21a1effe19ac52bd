"""What the fused-update switches, the set_fused_* setters and the front of embedding_bag refuse -- with which exception
class and message, and which refusal wins where two apply -- and what they accept: the cases of
tests/golden/fused_refusals.json and the driver that runs them.  Shared by the recorder
(tests/golden/record_fused_refusals.py) and the replays (tests/test_fused_refusals_cpu.py,
tests/test_gpu_fused_refusals.py), so all walk the same calls in the same order.

No kernel runs, not even on a GPU: `sinks(F)` replaces `_BagFn.apply`, `_BagMaxFn.apply` and `_forward_q8` by functions
that raise `Reached` (the sink's name, the mode code and the output dtype it was handed) and `renorm_rows_` by one that
only notes the call.  An outcome is a pair of strings: (exception class, message), ("reached", where) or
("accepted", what was accepted).

Stage A: the switches' constructors.  Stage B: the setters, unbound on a SimpleNamespace stub; the outcome carries every
switch's fields AFTER the call, so a refused setter is seen to change nothing.  Stage C: embedding_bag up to the sinks.
The case lists hold the product of the values that are good somewhere, then every bad value alone and every two of them
together: of two refusals a call names the one it checks first, so the pairs pin the order.

The GPU column (gpu_cases()): on tensors that are not on the GPU FusedRowwiseAdagrad.check refuses the momentum and the
in-row switches' check the step count, so on the CPU every stage-C case of those switches with an lr ends there at the
latest.  Those cases run a second time with every tensor on the device, and with them the one thing the CPU cannot
make: a CPU learning-rate tensor beside a device weight."""
import contextlib
import itertools
import math
import types
import zlib

import torch

KINDS = ("sgd", "rowwise_adagrad", "adam", "partial_rowwise_adam", "adagrad")
IN_ROW = KINDS[2:]
NO_DECAY_NAMES = ("ParallelCachedEmbeddingBag", "ParallelCachedEmbeddingBagTablewise")
Q4 = torch.quint4x2

_NAMES = {}                                      # id(tensor) -> the name it is reported by
_KEEP = []                                       # (the named tensors stay alive, so an id names one tensor)


def named(name, t):
    _NAMES[id(t)] = name
    _KEEP.append(t)
    return t


_SHARED = {}                                     # the CPU tensors of stages A and B, each made once


def shared(name, make):
    if name not in _SHARED:
        _SHARED[name] = named(name, make())
    return _SHARED[name]


def show(v):
    if isinstance(v, torch.Tensor):
        return "tensor:" + _NAMES.get(id(v), "?")
    return repr(v)


FIELDS = ("lr", "deterministic", "accumulator", "weight_decay", "weight_decay_mode", "grad_clip", "grad_clip_mode",
          "rounding", "seed", "eps", "betas", "lr_decay", "layout", "span", "momentum", "row_of_slot", "step",
          "exp_avg_sq")


def fields(switch) -> str:
    """the public fields of a switch, as one string"""
    if switch is None:
        return "None"
    return " ".join([type(switch).__name__] + [f"{n}={show(getattr(switch, n))}" for n in FIELDS if hasattr(switch, n)])


def brief(text: str) -> str:
    """what the fixture keeps of an accepted call's fields: their digest (the fields repeat the arguments, and a
    thousand of them would be most of the file); a replay that differs prints its own fields in full"""
    return f"{zlib.crc32(text.encode()):08x}"


class Reached(Exception):
    pass


@contextlib.contextmanager
def sinks(F):
    """embedding_bag of the `functional` module F ends where a kernel would be launched; yields the list the stand-in
    of renorm_rows_ appends to"""
    notes = []

    def sink(name, mode_at, dtype_at):
        def raiser(*args):
            raise Reached(f"{name} mode={args[mode_at] if mode_at is not None else None} "
                          f"output_dtype={args[dtype_at] if dtype_at is not None else None}")
        return raiser

    saved = (F._forward_q8, F.renorm_rows_)
    F._BagFn.apply = staticmethod(sink("_BagFn", 4, 13))
    F._BagMaxFn.apply = staticmethod(sink("_BagMaxFn", None, None))
    F._forward_q8 = sink("_forward_q8", 4, 9)
    F.renorm_rows_ = lambda *a, **k: notes.append("renorm")
    try:
        yield notes
    finally:
        del F._BagFn.apply, F._BagMaxFn.apply
        F._forward_q8, F.renorm_rows_ = saved


def outcome(thunk) -> tuple:
    try:
        return ("accepted", thunk() or "")
    except Reached as r:
        return ("reached", str(r))
    except Exception as e:                       # noqa: BLE001 -- the class and the message ARE the outcome
        return (type(e).__name__, str(e))


def singles_and_pairs(bads):
    """bads: [(axis, value)] -> every one alone, then every two of different axes together, as {axis: value}"""
    out = [{a: v} for a, v in bads]
    out += [{a: v, b: w} for (a, v), (b, w) in itertools.combinations(bads, 2) if a != b]
    return out


# ------------------------------------------------------------------------------------------------ values by name
def lr_value(name, dev="cpu"):
    if name == "none":
        return None
    if name in ("float", "neg"):
        return 0.05 if name == "float" else -1.0
    t = {"tensor": lambda: torch.full((1,), 0.05, device=dev),
         "cpu_tensor": lambda: torch.full((1,), 0.05),
         "fp16": lambda: torch.full((1,), 0.05, dtype=torch.float16, device=dev),
         "two": lambda: torch.zeros(2, device=dev),
         "grad": lambda: torch.full((1,), 0.05, device=dev, requires_grad=True),
         # (a tensor of one element is contiguous whatever its strides: the strided one has two)
         "strided": lambda: torch.zeros(4, device=dev)[::2]}[name]
    return shared("lr_" + name, t) if dev == "cpu" else named("lr_" + name, t())


DECAY = {"0": (0.0, "l2"), "l2": (0.01, "l2"), "decoupled": (0.01, "decoupled"),
         "neg": (-1.0, "l2"), "nan": (math.nan, "l2"), "mode": (0.01, "l1"), "tensor": (None, "l2")}
CLIP = {"none": (None, "value"), "value": (0.5, "value"), "row_norm": (0.5, "row_norm"), "inf": (math.inf, "value"),
        "zero": (0, "value"), "mode": (0.5, "norm"), "tensor": (None, "value")}
EXTRA = {"": {}, "beta1": {"betas": (1.0, 0.999)}, "eps_neg": {"eps": -1.0}, "lr_decay_neg": {"lr_decay": -0.5},
         "layout": {"layout": "lamb"}}
EXTRAS_OF = {"sgd": (), "rowwise_adagrad": ("eps_neg",), "adam": ("beta1", "eps_neg", "layout"),
             "partial_rowwise_adam": ("beta1", "eps_neg"), "adagrad": ("eps_neg", "lr_decay_neg")}


def decay_kw(name):
    wd, mode = DECAY[name]
    return {"weight_decay": shared("decay_tensor", lambda: torch.tensor(0.01)) if name == "tensor" else wd,
            "weight_decay_mode": mode}


def clip_kw(name):
    clip, mode = CLIP[name]
    return {"grad_clip": shared("clip_tensor", lambda: torch.tensor(0.5)) if name == "tensor" else clip, "grad_clip_mode": mode}


# ------------------------------------------------------------------------------------------------ stage A
ARGS = ("lr", "det", "acc", "decay", "clip", "extra")
BAD_ARGS = [("lr", v) for v in ("neg", "fp16", "two", "grad", "strided")] + [("acc", "rows")] + \
    [("decay", v) for v in ("neg", "nan", "mode", "tensor")] + [("clip", v) for v in ("zero", "mode", "tensor")]
# the bad values are laid over a plain call and over one whose good values already collide with each other
ARG_BASES = (dict(lr="float", det=False, acc="cache", decay="0", clip="none", extra=""),
             dict(lr="tensor", det=True, acc="step", decay="l2", clip="value", extra=""))


def arg_sets(extras=()):
    """the constructors' and setters' arguments: the product of the good values, then every bad value alone and every
    two together over ARG_BASES"""
    out = [dict(zip(ARGS, g)) for g in itertools.product(
        ("none", "float", "tensor"), (False, True), ("cache", "step", "sorted"), ("0", "l2", "decoupled"),
        ("none", "value", "row_norm", "inf"), ("",))]
    bads = BAD_ARGS + [("extra", e) for e in extras]
    for base in ARG_BASES:
        out += [{**base, **bad} for bad in singles_and_pairs(bads)]
    return out


def stage_a_cases():
    return [(kind, a) for kind in KINDS for a in arg_sets(EXTRAS_OF[kind])]


def construct(F, kind, a):
    kw = dict(deterministic=a["det"], accumulator=a["acc"], **decay_kw(a["decay"]), **clip_kw(a["clip"]),
              **EXTRA[a["extra"]])
    if kind in ("adam", "partial_rowwise_adam"):
        kw.setdefault("layout", kind)
    cls = {"sgd": F.FusedSGD, "rowwise_adagrad": F.FusedRowwiseAdagrad, "adagrad": F.FusedAdagrad}.get(kind, F.FusedAdam)
    return cls(lr_value(a["lr"]), **kw)


def run_stage_a(F):
    return [outcome(lambda: fields(construct(F, kind, a))) for kind, a in stage_a_cases()]


def brief_outcomes(rows):
    """stage A as the fixture holds it: the fields of an accepted constructor by their digest"""
    return [(k, brief(what)) if k == "accepted" else (k, what) for k, what in rows]


# ------------------------------------------------------------------------------------------------ stage B
SETTERS = ("set_fused_sgd", "set_fused_rowwise_adagrad", "set_fused_adam", "set_fused_adagrad")
STUB_AXES = ("layout", "table", "mode", "no_decay", "rounding", "other", "momentum1")
STUB_BASE = dict(layout=None, table=torch.float32, mode="sum", no_decay=None, rounding="stochastic", other="none",
                 momentum1="none")
STUB_DEVIATIONS = [("layout", v) for v in IN_ROW] + [("table", v) for v in (torch.bfloat16, torch.float16, torch.uint8, Q4)] + \
    [("mode", v) for v in ("mean", "max")] + [("no_decay", v) for v in NO_DECAY_NAMES] + [("rounding", "nearest")] + \
    [("other", v) for v in ("sgd", "rowwise_adagrad")] + [("momentum1", "ones")]
# the arguments every pair of stub deviations is called with
FEW_ARGS = [{**ARG_BASES[0], **d} for d in (
    {}, {"lr": "none", "acc": "step"}, {"lr": "tensor"}, {"det": True}, {"lr": "tensor", "det": True}, {"acc": "step"},
    {"decay": "l2"}, {"clip": "value"}, {"decay": "l2", "clip": "value", "det": True}, {"lr": "neg"}, {"acc": "rows"},
    {"decay": "neg"}, {"clip": "zero"})]


def make_stub(F, s):
    step = shared("step", lambda: torch.zeros(1, dtype=torch.int64))
    mgr = types.SimpleNamespace(momentum1=None if s["momentum1"] == "none" else shared("momentum1", lambda: torch.ones(4)),
                                cached_idx_map=shared("cached_idx_map", lambda: torch.arange(4, dtype=torch.int32)),
                                exp_avg_sq=shared("exp_avg_sq", lambda: torch.zeros(4)), num_embeddings=4, device="cpu")
    stub = types.SimpleNamespace(fused_optimizer=s["layout"], table_dtype=s["table"], mode=s["mode"],
                                 _no_weight_decay=s["no_decay"], weight_rounding=s["rounding"], weight_rounding_seed=0,
                                 fused_sgd=F.FusedSGD(None), fused_adagrad=F.FusedRowwiseAdagrad(None), fused_adam=None,
                                 fused_elementwise_adagrad=None, cache_weight_mgr=mgr, num_embeddings=4, embedding_dim=8)
    if s["layout"] == "adagrad":
        stub.fused_elementwise_adagrad = F.FusedAdagrad(None, step=step)
    elif s["layout"] == "partial_rowwise_adam":
        stub.fused_adam = F.FusedAdam(None, step=step, layout=s["layout"], exp_avg_sq=mgr.exp_avg_sq,
                                      row_of_slot=mgr.cached_idx_map)
    elif s["layout"] == "adam":
        stub.fused_adam = F.FusedAdam(None, step=step)
    if s["other"] != "none":
        (stub.fused_sgd if s["other"] == "sgd" else stub.fused_adagrad).lr = 0.1
    return stub


def stub_state(stub) -> str:
    m1 = stub.cache_weight_mgr.momentum1
    return " | ".join([fields(stub.fused_sgd), fields(stub.fused_adagrad), fields(stub.fused_adam),
                       fields(stub.fused_elementwise_adagrad), f"rounding={stub.weight_rounding!r},{stub.weight_rounding_seed!r}",
                       "momentum1=" + ("None" if m1 is None else f"{show(m1)} sum {float(m1.sum())}")])


def stage_b_cases():
    """[(setter, stub deviations, arguments)]; the sharded module's setters and set_weight_rounding come last"""
    one = [{a: v} for a, v in STUB_DEVIATIONS]
    two = [d for d in singles_and_pairs(STUB_DEVIATIONS) if len(d) == 2]
    out = []
    for setter in SETTERS:
        extras = {"set_fused_adam": ("beta1", "eps_neg"), "set_fused_adagrad": ("eps_neg", "lr_decay_neg")}.get(setter, ())
        ok = lambda a: not (setter == "set_fused_adagrad" and a["det"])       # noqa: E731 -- (it has no deterministic=)
        # the plain stub -- for an in-row setter the stub of its layout -- takes every argument set; a stub that differs
        # in one thing the few and every bad argument alone; one that differs in two things the few
        plain = {"set_fused_adam": {"layout": "adam"}, "set_fused_adagrad": {"layout": "adagrad"}}.get(setter, {})
        out += [(setter, plain, a) for a in arg_sets(extras) if ok(a)]
        bad = [{**base, a: v} for base in ARG_BASES for a, v in BAD_ARGS + [("extra", e) for e in extras]]
        out += [(setter, d, a) for d in ([{}] if plain else []) + one if d != plain for a in FEW_ARGS + bad if ok(a)]
        out += [(setter, d, a) for d in two for a in FEW_ARGS if ok(a)]
    for setter in ("sharded.set_fused_sgd", "sharded.set_fused_rowwise_adagrad"):
        out += [(setter, {}, {**ARG_BASES[0], "lr": lr, "decay": d, "clip": c}) for lr, d, c in itertools.product(
            ("none", "float", "tensor"), ("0", "l2", "neg", "mode"), ("none", "value", "zero", "mode"))]
    for d in [{}] + [{"table": v} for v in (torch.bfloat16, torch.float16, torch.uint8, Q4)]:
        out += [("set_weight_rounding", d, {"rounding": r, "seed": s}) for r in ("nearest", "stochastic", "up")
                for s in (0, 7)]
    return out


def run_stage_b(F, E, Sharded):
    """E: CachedEmbeddingBag, Sharded: the row-wise sharded module.  [(outcome, state after the call)]"""
    rows = []
    for setter, dev, a in stage_b_cases():
        if setter.startswith("sharded."):
            stub = types.SimpleNamespace(_lr=[None])
            fn = getattr(Sharded, setter[8:])
            got = outcome(lambda: fn(stub, lr_value(a["lr"]), **decay_kw(a["decay"]), **clip_kw(a["clip"])))
            rows.append((got, f"_lr={stub._lr[0] if not isinstance(stub._lr[0], torch.Tensor) else show(stub._lr[0])!r}"))
            continue
        stub = make_stub(F, {**STUB_BASE, **dev})
        if setter == "set_weight_rounding":
            got = outcome(lambda: E.set_weight_rounding(stub, a["rounding"], a["seed"]))
        else:
            kw = dict(accumulator=a["acc"], **decay_kw(a["decay"]), **clip_kw(a["clip"]), **EXTRA[a["extra"]])
            if setter != "set_fused_adagrad":
                kw["deterministic"] = a["det"]
            got = outcome(lambda: getattr(E, setter)(stub, lr_value(a["lr"]), **kw))
        rows.append((got, stub_state(stub)))
    return rows


def brief_states(rows):
    """stage B as the fixture holds it: the state after the call by its digest"""
    return [(got, brief(state)) for got, state in rows]


# ------------------------------------------------------------------------------------------------ stage C
# name -> (shape, dtype, quant_bits)
WEIGHTS = {"fp32": ((8, 8), torch.float32, 8), "bf16": ((8, 8), torch.bfloat16, 8), "fp16": ((8, 8), torch.float16, 8),
           "bf16_dim12": ((8, 12), torch.bfloat16, 8),             # check_w16_dim refuses it
           "q8": ((8, 32), torch.uint8, 8), "q4": ((8, 32), torch.uint8, 4), "q8_dim8": ((8, 24), torch.uint8, 8),
           "q4_dim16": ((8, 24), torch.uint8, 4), "uint8_1d_q4": ((32,), torch.uint8, 4),
           "quant_bits3": ((8, 32), torch.uint8, 3), "uint8_1d": ((32,), torch.uint8, 8),
           "adam": ((8, 24), torch.float32, 8), "partial_rowwise_adam": ((8, 16), torch.float32, 8),
           "adagrad": ((8, 16), torch.float32, 8),
           "fp32_w25": ((8, 25), torch.float32, 8),                # no multiple of a span
           "bf16_w24": ((8, 24), torch.bfloat16, 8)}               # an in-row switch over a 16-bit weight
PLAIN = ("fp32", "bf16", "fp16")
SWITCH = ("kind", "lr", "det", "acc", "decay", "clip", "rounding", "state")

CALL = ("mode", "max_norm", "sparse", "psw", "output_dtype")
CALL_BASE = dict(mode="sum", max_norm=None, sparse=False, psw="none", output_dtype=None)
CALL_DEVIATIONS = [("mode", v) for v in ("mean", "max", "prod")] + [("max_norm", 1.0), ("sparse", True)] + \
    [("psw", v) for v in ("plain", "grad", "grad_no_grad")] + [("output_dtype", v) for v in (torch.bfloat16, torch.int32)]


def calls(full=False):
    if full:
        return [dict(zip(CALL, c)) for c in itertools.product(
            ("sum", "mean", "max", "prod"), (None, 1.0), (False, True), ("none", "plain", "grad", "grad_no_grad"),
            (None, torch.bfloat16, torch.int32))]
    return [dict(CALL_BASE)] + [{**CALL_BASE, **d} for d in singles_and_pairs(CALL_DEVIATIONS)]


def switches():
    """the switch of every context, as a dict over SWITCH; None: no switch.  The fields are SET on a switch built with
    lr=None, so that what a constructor refuses -- deterministic=True beside a tensor lr, a decay on an fp32 SGD switch
    -- is there too: the front asks again because a switch can change after it was built."""
    out = []
    for kind in ("sgd", "rowwise_adagrad"):
        for lr, det, acc, decay, clip in itertools.product(("none", "float", "tensor"), (False, True), ("cache", "step"),
                                                           ("0", "l2"), ("none", "value")):
            for rounding in ("stochastic", "nearest") if kind == "rowwise_adagrad" else ("stochastic",):
                out.append(dict(zip(SWITCH, (kind, lr, det, acc, decay, clip, rounding, "ok"))))
    return out


def in_row_switches(kind):
    states = ("ok", "none") + (("no_exp_avg_sq", "empty_exp_avg_sq", "row_of_slot", "row_of_slot_int64")
                               if kind == "partial_rowwise_adam" else ())
    return [dict(zip(SWITCH, (kind, lr, False, "step", "0", "none", "nearest", st)))
            for lr in ("none", "float", "neg", "tensor") for st in states]


def contexts():
    """[(weight name, switch dict or None, full product of the call's arguments?)]"""
    out = [(w, None, True) for w in WEIGHTS]
    out += [(w, s, False) for w in PLAIN[:2] for s in switches()]          # (fp16: the few below; bf16 has them all)
    few = [dict(zip(SWITCH, s)) for s in (
        ("sgd", "none", False, "cache", "0", "none", "stochastic", "ok"),
        ("sgd", "float", False, "cache", "0", "none", "stochastic", "ok"),
        ("sgd", "tensor", False, "cache", "0", "none", "stochastic", "ok"),
        ("sgd", "float", True, "cache", "l2", "none", "stochastic", "ok"),
        ("sgd", "float", False, "step", "0", "value", "stochastic", "ok"),
        ("rowwise_adagrad", "float", False, "cache", "0", "none", "stochastic", "ok"),
        ("rowwise_adagrad", "tensor", True, "step", "l2", "value", "stochastic", "ok"))]
    out += [(w, s, False) for w in WEIGHTS if w not in PLAIN[:2] for s in few]
    # row-wise Adagrad's own state, as FusedRowwiseAdagrad.check looks at it
    out += [("fp32", dict(zip(SWITCH, ("rowwise_adagrad", "float", False, "cache", "0", "none", "stochastic", st))), False)
            for st in ("none", "short_momentum", "row_of_slot", "row_of_slot_short", "row_of_slot_int64")]
    for kind in IN_ROW:
        out += [(kind, s, False) for s in in_row_switches(kind)]
        odd = [s for s in in_row_switches(kind) if s["state"] == "ok" and s["lr"] in ("none", "float")]
        out += [(w, s, False) for w in ("fp32", "fp32_w25", "bf16_w24", "q8") for s in odd]
    return out


def stage_c_cases():
    return [(w, s, c) for w, s, full in contexts() for c in calls(full)]


def gpu_cases():
    """the stage-C cases whose switch keeps state on the device and has an lr, and a CPU lr beside a device weight"""
    out = [(w, s, c) for w, s, c in stage_c_cases()
           if s is not None and s["kind"] != "sgd" and s["lr"] != "none"]
    for kind, w in (("sgd", "fp32"), ("sgd", "bf16"), ("rowwise_adagrad", "fp32"), ("adam", "adam"),
                    ("adagrad", "adagrad")):
        s = dict(zip(SWITCH, (kind, "cpu_tensor", False, "step" if kind in IN_ROW else "cache", "0", "none", "nearest", "ok")))
        out += [(w, s, c) for c in calls()[:len(CALL_DEVIATIONS) + 1]]
    return out


class Tensors:
    """the tensors of stage C on one device, each made once"""

    def __init__(self, dev):
        self.dev, self.made = dev, {}

    def get(self, name, make):
        if name not in self.made:
            self.made[name] = named(name, make())
        return self.made[name]

    def weight(self, name):
        shape, dtype, _ = WEIGHTS[name]
        return self.get("weight_" + name, lambda: torch.zeros(shape, dtype=dtype, device=self.dev))

    def lr(self, name):
        if name in ("none", "float", "neg"):
            return lr_value(name)
        return self.get("lr_" + name, lambda: lr_value(name, self.dev))


def make_switch(F, s, t: Tensors):
    if s is None:
        return None
    dev, kind, state = t.dev, s["kind"], s["state"]
    int32 = lambda n, dt=torch.int32: torch.arange(n, dtype=dt, device=dev)          # noqa: E731
    if kind == "sgd":
        sw = F.FusedSGD(None)
    elif kind == "rowwise_adagrad":
        sw = F.FusedRowwiseAdagrad(None, 1e-6)
        if state != "none":
            sw.momentum = t.get("momentum4", lambda: torch.zeros(4, device=dev)) if state == "short_momentum" else \
                t.get("momentum", lambda: torch.zeros(8, device=dev))
        if state.startswith("row_of_slot"):
            sw.row_of_slot = {"row_of_slot": lambda: t.get("row_of_slot", lambda: int32(8)),
                              "row_of_slot_short": lambda: t.get("row_of_slot4", lambda: int32(4)),
                              "row_of_slot_int64": lambda: t.get("row_of_slot64", lambda: int32(8, torch.int64))}[state]()
    else:
        step = None if state == "none" else t.get("step", lambda: torch.zeros(1, dtype=torch.int64, device=dev))
        if kind == "adagrad":
            sw = F.FusedAdagrad(None, step=step)
        elif kind == "adam":
            sw = F.FusedAdam(None, step=step)
        else:
            v = None if state == "no_exp_avg_sq" else t.get("exp_avg_sq0", lambda: torch.zeros(0, device=dev)) \
                if state == "empty_exp_avg_sq" else t.get("exp_avg_sq", lambda: torch.zeros(8, device=dev))
            ros = None if not state.startswith("row_of_slot") else t.get("row_of_slot", lambda: int32(8)) \
                if state == "row_of_slot" else t.get("row_of_slot64", lambda: int32(8, torch.int64))
            sw = F.FusedAdam(None, step=step, layout=kind, exp_avg_sq=v, row_of_slot=ros)
    sw.lr = t.lr(s["lr"])
    if kind not in IN_ROW:
        sw.deterministic, sw.accumulator, sw.rounding = s["det"], s["acc"], s["rounding"]
        sw.weight_decay = DECAY[s["decay"]][0]
        sw.grad_clip = CLIP[s["clip"]][0]
    return sw


def run_stage_c(F, cases, dev="cpu"):
    """the outcome of every case, inside sinks(F); ("reached", ...) says which sink, and how often renorm_rows_ ran"""
    t = Tensors(dev)
    indices = torch.tensor([0, 3, 3, 7, 1, 5], device=dev)
    offsets = torch.tensor([0, 2, 3, 5], device=dev)
    psws = {"none": None, "plain": torch.ones(6, device=dev), "grad": torch.ones(6, device=dev, requires_grad=True)}
    psws["grad_no_grad"] = psws["grad"]
    rows, last, sw = [], None, None
    with sinks(F) as notes:
        for w, s, c in cases:
            if last is not s:                    # (the cases of one context follow each other)
                sw, last = make_switch(F, s, t), s
            del notes[:]
            with torch.no_grad() if c["psw"] == "grad_no_grad" else contextlib.nullcontext():
                kind, what = outcome(lambda: F.embedding_bag(
                    indices, t.weight(w), offsets, c["max_norm"], mode=c["mode"], sparse=c["sparse"],
                    per_sample_weights=psws[c["psw"]], fused_sgd=sw, output_dtype=c["output_dtype"],
                    quant_bits=WEIGHTS[w][2]))
            rows.append((kind, what + f" renorm={len(notes)}" if kind == "reached" else what))
    return rows


# ------------------------------------------------------------------------------------------------ the fixture's form
_DIGITS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def encode(index: list) -> str:
    """two base-62 digits per case"""
    assert max(index, default=0) < 62 * 62
    return "".join(_DIGITS[i // 62] + _DIGITS[i % 62] for i in index)


def decode(text: str) -> list:
    return [62 * _DIGITS.index(text[i]) + _DIGITS.index(text[i + 1]) for i in range(0, len(text), 2)]


def digest(cases) -> int:
    """of a case list: the fixture names the list it was recorded for"""
    return zlib.crc32(repr(cases).encode())


def differences(got: list, want: list, cases: list, limit: int = 5) -> str:
    """'' where got == want, else how many cases differ and the first few"""
    assert len(got) == len(want) == len(cases), (len(got), len(want), len(cases))
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    if not bad:
        return ""
    return f"{len(bad)} of {len(got)} cases answered differently:\n" + "\n".join(
        f"  {c}\n    got      {g}\n    recorded {w}" for c, g, w in bad[:limit])
