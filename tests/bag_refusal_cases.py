"""The argument sets behind tests/golden/bag_refusals.json: every C entry that ce_bag.hip defines, called from one good
argument set with every argument in turn -- and every two arguments together -- set to its bad values.  Shared by the
recorder (tests/golden/record_bag_refusals.py) and the replay (tests/test_bag_refusals_cpu.py), so both walk the same
calls in the same order.

The pointers are made-up, aligned addresses: nothing here may run where a launch could succeed.  A call that passes
every check reaches its first launch, which fails without a GPU (CE_ERR_HIP)."""
import itertools

CE_ERR_HIP = 2


def _p(i):
    return 0x7f0000000000 + 0x100000 * i            # non-null, 256-byte aligned


_SIZES = {"0": 0, "-1": -1, "2^31-1": 2 ** 31 - 1, "2^31": 2 ** 31}
# kind -> {label: bad value}; a pointer's bad values are made from its good one
_BAD = {
    "rows": _SIZES,
    "size": _SIZES,
    "dim": {"0": 0, "-4": -4, "6": 6, "12": 12, "260": 260, "2048": 2048},
    "act": {"9": 9, "bf16": 1},                       # (bf16: not bad in itself; it moves the alignment rules)
    "wdtype": {"f32": 0, "f16": 2, "7": 7},
    "mode": {"mean": 1, "7": 7},
    "hook": {"7": 7, "-1": -1},                       # 7 does not divide the 64 bags
    "stride": {"-1": -1},
    "keep": {},
}


def _bad_values(kind, good):
    if kind == "ptr":
        return {"null": None, "+4": good + 4, "+8": good + 8}
    if kind == "optptr":                              # good = None: an optional tensor that is absent
        return {"set": _p(15), "+4": _p(15) + 4}
    return _BAD[kind]


def _bag(first, last):
    return [first, ("num_rows", "rows", 1000), ("dim", "dim", 128), ("indices", "ptr", _p(1)), ("nnz", "size", 64),
            ("offsets", "ptr", _p(2)), ("offsets_are_i64", "keep", 0), ("num_bags", "size", 64),
            ("include_last_offset", "keep", 1), ("per_sample_weights", "optptr", None), ("mode", "mode", 0),
            ("hook_features", "hook", 4), (last, "ptr", _p(3))]


_W = ("weight", "ptr", _p(0))
_WD = ("weight_dtype", "wdtype", 1)
_ACT = ("act_dtype", "act", 0)
_LR = ("lr", "keep", 0.1)
_KEYS = ("keys", "ptr", _p(4))
_OPT_KEYS = ("presorted_keys", "optptr", None)
_STREAM = ("stream", "keep", None)


def _src(last):
    return [_W, ("num_rows", "rows", 1000), ("dim", "dim", 128), ("nnz", "size", 64), (last, "ptr", _p(3))]


_WINDOW = [("slots", "ptr", _p(1)), ("nnz_per_batch", "size", 64), ("n_batches", "size", 2), ("num_rows", "rows", 1000)]
_WINDOW_SRC = _WINDOW + [("offsets", "ptr", _p(2)), ("offsets_are_i64", "keep", 0), ("offsets_batch_stride", "stride", 65),
                         ("num_bags", "size", 64), ("include_last_offset", "keep", 1), ("hook_features", "hook", 4)]
_KEYS_OUT = ("keys_out", "ptr", _p(5))

# entry -> [(argument, kind, good value)], in the order of its declaration in include/ce_api.h
ENTRIES = {
    "ce_bag_forward": _bag(_W, "out") + [_STREAM],
    "ce_bag_forward_act": _bag(_W, "out") + [_ACT, _STREAM],
    "ce_bag_forward_w16": [_W, _WD] + _bag(_W, "out")[1:] + [_ACT, _STREAM],
    "ce_bag_forward_src_keys": _src("keys")[:4] + [_KEYS, ("out", "ptr", _p(3)), _STREAM],
    "ce_bag_forward_src_keys_act": _src("keys")[:4] + [_KEYS, ("out", "ptr", _p(3)), _ACT, _STREAM],
    "ce_bag_forward_src_keys_w16": [_W, _WD] + _src("keys")[1:4] + [_KEYS, ("out", "ptr", _p(3)), _ACT, _STREAM],
    "ce_bag_backward_dense": _bag(_W, "grad_out") + [_STREAM],
    "ce_bag_backward_dense_act": _bag(_W, "grad_out") + [_ACT, _OPT_KEYS, _STREAM],
    "ce_bag_backward_dense_presorted": _bag(_W, "grad_out") + [_KEYS, _STREAM],
    "ce_bag_backward_sgd": _bag(_W, "grad_out") + [_LR, _STREAM],
    "ce_bag_backward_sgd_act": _bag(_W, "grad_out") + [_ACT, _LR, _OPT_KEYS, _STREAM],
    "ce_bag_backward_sgd_presorted": _bag(_W, "grad_out") + [_LR, _KEYS, _STREAM],
    "ce_bag_backward_sgd_presorted_src": _src("grad_out") + [_LR, _KEYS, _STREAM],
    "ce_bag_backward_sgd_presorted_src_excl": _src("grad_out") + [_LR, _KEYS, ("seg_id_ranges", "ptr", _p(6)), _STREAM],
    "ce_bag_backward_sgd_src_act": _src("grad_out") + [_ACT, _LR, _KEYS, ("seg_id_ranges", "optptr", None), _STREAM],
    "ce_bag_backward_dense_src_act": _src("grad_out") + [_ACT, _KEYS, _STREAM],
    "ce_bag_backward_dense_presorted_src": _src("grad_out") + [_KEYS, _STREAM],
    "ce_bag_backward_rows": [("grad_rows", "ptr", _p(0)), ("dest_index", "optptr", None)] + _bag(_W, "grad_out")[2:3]
                            + _bag(_W, "grad_out")[4:] + [_STREAM],
    "ce_rows_axpy": [_W, ("num_rows", "rows", 1000), ("dim", "dim", 128), ("index", "ptr", _p(1)), ("n", "size", 64),
                     ("src_rows", "ptr", _p(3)), ("alpha", "keep", -0.1), _STREAM],
    "ce_bag_presort_len": [("nnz", "size", 64)],
    "ce_bag_presort": [("slots", "ptr", _p(1)), ("nnz", "size", 64), ("num_rows", "rows", 1000), _KEYS_OUT, _STREAM],
    "ce_bag_presort_window": _WINDOW + [_KEYS_OUT, _STREAM],
    "ce_bag_presort_window_src": _WINDOW_SRC + [_KEYS_OUT, _STREAM],
    "ce_bag_presort_window_src_excl": _WINDOW_SRC + [("ids", "optptr", None), _KEYS_OUT,
                                                     ("seg_id_ranges", "ptr", _p(6)), _STREAM],
}


def singles(entry):
    """[(label, argument position, bad value)]: every argument of the entry with each of its bad values"""
    out = []
    for pos, (name, kind, good) in enumerate(ENTRIES[entry]):
        out += [(f"{name}={label}", pos, bad) for label, bad in _bad_values(kind, good).items()]
    return out


def cases(entry):
    """[(label, argument tuple)]: the good call, every single perturbation, then every two perturbations of two
    different arguments together"""
    good = [g for _, _, g in ENTRIES[entry]]
    one = singles(entry)
    out = [("good", tuple(good))]
    for label, pos, bad in one:
        args = list(good)
        args[pos] = bad
        out.append((label, tuple(args)))
    for (la, pa, ba), (lb, pb, bb) in itertools.combinations(one, 2):
        if pa == pb:
            continue
        args = list(good)
        args[pa], args[pb] = ba, bb
        out.append((f"{la},{lb}", tuple(args)))
    return out


def run(lib, last_error, entry):
    """[(label, return value, message)] of every case of the entry on the library `lib`.  The message is None where
    the return value says nothing was refused, or where the refusal is the launch's (it carries a line number)."""
    fn = getattr(lib, entry)
    out = []
    for label, args in cases(entry):
        rc = fn(*args)
        refused = entry != "ce_bag_presort_len" and rc not in (0, CE_ERR_HIP)
        out.append((label, int(rc), last_error() if refused else None))
    return out
