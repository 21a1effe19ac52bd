"""torch-facing wrappers of the HIP EmbeddingBag kernels (ce_bag_* in include/ce_api.h).

`embedding_bag` mirrors the call the reference makes through ColossalAI:
``F.embedding_bag(slots, cuda_cached_weight, offsets, max_norm, norm_type, scale_grad_by_freq,
mode, sparse, per_sample_weights, include_last_offset, padding_idx)`` (SURVEY.md A.7;
call sites recsys/models/dlrm.py:99-110, benchmark/benchmark_cache.py:62), with two
additions the reference does not have: `hook_features` folds sparse_embedding_shape_hook
(recsys/models/dlrm.py:26-27) into the output store, and `fused_sgd` applies
SGD.step (recsys/dlrm_main.py:279) -- or, given a FusedRowwiseAdagrad, the exact row-wise
Adagrad step of the reference's baseline (baselines/dlrm_main.py:698-702) -- inside the backward pass.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Union

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

_MODES = {"sum": _lib.CE_MODE_SUM, "mean": _lib.CE_MODE_MEAN}


def _prep(indices: torch.Tensor, offsets: Optional[torch.Tensor], include_last_offset: bool):
    if indices.dim() == 2:
        if offsets is not None:
            raise ValueError("if input is 2D, then offsets has to be None, as input is treated is a "
                             "mini-batch of fixed length sequences")
        rows, length = indices.shape
        offsets = torch.arange(0, rows * length + 1, length, device=indices.device, dtype=torch.int64)
        indices = indices.reshape(-1)
        include_last_offset = True
    elif indices.dim() == 1:
        if offsets is None:
            raise ValueError("offsets has to be a 1D Tensor but got None")
        if offsets.dim() != 1:
            raise ValueError("offsets has to be a 1D Tensor")
    else:
        raise ValueError(f"input has to be 1D or 2D Tensor, but got Tensor of dimension {indices.dim()}")
    if indices.dtype != torch.int64:
        indices = indices.long()
    if offsets.dtype not in (torch.int32, torch.int64):
        offsets = offsets.long()
    indices = indices.contiguous()
    offsets = offsets.contiguous()
    num_bags = offsets.numel() - 1 if include_last_offset else offsets.numel()
    return indices, offsets, include_last_offset, num_bags


class SrcKeys(NamedTuple):
    """Keys of one batch from presort_window(..., offsets=...): row << 32 | grad_out row (ce_bag_presort_window_src).
    They already hold the bag layout they were built for, so embedding_bag(presorted=SrcKeys) checks that the call
    uses the same one; mode must be 'sum' without per-sample weights.
    ranges (presort_window(..., ids=...)): the [min, max] id of every 16384-lookup segment of the batch, int64
    [segments, 2] -- with them the fused-SGD backward updates rows that one lane group owns entirely (flagged in the
    keys) by plain read-modify-write instead of atomics, after checking that no id can occur in two segments."""
    keys: torch.Tensor
    num_bags: int
    include_last_offset: bool
    hook_features: int
    ranges: Optional[torch.Tensor] = None
    # the keys were built for the one-id-per-bag layout (presort_window(identity_bags=True)): the FORWARD can then run
    # from them as well (ce_bag_forward_src_keys: a cache row is loaded once per run of equal rows)
    identity: bool = False


class _BagFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, indices, offsets, psw, mode, include_last, hook_features, sparse, fused, presorted,
                bwd_scale=None, masked=False, out_box=None, out_dtype=torch.float32):
        _lib.require_gpu()
        w16 = weight.dtype in _lib.W16_DTYPES
        assert weight.is_cuda and (w16 or weight.dtype == torch.float32) and weight.is_contiguous()
        # the weight is then [rows, 3 * D]: w | m | v, or [rows, 2 * D]: w | m (3.13) or w | h (3.15)
        adam = isinstance(fused, _IN_ROW)
        partial = adam and fused.layout == "partial_rowwise_adam"
        if psw is not None and ctx.needs_input_grad[3] and fused is not None and fused.lr is not None:
            # d loss / d per_sample_weights[j] = <grad_out[bag of j], weight[indices[j]]> needs the rows as the forward
            # saw them, and the fused update moves them inside backward: refused HERE, before any kernel has run (a
            # refusal inside backward would leave the caller with an exception AND an updated table)
            raise NotImplementedError("gradient w.r.t. per_sample_weights with the fused SGD / row-wise Adagrad "
                                      "update")
        num_bags = offsets.numel() - 1 if include_last else offsets.numel()
        dim = weight.shape[1] // fused.span if adam else weight.shape[1]
        shape = (num_bags // hook_features, hook_features, dim) if hook_features else (num_bags, dim)
        if out_box is not None:
            # the caller's buffer (embedding_bag(out=...)): a static output for graph-captured steps, or one chosen by
            # pick_fast_buffer.  It comes in a box because it is no input of the autograd function.
            out = out_box[0]
            if tuple(out.shape) != shape or out.dtype != out_dtype or not out.is_contiguous() or \
                    out.device != weight.device:
                raise ValueError(f"out= must be a contiguous {_DTYPE_NAMES[out_dtype]} tensor of shape {shape} on "
                                 f"{weight.device}")
        else:
            out = torch.empty(shape, device=weight.device, dtype=out_dtype)
        from_keys = FORWARD_FROM_KEYS and isinstance(presorted, SrcKeys) and presorted.identity and psw is None \
            and mode == _lib.CE_MODE_SUM and num_bags == indices.numel()
        # the ce_*_act entries for every dtype: the kernels store the output as `act` (CE_ACT_F32: the fp32 form)
        act = _lib.ACT_DTYPES[out_dtype]
        if from_keys:
            # one id per bag: out[bag] = W[slot], and the window's keys hold (slot, output row) grouped by slot
            args = (indices.numel(), ptr(presorted.keys), ptr(out), act, stream_ptr())
        else:
            args = (ptr(indices), indices.numel(), ptr(offsets), int(offsets.dtype == torch.int64), num_bags,
                    int(include_last), ptr(psw), mode, hook_features, ptr(out), act, stream_ptr())
        if w16:
            # a 16-bit table: the same two kernels with the row type as a further argument (rows up-converted exactly,
            # fp32 sums, one rounding on the store; from keys with out_dtype == the table's dtype: a bit copy)
            fn = lib.ce_bag_forward_src_keys_w16 if from_keys else lib.ce_bag_forward_w16
            check(fn(ptr(weight), _lib.ACT_DTYPES[weight.dtype], weight.shape[0], dim, *args))
        elif adam:
            # the fp32 kernels with the Adam row type: the w part of every row, the rows three times as far apart
            if fused.layout == "adagrad":
                fn = lib.ce_bag_forward_src_keys_adagrad if from_keys else lib.ce_bag_forward_adagrad
            elif partial:
                fn = lib.ce_bag_forward_src_keys_pradam if from_keys else lib.ce_bag_forward_pradam
            else:
                fn = lib.ce_bag_forward_src_keys_adam if from_keys else lib.ce_bag_forward_adam
            check(fn(ptr(weight), weight.shape[0], dim, *args))
        else:
            fn = lib.ce_bag_forward_src_keys_act if from_keys else lib.ce_bag_forward_act
            check(fn(ptr(weight), weight.shape[0], dim, *args))
        # bwd_scale (scale_grad_by_freq): per-lookup factor of the backward only; it takes the place of psw there
        ctx.save_for_backward(indices, offsets, psw if bwd_scale is None else bwd_scale.contiguous())
        ctx.weight = weight
        ctx.args = (mode, include_last, hook_features, sparse, fused, num_bags)
        ctx.presorted = presorted
        ctx.masked = masked
        return out

    @staticmethod
    def backward(ctx, grad_out):
        indices, offsets, psw = ctx.saved_tensors
        weight = ctx.weight
        mode, include_last, hook_features, sparse, fused, num_bags = ctx.args
        grad_out = grad_out.contiguous()
        adam = isinstance(fused, _IN_ROW)
        if isinstance(fused, FusedAdagrad) and fused.lr is None:
            raise RuntimeError("backward through an Adagrad-layout table with no fused Adagrad set: an autograd gradient "
                               "in slot space over 2 * D columns means nothing (set_fused_adagrad(lr) first, or run the "
                               "forward under torch.no_grad())")
        if adam and fused.lr is None:
            raise RuntimeError("backward through an Adam-layout table with no fused Adam set: an autograd gradient in "
                               f"slot space over {getattr(fused, 'span', 3)} * D columns means nothing (set_fused_adam(lr) first, or run the "
                               "forward under torch.no_grad())")
        dim = weight.shape[1] // fused.span if adam else weight.shape[1]
        off64 = int(offsets.dtype == torch.int64)
        nnz = indices.numel()
        R = weight.shape[0]
        gw = None
        pre = ctx.presorted
        src = isinstance(pre, SrcKeys)
        # the update entries -- the in-row layouts' (Adam, partial row-wise Adam, element-wise Adagrad), row-wise Adagrad,
        # fused SGD -- and the dense gradient read grad_out as it comes (fp32, bf16 or fp16: what autograd delivers for
        # an output of that dtype), from source-row keys or from slots + offsets
        act = _lib.ACT_DTYPES.get(grad_out.dtype)
        if act is None:
            raise NotImplementedError(f"gradient of dtype {grad_out.dtype}: fp32, bf16 and fp16 are implemented")
        update = fused is not None and fused.lr is not None
        rowwise = update and isinstance(fused, FusedRowwiseAdagrad)
        sgd = update and not rowwise and not adam
        # deterministic fp32 SGD without decay or clip (ce_bag_backward_sgd_sorted) and the two sparse=True forms read
        # fp32 only and take the exact upcast of a 16-bit gradient; every other entry reads `act` in place
        clip = (rowwise or sgd) and fused.grad_clip is not None
        fp32_only = (fused.deterministic and fused.weight_decay == 0.0 and not clip) if sgd else \
            (sparse and not rowwise and not adam)
        if fp32_only and act != _lib.CE_ACT_F32:
            grad_out = grad_out.float()
        slots_args = (ptr(indices), nnz, ptr(offsets), off64, num_bags, int(include_last), ptr(psw), mode,
                      hook_features, ptr(grad_out))
        if update:
            # the optimizer's step inside backward: it sees grad=None for the cache parameter
            entry, args = _fused_update_call(fused, weight, dim, slots_args, nnz, grad_out, act, pre)
            with torch.no_grad():
                check(getattr(lib, entry)(*args))
            return (None,) * 14
        if weight.dtype in _lib.W16_DTYPES:
            # a 16-bit table (sparse=True was refused in embedding_bag, before the forward): the dense gradient is
            # accumulated in fp32 and cast once to the parameter's dtype
            g32 = torch.zeros(R, dim, device=weight.device, dtype=torch.float32)
            if src:
                check(lib.ce_bag_backward_dense_src_act(ptr(g32), R, dim, nnz, ptr(grad_out), act, ptr(pre.keys),
                                                        stream_ptr()))
            else:
                check(lib.ce_bag_backward_dense_act(ptr(g32), R, dim, *slots_args, act, ptr(pre), stream_ptr()))
            return (g32.to(weight.dtype),) + (None,) * 13
        if sparse and COALESCED_SPARSE_GRAD and nnz > 0 and not torch.cuda.is_current_stream_capturing():
            # sparse=True (scripts/kaggle.sh:71 --use_sparse_embed_grad): the COO gradient is handed over COALESCED --
            # unique rows (ce_dedupe_bucket_rows), ascending, each with the sum of its lookups' gradient rows (the dense
            # backward kernel over the unique positions) -- so torch.optim.SGD's grad.coalesce() (a sort of every lookup
            # and a segmented sum over nnz x D floats, most of an unchanged trainer's step) has nothing left to do.
            # One host read (the number of unique rows), as coalesce() has too -- which is why a backward that is being
            # captured into a hipGraph takes the one-row-per-lookup form below instead.
            # The dedupe scratch (int32[rows] + int32[2 nnz]; nothing in it needs initialising) comes from the
            # caching allocator per call, so its lifetime is ordered on the stream this backward runs on: two
            # same-sized tables running their backwards on two streams do not share it.
            dev = weight.device
            R = weight.shape[0]
            ws = (torch.empty(R, dtype=torch.int32, device=dev), None,
                  torch.empty(max(2 * nnz, 1 << 16), dtype=torch.int32, device=dev))
            urows = torch.empty(nnz, dtype=torch.int64, device=dev)
            pos = torch.empty(nnz, dtype=torch.int64, device=dev)
            cnt = torch.empty(1, dtype=torch.int64, device=dev)
            check(lib.ce_dedupe_bucket_rows(ptr(indices), nnz, None, R, 1, ptr(ws[0]), ptr(ws[1]), ptr(ws[2]), ptr(urows),
                                            ptr(pos), ptr(cnt), stream_ptr()))
            n_u = int(cnt.item())           # the ONE host sync of this path (torch's coalesce() has the same one)
            folded = torch.zeros(max(n_u, 1), dim, device=dev, dtype=torch.float32)
            if n_u:
                check(lib.ce_bag_backward_dense(ptr(folded), n_u, dim, ptr(pos), nnz, ptr(offsets), off64, num_bags,
                                                int(include_last), ptr(psw), mode, hook_features, ptr(grad_out),
                                                stream_ptr()))
            order = torch.argsort(urows[:n_u])
            gw = torch.sparse_coo_tensor(urows[:n_u][order].view(1, -1), folded[:n_u][order], weight.shape,
                                         is_coalesced=True, check_invariants=False)
        elif sparse:
            rows = torch.empty(nnz, dim, device=weight.device, dtype=torch.float32)
            check(lib.ce_bag_backward_rows(ptr(rows), None, dim, nnz, ptr(offsets), off64, num_bags, int(include_last),
                                           ptr(psw), mode, hook_features, ptr(grad_out), stream_ptr()))
            if ctx.masked:          # lookups masked to -1 (padding_idx): zero contribution at a valid index
                rows = rows * (indices >= 0).unsqueeze(1)
                indices = indices.clamp(min=0)
            gw = torch.sparse_coo_tensor(indices.view(1, -1), rows, weight.shape, check_invariants=False)
        else:
            gw = torch.zeros_like(weight)
            if src:
                check(lib.ce_bag_backward_dense_src_act(ptr(gw), R, dim, nnz, ptr(grad_out), act, ptr(pre.keys),
                                                        stream_ptr()))
            else:
                check(lib.ce_bag_backward_dense_act(ptr(gw), R, dim, *slots_args, act, ptr(pre), stream_ptr()))
        gpsw = None
        if ctx.needs_input_grad[3] and grad_out.dtype != torch.float32:
            grad_out = grad_out.float()              # (off the hot path: ce_bag_backward_psw reads fp32)
        if ctx.needs_input_grad[3]:
            # d loss / d per_sample_weights[j] = <grad_out[bag of j], weight[indices[j]]> (the combination with the
            # fused update was refused in forward)
            gpsw = torch.empty(nnz, device=weight.device, dtype=torch.float32)
            check(lib.ce_bag_backward_psw(ptr(weight), weight.shape[0], dim, ptr(indices), nnz, ptr(offsets), off64,
                                          num_bags, int(include_last), hook_features, ptr(grad_out), ptr(gpsw),
                                          stream_ptr()))
        return gw, None, None, gpsw, None, None, None, None, None, None, None, None, None, None


def _forward_q8(weight, indices, offsets, psw, mode, include_last, hook_features, presorted, out, out_dtype, bits=8):
    """The forward over a row-wise quantized table: weight is [R, 16 + D] uint8 (q8: ce_bag_forward_q8 /
    ce_bag_forward_src_keys_q8) or, with bits=4, [R, 16 + D / 2] uint8 (q4: the _q4 pair).  No autograd node: there is
    no backward, the output never requires grad."""
    _lib.require_gpu()
    assert weight.is_cuda and weight.is_contiguous()
    num_bags = offsets.numel() - 1 if include_last else offsets.numel()
    dim = _quant_dim(weight.shape[1], bits)
    fwd, fwd_keys = (lib.ce_bag_forward_q4, lib.ce_bag_forward_src_keys_q4) if bits == 4 else \
        (lib.ce_bag_forward_q8, lib.ce_bag_forward_src_keys_q8)
    shape = (num_bags // hook_features, hook_features, dim) if hook_features else (num_bags, dim)
    if out is not None:
        if tuple(out.shape) != shape or out.dtype != out_dtype or not out.is_contiguous() or out.device != weight.device:
            raise ValueError(f"out= must be a contiguous {_DTYPE_NAMES[out_dtype]} tensor of shape {shape} on "
                             f"{weight.device}")
    else:
        out = torch.empty(shape, device=weight.device, dtype=out_dtype)
    act = _lib.ACT_DTYPES[out_dtype]
    from_keys = FORWARD_FROM_KEYS and isinstance(presorted, SrcKeys) and presorted.identity and psw is None \
        and mode == _lib.CE_MODE_SUM and num_bags == indices.numel()
    if psw is not None:
        psw = psw.detach()
    if from_keys:
        check(fwd_keys(ptr(weight), weight.shape[0], dim, indices.numel(), ptr(presorted.keys), ptr(out), act,
                       stream_ptr()))
    else:
        check(fwd(ptr(weight), weight.shape[0], dim, ptr(indices), indices.numel(), ptr(offsets),
                  int(offsets.dtype == torch.int64), num_bags, int(include_last), ptr(psw), mode, hook_features, ptr(out),
                  act, stream_ptr()))
    return out


def _quant_dim(width: int, bits: int) -> int:
    """elements of a quantized row that is `width` bytes wide"""
    return 2 * (width - _lib.CE_Q4_HEADER_BYTES) if bits == 4 else width - _lib.CE_Q8_HEADER_BYTES


def _q8_host_src(t: torch.Tensor, bits: int = 8):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in _lib.ACT_DTYPES:
        raise NotImplementedError("quantize_rows takes a 2-D torch.float32, torch.bfloat16 or torch.float16 tensor")
    (_lib.check_q4_dim if bits == 4 else _lib.check_q8_dim)(t.shape[1])
    return t.detach().cpu().contiguous()


def quantize_rows(t: torch.Tensor, threads: int = 0, bits: int = 8) -> torch.Tensor:
    """[N, D] fp32 / bf16 / fp16 rows (any device; quantized on the host) -> [N, 16 + D] uint8 q8 rows on the CPU
    (ce_host_quantize_q8: scale = (max - min) / 255, bias = min, code = rint((x - min) / scale)).  A row holding a NaN
    or an infinity raises (CE_ERR_INVALID names the first one).  Needs no GPU.
    bits=4: [N, 16 + D / 2] uint8 q4 rows (ce_host_quantize_q4: 15 in place of 255, two codes per byte)."""
    src = _q8_host_src(t, _lib.check_quant_bits(bits))
    n, dim = src.shape
    row_bytes, quantize = (_lib.q4_row_bytes, lib.ce_host_quantize_q4) if bits == 4 else \
        (_lib.q8_row_bytes, lib.ce_host_quantize_q8)
    q = torch.empty(n, row_bytes(dim), dtype=torch.uint8)
    check(quantize(ptr(src), _lib.ACT_DTYPES[src.dtype], n, dim, ptr(q), threads or _q8_threads()))
    return q


_NO_BAD_ROW = 2 ** 63 - 1                                   # INT64_MAX: what ce_quantize_rows_* leaves in first_bad


def check_quantize_rows_device(t, bits: int = 8, out=None) -> int:
    """what quantize_rows_device refuses before the GPU is asked for; the width of a quantized row, in bytes"""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in _lib.ACT_DTYPES:
        raise NotImplementedError("quantize_rows_device takes a 2-D torch.float32, torch.bfloat16 or torch.float16 "
                                  "tensor")
    (_lib.check_q4_dim if _lib.check_quant_bits(bits) == 4 else _lib.check_q8_dim)(t.shape[1])
    if t.device.type != "cuda":
        raise ValueError("quantize_rows_device takes rows that are on the GPU (quantize_rows quantizes on the host)")
    width = (_lib.q4_row_bytes if bits == 4 else _lib.q8_row_bytes)(t.shape[1])
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != t.device
                            or tuple(out.shape) != (t.shape[0], width) or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous [{t.shape[0]}, {width}] torch.uint8 tensor on {t.device}")
    return width


def quantize_rows_device(t: torch.Tensor, bits: int = 8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """quantize_rows on the GPU: [n, D] fp32 / bf16 / fp16 rows in device memory -> [n, 16 + D] uint8 q8 rows (bits=4:
    [n, 16 + D / 2] q4 rows) in device memory, byte for byte the rows quantize_rows gives (ce_quantize_rows_q8 / _q4).
    A row holding a NaN or an infinity raises what quantize_rows raises, naming the same row (the first one); the other
    rows of `out` are written by then.  Reads one int64 back, so it waits for the kernel."""
    width = check_quantize_rows_device(t, bits, out)
    src = t.detach().contiguous()
    n, dim = src.shape
    if out is None:
        out = torch.empty(n, width, dtype=torch.uint8, device=src.device)
    if n == 0:
        return out
    first_bad = torch.empty(1, dtype=torch.int64, device=src.device)
    quantize = lib.ce_quantize_rows_q4 if bits == 4 else lib.ce_quantize_rows_q8
    with torch.cuda.device(src.device):
        check(quantize(ptr(src), _lib.ACT_DTYPES[src.dtype], n, dim, ptr(out), ptr(first_bad), stream_ptr()))
        bad = int(first_bad.item())
    if bad != _NO_BAD_ROW:
        raise _lib.CeError(_lib.CE_ERR_INVALID, f"row {bad} holds a NaN or an infinity (or its range overflows fp32): "
                                                "it cannot be quantized")
    return out


def dequantize_rows(q: torch.Tensor, dim: Optional[int] = None, threads: int = 0, bits: int = 8) -> torch.Tensor:
    """[N, 16 + dim] uint8 q8 rows -> [N, dim] fp32 on the CPU: fmaf(code, scale, bias), the value the kernels use.
    bits=4: [N, 16 + dim / 2] uint8 q4 rows (a uint8 tensor's width cannot tell the two apart)."""
    name = "q4" if _lib.check_quant_bits(bits) == 4 else "q8"
    row_bytes, dequantize = (_lib.q4_row_bytes, lib.ce_host_dequantize_q4) if bits == 4 else \
        (_lib.q8_row_bytes, lib.ce_host_dequantize_q8)
    if not isinstance(q, torch.Tensor) or q.dim() != 2 or q.dtype != _lib.Q8:
        raise NotImplementedError(f"dequantize_rows takes a 2-D torch.uint8 tensor of {name} rows")
    if dim is None:
        dim = _quant_dim(q.shape[1], bits)
    if q.shape[1] != row_bytes(dim):
        raise ValueError(f"{name} rows of dim {dim} are {row_bytes(dim)} bytes wide (got {q.shape[1]})")
    src = q.detach().cpu().contiguous()
    out = torch.empty(src.shape[0], dim, dtype=torch.float32)
    check(dequantize(ptr(src), src.shape[0], dim, ptr(out), threads or _q8_threads()))
    return out


def _q8_threads() -> int:
    return int(lib.ce_cpu_budget())


def check_lr(lr):
    """What a fused update's learning rate may be: None (the update is off), a number, or a tensor of ONE fp32 element,
    contiguous, that does not require grad.  The tensor is kept by reference and never read on the host: the kernels
    read it when they run (the ce_*_lrdev entries), so a fill_ / copy_ before a step -- or before the replay of a
    hipGraph that captured the step -- is the learning rate of that step.  Its device is checked against the weight in
    embedding_bag, before the forward.  Host logic only; nothing here looks at the value."""
    if isinstance(lr, torch.Tensor):
        if lr.dtype != torch.float32:
            raise TypeError(f"a tensor learning rate must be torch.float32 (got {lr.dtype})")
        if lr.numel() != 1:
            raise ValueError(f"a tensor learning rate must have one element (got {lr.numel()})")
        if lr.requires_grad:
            raise ValueError("a tensor learning rate must not require grad")
        if not lr.is_contiguous():
            raise ValueError("a tensor learning rate must be contiguous")
    return lr


def _at_least_0(name: str, value) -> float:
    if not float(value) >= 0.0:
        raise ValueError(f"{name}={value!r}: must be >= 0")
    return float(value)


# the in-row layouts' entries, ce_bag_backward_<stem>[_src]<suffix> and ce_bag_backward_<stem>_sorted: the suffix by what
# the list holds behind eps -- 0: nothing, 1: the decay, 2: the decay and the clip -- and the least the layout's lists hold
_IN_ROW_ENTRIES = {"adam": ("adam", ("", "_wd", "_clip"), 0),
                   "partial_rowwise_adam": ("pradam", (None, "", "_clip"), 1),
                   "adagrad": ("adagrad", (None, None, ""), 2)}
# the ce_bag_backward_update_* entries that walk keys, by what they take beyond the plain list: (from slots + offsets,
# from source-row keys)
_UPDATE_ENTRIES = {"clip": ("ce_bag_backward_update_clip", "ce_bag_backward_update_src_clip"),
                   "wd": ("ce_bag_backward_update_wd", "ce_bag_backward_update_src_wd"),
                   "lrdev": ("ce_bag_backward_update_lrdev", "ce_bag_backward_update_src_lrdev"),
                   "compact": ("ce_bag_backward_update_compact", "ce_bag_backward_update_compact_src"),
                   "w16": ("ce_bag_backward_update_w16", "ce_bag_backward_update_src_w16")}


def _decay(fused) -> tuple:
    """weight_decay, weight_decay_mode as the lists that hold a decay take them"""
    return (float(fused.weight_decay), WEIGHT_DECAY_MODES[fused.weight_decay_mode])


def _fused_update_call(fused, weight, dim: int, slots: tuple, nnz: int, grad_out, act: int, pre) -> tuple:
    """The one place that says which C entry applies `fused` (a switch whose lr is set) inside the backward, with which
    arguments and on which workspace: (entry, args) -- a name of _lib.SIGNATURES and its complete positional list.
    slots: the slots + offsets lookups up to grad_out; act: grad_out's CE_ACT_*; pre: None, presorted keys or SrcKeys.
    A list is made of groups, each written once and in the order every list has them (_lib.py declares the same ones):
        table | lookups (`walk`: slots + offsets, or source-row keys) and act | keys | row state | moments | rate |
        decay | clip | optimizer, rounding, seed | step | accumulator | workspace, its bytes, stream
    tests/golden/update_dispatch.json pins every list."""
    R, dev = weight.shape[0], weight.device
    src = isinstance(pre, SrcKeys)
    # the lookups as the entry walks them, with the dtype of grad_out; the keys behind them (a sorted entry takes slots +
    # offsets and no keys, whatever `pre` is)
    walk = (nnz, ptr(grad_out), act) if src else (*slots, act)
    keys = ptr(pre.keys) if src else ptr(pre)
    # the rate.  lr: a float, or -- the ce_*_lrdev entries -- the address of ONE fp32 in device memory that the kernels
    # read when they run; lr_both: `lr, lr_dev` of the entries that take it both ways, the other one 0 / NULL.  What a
    # tensor learning rate does not go with was refused before the forward.
    lr_dev = isinstance(fused.lr, torch.Tensor)
    lr = ptr(fused.lr) if lr_dev else float(fused.lr)
    lr_both = (0.0, lr) if lr_dev else (lr, None)
    clip = fused.grad_clip is not None
    decay = clip or fused.weight_decay != 0.0
    if isinstance(fused, _IN_ROW):
        # one fold, then one apply pass over the rows the step looked up; the step count lives on the device.  The
        # workspace follows fused.accumulator: _ws ("cache"), _ws_step ("step") or _ws_sorted ("sorted")
        stem, suffixes, least = _IN_ROW_ENTRIES[fused.layout]
        by_sort = fused.accumulator == "sorted"
        holds = 2 if by_sort else max(least, 2 if clip else 1 if decay else 0)
        ws = fused.workspace(R, nnz, dim, dev)
        # (partial row-wise Adam: the second moment, one fp32 per table row, is named like row-wise Adagrad's momentum)
        state = ()
        if fused.layout == "partial_rowwise_adam":
            state = (ptr(fused.row_of_slot), ptr(fused.exp_avg_sq), fused.exp_avg_sq.numel())
        moments = (float(fused.lr_decay),) if fused.layout == "adagrad" else (float(fused.betas[0]), float(fused.betas[1]))
        decay_part = _decay(fused) if holds >= 1 else ()
        clip_part = () if holds < 2 else fused.clip_args() if clip else (0.0, _lib.CE_CLIP_NONE)
        if by_sort:
            return f"ce_bag_backward_{stem}_sorted", \
                (ptr(weight), R, dim, *slots, act, *state, *moments, *lr_both, float(fused.eps), *decay_part, *clip_part,
                 ptr(fused.step), ptr(ws), ws.numel(), stream_ptr())
        return f"ce_bag_backward_{stem}{'_src' if src else ''}{suffixes[holds]}", \
            (ptr(weight), R, dim, *walk, keys, *state, *moments, *lr_both, float(fused.eps), *decay_part, *clip_part,
             ptr(fused.step), _lib.CE_ACC_STEP if fused.accumulator == "step" else _lib.CE_ACC_CACHE,
             ptr(ws), ws.numel(), stream_ptr())
    rowwise = isinstance(fused, FusedRowwiseAdagrad)
    w16 = weight.dtype in _lib.W16_DTYPES
    by_step = fused.accumulator == "step"
    if not (rowwise or w16 or decay or by_step):
        # fused SGD on an fp32 table folds straight into the rows (K13 + K14 in one pass): no row state, no accumulator
        if fused.deterministic:
            ws = fused.workspace(R, nnz, dev)
            return "ce_bag_backward_sgd_sorted", (ptr(weight), R, dim, *slots, lr, ptr(ws), ws.numel(), stream_ptr())
        if src:
            return "ce_bag_backward_sgd_src_lrdev" if lr_dev else "ce_bag_backward_sgd_src_act", \
                (ptr(weight), R, dim, *walk, lr, keys, ptr(pre.ranges), stream_ptr())
        return "ce_bag_backward_sgd_lrdev" if lr_dev else "ce_bag_backward_sgd_act", \
            (ptr(weight), R, dim, *walk, lr, keys, stream_ptr())
    # row-wise Adagrad, and SGD where it has a per-row pass.  The workspace first: the
    # sorted fold's arrays, the step-sized accumulator, or the cache-sized one of the table's dtype
    if fused.deterministic:
        ws = _workspace_sorted(fused, R, nnz, dim, dev)
    elif by_step:
        ws = fused.workspace_step(R, nnz, dim, dev)
    else:
        ws = fused.workspace_w16(R, dim, dev) if w16 else fused.workspace(R, dim, dev)
    mom = fused.momentum if rowwise else None
    state = (ptr(fused.row_of_slot), ptr(mom), 0 if mom is None else mom.numel())
    eps = float(fused.eps) if rowwise else 0.0
    # what the call needs beyond the plain list picks the entry: a clip, a decay, the learning rate from device memory,
    # the step-sized accumulator, a 16-bit table
    kind = "clip" if clip else "wd" if decay else "" if fused.deterministic else "lrdev" if lr_dev else \
        "compact" if by_step else "w16" if w16 else None
    if kind is None:
        # exact row-wise Adagrad on an fp32 table, cache-sized accumulator, lr by value: the first pair, the short list
        return "ce_bag_backward_rowwise_adagrad_src_act" if src else "ce_bag_backward_rowwise_adagrad_act", \
            (ptr(weight), R, dim, *walk, keys, *state, lr, eps, ptr(ws), ws.numel(), stream_ptr())
    table = (ptr(weight), _lib.ACT_DTYPES[weight.dtype], R, dim)
    # an fp32 table is never rounded, whatever fused.rounding says (the plain sorted entry is handed it as it is set)
    stochastic = fused.rounding == "stochastic" and (w16 or kind == "")
    optimizer = (_lib.CE_OPT_ROWWISE_ADAGRAD if rowwise else _lib.CE_OPT_SGD,
                 _lib.CE_ROUND_STOCHASTIC if stochastic else _lib.CE_ROUND_NEAREST, int(fused.seed) & (2 ** 64 - 1))
    decay_part = _decay(fused) if decay else ()
    clip_part = fused.clip_args() if clip else ()
    if fused.deterministic:
        # bit-reproducible, no accumulator: ce_bag_backward_update_sorted[_wd | _clip], the learning rate a float
        return "ce_bag_backward_update_sorted" + (kind and "_" + kind), \
            (*table, *slots, act, *state, lr, eps, *decay_part, *clip_part, *optimizer, ptr(ws), ws.numel(), stream_ptr())
    # the _wd / _clip lists take the learning rate both ways; they and the _lrdev list say which accumulator `ws` is
    rate = (*lr_both, eps) if decay else (lr, eps)
    acc = (_lib.CE_ACC_STEP if by_step else _lib.CE_ACC_CACHE,) if decay or lr_dev else ()
    return _UPDATE_ENTRIES[kind][src], \
        (*table, *walk, keys, *state, *rate, *decay_part, *clip_part, *optimizer, *acc, ptr(ws), ws.numel(), stream_ptr())


_DTYPE_NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


# forward from the window's source-row keys when they were built for the one-id-per-bag layout (False: always the
# gather-shaped kernel over slots + offsets); sparse=True hands torch a coalesced COO gradient (False: one value row per
# lookup).  Module constants (they were environment switches until round 6): a test or a probe may set them.
FORWARD_FROM_KEYS = True
COALESCED_SPARSE_GRAD = True


class _BagMaxFn(torch.autograd.Function):
    """mode='max' (ce_bag_forward_max / ce_bag_backward_max): dense gradient or the fused SGD update."""

    @staticmethod
    def forward(ctx, weight, indices, offsets, include_last, hook_features, fused):
        _lib.require_gpu()
        assert weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous()
        num_bags = offsets.numel() - 1 if include_last else offsets.numel()
        dim = weight.shape[1]
        shape = (num_bags // hook_features, hook_features, dim) if hook_features else (num_bags, dim)
        out = torch.empty(shape, device=weight.device, dtype=torch.float32)
        pos = torch.empty(num_bags, dim, device=weight.device, dtype=torch.int32)
        check(lib.ce_bag_forward_max(ptr(weight), weight.shape[0], dim, ptr(indices), indices.numel(), ptr(offsets),
                                     int(offsets.dtype == torch.int64), num_bags, int(include_last), hook_features,
                                     ptr(out), ptr(pos), stream_ptr()))
        ctx.save_for_backward(indices, pos)
        ctx.weight = weight
        ctx.args = (num_bags, hook_features, fused)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        indices, pos = ctx.saved_tensors
        weight = ctx.weight
        num_bags, hook_features, fused = ctx.args
        grad_out = grad_out.contiguous()
        dim = weight.shape[1]
        if fused is not None and fused.lr is not None:
            with torch.no_grad():
                check(lib.ce_bag_backward_max(ptr(weight), weight.shape[0], dim, ptr(indices), indices.numel(), num_bags,
                                              hook_features, ptr(grad_out), ptr(pos), -float(fused.lr), stream_ptr()))
            return None, None, None, None, None, None
        gw = torch.zeros_like(weight)
        check(lib.ce_bag_backward_max(ptr(gw), weight.shape[0], dim, ptr(indices), indices.numel(), num_bags,
                                      hook_features, ptr(grad_out), ptr(pos), 1.0, stream_ptr()))
        return gw, None, None, None, None, None


def renorm_rows_(weight: torch.Tensor, indices: torch.Tensor, max_norm: float, norm_type: float = 2.0) -> None:
    """torch.embedding_renorm_ on the rows `indices` names (out-of-range entries are skipped), in place."""
    assert weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous()
    idx = indices.reshape(-1).long().contiguous()
    ws = torch.empty(lib.ce_rows_renorm_workspace(weight.shape[0]), dtype=torch.uint8, device=weight.device)
    with torch.no_grad():
        check(lib.ce_rows_renorm(ptr(weight), weight.shape[0], weight.shape[1], ptr(idx), idx.numel(), float(max_norm),
                                 float(norm_type), ptr(ws), ws.numel(), stream_ptr()))


def _cached_bytes(self, attr: str, need: int, device, zero: bool) -> torch.Tensor:
    """the byte buffer kept in self.<attr>: reused while it holds `need` bytes on `device`, else dropped BEFORE its
    successor is allocated -- zero-filled (for kernels that leave it zero-filled again) or uninitialised"""
    ws = getattr(self, attr)
    if ws is not None and ws.numel() >= need and ws.device == device:
        return ws
    del ws
    setattr(self, attr, None)
    setattr(self, attr, (torch.zeros if zero else torch.empty)(need, dtype=torch.uint8, device=device))
    return getattr(self, attr)


def _workspace_w16(self, num_rows: int, dim: int, device) -> torch.Tensor:
    """workspace of the 16-bit table's update (fp32 accumulator [num_rows, dim] -- twice the 16-bit rows it serves --,
    byte flags, the step counter): zero-filled once; every call leaves it zero-filled except the counter"""
    return _cached_bytes(self, "_ws16", lib.ce_bag_backward_w16_workspace(num_rows, dim), device, zero=True)


ACCUMULATORS = ("cache", "step")
# the in-row layouts (FusedAdam, FusedAdagrad) also take "sorted": the deterministic fold, which has no accumulator
# 
IN_ROW_ACCUMULATORS = ACCUMULATORS + ("sorted",)


def check_accumulator(optimizer: str, table_dtype, accumulator: str, deterministic: bool = False,
                      rounding: str = "nearest") -> None:
    """Refusals of accumulator= ("cache": the fp32 accumulator of the atomic updates has a row per row of the weight;
    "step": a row per lookup of the step at most).  optimizer: "sgd" or "rowwise_adagrad"; table_dtype: the weight's
    (None: not known yet -- what depends on it is asked again before the forward).
    Host logic only -- it is asked before the forward, so that nothing is refused after a kernel has run."""
    if accumulator not in ACCUMULATORS:
        raise ValueError(f"accumulator={accumulator!r}: 'cache' or 'step'")
    if accumulator == "cache":
        return
    if deterministic:
        raise NotImplementedError("accumulator='step' with deterministic=True: the sorted update has no accumulator")
    w16 = table_dtype in _lib.W16_DTYPES
    if optimizer == "sgd" and table_dtype is not None and not w16:
        raise NotImplementedError("accumulator='step' with fused SGD on an fp32 table: that update folds straight "
                                  "into the rows and has no accumulator")
    if optimizer == "rowwise_adagrad" and w16 and rounding == "stochastic":
        raise NotImplementedError("accumulator='step' with row-wise Adagrad and rounding='stochastic' on a 16-bit "
                                  "table (set rounding='nearest')")


def _workspace_step(self, num_rows: int, nnz: int, dim: int, device) -> torch.Tensor:
    """workspace of accumulator="step" (step counter, byte flags, fp32 accumulator [min(nnz, num_rows), dim], the
    compaction's arrays): zero-filled once; every call leaves it zero-filled except the counter and what needs no
    initialising.  Its layout belongs to one (num_rows, nnz, dim): for another one it is zero-filled again, the
    counter -- the first 8 bytes -- kept, so stochastic rounding goes on drawing fresh bits."""
    need = lib.ce_bag_backward_update_compact_workspace(num_rows, nnz, dim)
    key = (int(num_rows), int(nnz), int(dim))
    ws = self._ws_step
    if ws is None or ws.numel() < need or ws.device != device:
        counter = None if ws is None or ws.device != device else ws[:8].clone()
        self._ws_step = ws = None                       # (the old one goes before the new one comes)
        self._ws_step = ws = torch.zeros(need, dtype=torch.uint8, device=device)
        if counter is not None:
            ws[:8].copy_(counter)
    elif self._ws_step_key != key:
        ws[256:].zero_()
    self._ws_step_key = key
    return ws


def check_lr_path(lr, deterministic: bool, mode: Optional[str] = None) -> None:
    """Refusals of a tensor learning rate that do not depend on the weight: the sorted, deterministic updates and
    mode='max' take a float only.  Host logic only, asked before the forward."""
    if not isinstance(lr, torch.Tensor):
        return
    if deterministic:
        raise NotImplementedError("a tensor learning rate with deterministic=True: the sorted updates take a float")
    if mode == "max":
        raise NotImplementedError("a tensor learning rate with mode='max'")


WEIGHT_DECAY_MODES = {"l2": _lib.CE_WD_L2, "decoupled": _lib.CE_WD_DECOUPLED}


def check_weight_decay(weight_decay, weight_decay_mode) -> float:
    """weight_decay: a number >= 0 (a negative or NaN one is a ValueError); weight_decay_mode: "l2" (the decay joins the
    gradient: torch.optim.{SGD, Adagrad, Adam}(weight_decay=), FBGEMM's L2) or "decoupled" (the row is scaled by
    1 - lr * weight_decay first: torch.optim.AdamW, FBGEMM's DECOUPLE).  Returns the decay as a float."""
    if weight_decay_mode not in WEIGHT_DECAY_MODES:
        raise ValueError(f"weight_decay_mode={weight_decay_mode!r}: 'l2' or 'decoupled'")
    if isinstance(weight_decay, torch.Tensor):
        raise ValueError("weight_decay is a float: only the learning rate may live in device memory")
    return _at_least_0("weight_decay", weight_decay)


def _refuse_per_row_path(what: str, does: str, optimizer: str, table_dtype, deterministic: bool, lr, mode) -> None:
    """The decay and the clip both need the update's per-row pass: what either of them, switched on, is refused for.
    what: "weight_decay" or "grad_clip"; does: what the pass would do with a row."""
    if mode == "max":
        raise NotImplementedError(f"{what} with mode='max': that update has no per-row pass")
    if isinstance(lr, torch.Tensor) and deterministic:
        raise NotImplementedError(f"{what} with a tensor learning rate and deterministic=True: the sorted updates "
                                  "take a float")
    if optimizer == "sgd" and table_dtype == torch.float32 and not deterministic:
        raise NotImplementedError(f"{what} with fused SGD on an fp32 table: the atomic scatter has no per-row pass "
                                  f"that could {does} -- set deterministic=True (the sorted update)")


def _refuse_owner_side(what: str, lacks: str, who: str) -> None:
    raise NotImplementedError(f"{what} is not implemented for {who}: its owner-side update is ce_rows_axpy, "
                              f"which has no per-row {lacks}")


def check_weight_decay_path(optimizer: str, table_dtype, weight_decay: float, deterministic: bool = False, lr=None,
                            mode: Optional[str] = None) -> None:
    """Refusals of weight_decay != 0 (optimizer: "sgd", "rowwise_adagrad" or "adam"; table_dtype: the weight's, None:
    not known yet -- what depends on it is asked again before the forward).  Host logic only -- it is asked before the
    forward, so that nothing is refused after a kernel has run."""
    if weight_decay:
        _refuse_per_row_path("weight_decay", "decay a row once", optimizer, table_dtype, deterministic, lr, mode)


def refuse_weight_decay(who: Optional[str], weight_decay) -> None:
    """the sharded and table-wise modules: their owner-side update is ce_rows_axpy, which has no decay"""
    if who and weight_decay:
        _refuse_owner_side("weight_decay", "decay", who)


def _workspace_in_row_sorted(self, num_rows: int, nnz: int, dim: int, device) -> torch.Tensor:
    """workspace of ce_bag_backward_adam_sorted / _pradam_sorted / _adagrad_sorted (sort arrays, one partial row per
    lookup): nothing in it needs initialising"""
    need = lib.ce_bag_backward_in_row_sorted_workspace(num_rows, nnz, dim)
    return _cached_bytes(self, "_ws_sorted", need, device, zero=False)


def _workspace_sorted(self, num_rows: int, nnz: int, dim: int, device) -> torch.Tensor:
    """workspace of ce_bag_backward_update_sorted* (sort arrays, partial rows): nothing in it needs initialising"""
    need = lib.ce_bag_backward_update_sorted_workspace(num_rows, nnz, dim)
    return _cached_bytes(self, "_ws_sorted", need, device, zero=False)


GRAD_CLIP_MODES = ("value", "row_norm")
_GRAD_CLIP_CODES = {"value": _lib.CE_CLIP_VALUE, "row_norm": _lib.CE_CLIP_ROW_NORM}


def check_grad_clip(grad_clip, grad_clip_mode) -> Optional[float]:
    """grad_clip: None (no clipping) or a number > 0, +inf included (a tensor, zero, a negative one or a NaN is a
    ValueError); grad_clip_mode: "value" (every element of a row's folded gradient is clamped to [-grad_clip, grad_clip]:
    torch.nn.utils.clip_grad_value_) or "row_norm" (a row's folded gradient is scaled by grad_clip / (its 2-norm + 1e-6)
    where that is below 1: clip_grad_norm_ with every row its own parameter).  Returns the threshold as a float, or
    None."""
    if grad_clip_mode not in GRAD_CLIP_MODES:
        raise ValueError(f"grad_clip_mode={grad_clip_mode!r}: 'value' or 'row_norm'")
    if grad_clip is None:
        return None
    if isinstance(grad_clip, torch.Tensor):
        raise ValueError("grad_clip is a float: only the learning rate may live in device memory")
    c = float(grad_clip)
    if not c > 0.0:
        raise ValueError(f"grad_clip={grad_clip!r}: must be > 0 (None: no clipping)")
    return c


def check_grad_clip_path(optimizer: str, table_dtype, grad_clip: Optional[float], deterministic: bool = False, lr=None,
                         mode: Optional[str] = None) -> None:
    """Refusals of grad_clip is not None: those of check_weight_decay_path, for the same reasons (the clip needs the
    per-row pass the decay needs).  Host logic only -- it is asked before the forward, so that nothing is refused
    after a kernel has run."""
    if grad_clip is not None:
        _refuse_per_row_path("grad_clip", "clip a row's folded gradient", optimizer, table_dtype, deterministic, lr, mode)


def refuse_grad_clip(who: Optional[str], grad_clip) -> None:
    """the sharded and table-wise modules: their owner-side update is ce_rows_axpy, which has no clip"""
    if who and grad_clip is not None:
        _refuse_owner_side("grad_clip", "clip", who)


class _FusedSwitch:
    """What the four switches share.  `optimizer`: the name the check_* functions know the switch by.  `lr`: check_lr
    runs on every assignment, a direct one included.  `weight_decay` / `weight_decay_mode` and `grad_clip` /
    `grad_clip_mode` are checked on every set_weight_decay / set_grad_clip; the clip acts on a
    row's folded gradient of the step before everything else reads it -- the decay, the sums of squares, the moments, the
    step.  The workspaces (the workspace* methods fill the slots a switch uses) start out empty."""
    optimizer: str
    weight_decay, weight_decay_mode = 0.0, "l2"
    grad_clip, grad_clip_mode = None, "value"
    _ws = _ws16 = _ws_step = _ws_step_key = _ws_sorted = None

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        self._lr = check_lr(value)

    def set_weight_decay(self, weight_decay: float = 0.0, weight_decay_mode: str = "l2") -> None:
        self.weight_decay = check_weight_decay(weight_decay, weight_decay_mode)
        self.weight_decay_mode = weight_decay_mode

    def set_grad_clip(self, grad_clip: Optional[float] = None, grad_clip_mode: str = "value") -> None:
        self.grad_clip = check_grad_clip(grad_clip, grad_clip_mode)
        self.grad_clip_mode = grad_clip_mode

    def clip_args(self) -> tuple:
        """(grad_clip, grad_clip_mode) as the ce_*_clip entries take them"""
        return (float(self.grad_clip), _GRAD_CLIP_CODES[self.grad_clip_mode])

    def _init_by_accumulator(self, lr, deterministic: bool, accumulator: str, weight_decay, weight_decay_mode,
                             grad_clip, grad_clip_mode) -> None:
        """FusedSGD's and FusedRowwiseAdagrad's constructors: what they refuse while the table is not known yet"""
        check_accumulator(self.optimizer, None, accumulator, deterministic)
        check_lr_path(check_lr(lr), deterministic)
        self.set_weight_decay(weight_decay, weight_decay_mode)
        check_weight_decay_path(self.optimizer, None, self.weight_decay, deterministic, lr)
        self.set_grad_clip(grad_clip, grad_clip_mode)
        check_grad_clip_path(self.optimizer, None, self.grad_clip, deterministic, lr)
        self.lr, self.accumulator = lr, accumulator

    workspace_w16 = _workspace_w16
    workspace_step = _workspace_step


class FusedSGD(_FusedSwitch):
    """Switch for the fused backward+SGD path of one embedding module.

    lr=None disables fusion (the module behaves exactly like nn.EmbeddingBag under
    torch.optim.SGD); deterministic=True uses the sorted segmented update instead of atomics.
    accumulator="step" (a 16-bit table only; an fp32 table's SGD has no accumulator): the update's fp32 accumulator has
    min(lookups of the step, rows) rows instead of one per row of the weight.
    lr may be a tensor (check_lr): one fp32 element on the weight's device, kept by reference and read by the kernels
    when they run -- rewrite it in place (fill_ / copy_) between steps or between replays of a captured step.  Not
    with deterministic=True and not with mode='max'.
    weight_decay, weight_decay_mode ("l2": w -= lr (g + wd w); "decoupled": w = w (1 - lr wd) - lr g), lazy: the rows a
    step looks up decay once, in that step.  A 16-bit table with either accumulator; an fp32 table
    with deterministic=True only (the atomic scatter has no per-row pass); not with mode='max'.
    grad_clip, grad_clip_mode ("value" / "row_norm"; check_grad_clip): the row's folded gradient is
    clipped before the decay and the step see it.  Where the decay is taken, and nowhere else."""
    optimizer = "sgd"

    def __init__(self, lr: Union[float, torch.Tensor, None] = None, deterministic: bool = False,
                 accumulator: str = "cache", *, weight_decay: float = 0.0, weight_decay_mode: str = "l2",
                 grad_clip: Optional[float] = None, grad_clip_mode: str = "value"):
        self._init_by_accumulator(lr, bool(deterministic), accumulator, weight_decay, weight_decay_mode, grad_clip,
                                  grad_clip_mode)
        self.deterministic = deterministic
        # a 16-bit table only: how the update rounds a row ("nearest" / "stochastic"), the seed of the random bits and
        # the host-table row of every slot they are drawn for (None: the slot itself)
        self.rounding, self.seed, self.row_of_slot = "stochastic", 0, None

    def workspace(self, num_rows: int, nnz: int, device) -> torch.Tensor:
        return _cached_bytes(self, "_ws", lib.ce_bag_backward_sgd_sorted_workspace(num_rows, nnz), device, zero=False)


class FusedRowwiseAdagrad(_FusedSwitch):
    """Switch for the fused backward + exact row-wise Adagrad update of one embedding module (FBGEMM's
    EXACT_ROWWISE_ADAGRAD; weight_decay_mode "l2" / "decoupled" are its L2 / DECOUPLE).  Per step and per UNIQUE row r the step looks up, with g the sum of the
    row's gradient rows in the batch:  m[r] += sum(g * g) / D ;  W[r] -= lr * g / (sqrt(m[r]) + eps).

    momentum: fp32 [rows] on the device -- one accumulator per row of the table the momentum follows; row_of_slot:
    int32 [rows of the weight] mapping a row of the weight the kernels update to its momentum index (a cache's
    cached_idx_map), None = the weight row itself.  lr=None disables the update (the weight then gets a gradient).

    deterministic=True: the step's lookups are sorted by row and a row's gradient is folded in lookup order (in chunks of
    CE_SORTED_CHUNK for a hot row, the partial sums added in chunk order) instead of by atomics -- bit-reproducible
    from run to run and independent of which slot a row sits in.  It needs no [rows, D] accumulator: its workspace
    grows with the lookups of a step, not with the table.  A 16-bit table is rounded to nearest on this path: set
    rounding = "nearest" (the default, "stochastic", is a NotImplementedError there before any kernel runs).

    accumulator="step": the atomic update keeps its speed but folds into an fp32 accumulator of min(lookups of the
    step, rows) rows -- the flagged slots are compacted and the lookups renumbered first -- instead of one as large as
    the weight ("cache", the default).  Not with deterministic=True, and on a 16-bit table with rounding="nearest"
    only: both are refused before any kernel runs.

    lr may be a tensor, as for FusedSGD (check_lr); not with deterministic=True.

    weight_decay, weight_decay_mode, lazy (the rows a step looks up decay once, in that step):
    "l2": h = g + weight_decay * w takes the place of g everywhere, in sum(h * h) / D too; "decoupled": w is scaled by
    1 - lr * weight_decay first.  Every path above takes it.

    grad_clip, grad_clip_mode ("value" / "row_norm"; check_grad_clip): g is clipped first, and the
    decay's h, sum(h * h) / D and the step all see the clipped g.  Every path above takes it."""
    optimizer = "rowwise_adagrad"

    def __init__(self, lr: Union[float, torch.Tensor, None] = None, eps: float = 1e-8,
                 momentum: Optional[torch.Tensor] = None, row_of_slot: Optional[torch.Tensor] = None,
                 deterministic: bool = False, accumulator: str = "cache", *, weight_decay: float = 0.0,
                 weight_decay_mode: str = "l2", grad_clip: Optional[float] = None, grad_clip_mode: str = "value"):
        self._init_by_accumulator(lr, bool(deterministic), accumulator, weight_decay, weight_decay_mode, grad_clip,
                                  grad_clip_mode)
        self.deterministic = bool(deterministic)
        self.eps = float(eps)
        self.momentum = momentum
        self.row_of_slot = row_of_slot
        self.rounding, self.seed = "stochastic", 0          # a 16-bit table only (see FusedSGD)

    def check(self, weight: torch.Tensor) -> None:
        """refusals that must come before any kernel of the step has run"""
        m = self.momentum
        if m is None or not m.is_cuda or m.dtype != torch.float32 or not m.is_contiguous() or m.device != weight.device:
            raise ValueError("row-wise Adagrad needs a contiguous fp32 momentum tensor on the weight's device")
        rmap = self.row_of_slot
        if rmap is None:
            if m.numel() < weight.shape[0]:
                raise ValueError("momentum must have a row for every row of the weight")
        elif rmap.numel() != weight.shape[0]:
            # a cache with rows behind it (CachedParamMgr.reserve_tail: the row-wise exchange's received rows) would
            # hand the backward slots outside [0, C), which have no row of the table and so no state
            raise NotImplementedError("fused row-wise Adagrad updates the cache rows only: slots outside [0, C) "
                                      f"(a weight of {weight.shape[0]} rows over a cache of {rmap.numel()})")
        elif rmap.dtype != torch.int32 or not rmap.is_contiguous() or rmap.device != weight.device:
            raise ValueError("row_of_slot must be a contiguous int32 tensor on the weight's device")

    workspace_sorted = _workspace_sorted         # the deterministic path (sort arrays, partial rows)

    def workspace(self, num_rows: int, dim: int, device) -> torch.Tensor:
        # zero-filled once; every call of the kernels leaves it zero-filled again
        need = lib.ce_bag_backward_rowwise_adagrad_workspace(num_rows, dim)
        return _cached_bytes(self, "_ws", need, device, zero=True)


class _InRowSwitch(_FusedSwitch):
    """What FusedAdam and FusedAdagrad share: the table's rows carry the optimizer's state behind their w part (`span`
    parts of D floats, `layout` says which), the step count is one int64 on the device, and the accumulator -- "sorted"
    is the deterministic fold here -- picks the workspace."""
    deterministic = False                                   # (the sorted fold is accumulator="sorted" here)
    rounding, seed = "nearest", 0
    _name: str                                              # "Adam" / "Adagrad", as the refusals spell it
    _cache_workspace: str                                   # the library's size function of accumulator="cache"

    def _set_head(self, deterministic: bool, weight_decay, weight_decay_mode, grad_clip, grad_clip_mode) -> tuple:
        """how every set() begins: the checked (decay, clip), and deterministic=True refused"""
        wd = check_weight_decay(weight_decay, weight_decay_mode)
        clip = check_grad_clip(grad_clip, grad_clip_mode)
        if deterministic:
            raise NotImplementedError(f"fused {self._name} with deterministic=True: the deterministic (sorted) fold of "
                                      f"an {self._name}-layout table is accumulator='sorted'")
        return wd, clip

    def _set_tail(self, accumulator: str, wd: float, weight_decay_mode: str, clip, grad_clip_mode: str) -> None:
        """how every set() ends: the last check, then the first store -- a refused set() changes nothing"""
        if accumulator not in IN_ROW_ACCUMULATORS:
            raise ValueError(f"accumulator={accumulator!r}: 'cache', 'step' or 'sorted'")
        self.accumulator = accumulator
        self.weight_decay, self.weight_decay_mode = wd, weight_decay_mode
        self.grad_clip, self.grad_clip_mode = clip, grad_clip_mode

    def check(self, weight: torch.Tensor) -> None:
        """refusals that must come before any kernel of the step has run"""
        if weight.dtype != torch.float32 or weight.dim() != 2 or weight.shape[1] % self.span != 0:
            raise NotImplementedError(f"Fused{self._name} needs an fp32 weight of {self._name}-layout rows, [rows, "
                                      f"{self.span} * embedding_dim] (got {tuple(weight.shape)} {weight.dtype})")
        _lib.check_adam_dim(weight.shape[1] // self.span)
        if self.lr is None:
            return
        if not isinstance(self.lr, torch.Tensor):
            _at_least_0("lr", self.lr)
        st = self.step
        if st is None or not st.is_cuda or st.dtype != torch.int64 or st.numel() != 1 or st.device != weight.device:
            raise ValueError(f"fused {self._name} needs its step count: one int64 element on the weight's device")
        if self.layout == "partial_rowwise_adam":
            self.check_row_state(weight)                    # (FusedAdam's own)

    def workspace(self, num_rows: int, nnz: int, dim: int, device) -> torch.Tensor:
        # zero-filled once; every call of the kernels leaves what must be zero zero-filled again ("sorted": nothing
        # in it needs initialising)
        if self.accumulator == "sorted":
            return _workspace_in_row_sorted(self, num_rows, nnz, dim, device)
        if self.accumulator == "step":
            return _workspace_step(self, num_rows, nnz, dim, device)
        need = getattr(lib, self._cache_workspace)(num_rows, nnz, dim, _lib.CE_ACC_CACHE)
        return _cached_bytes(self, "_ws", need, device, zero=True)


# the switches that say the weight's rows carry optimizer state behind their w part (span parts of D floats)
_IN_ROW = _InRowSwitch


class FusedAdam(_InRowSwitch):
    """Switch for the fused backward + Adam update of one embedding module whose table carries its moments: the weight
    the kernels see is [rows, 3 * D] fp32, every row w | m | v.  torch.optim.SparseAdam's arithmetic,
    per step and per UNIQUE row the step looks up, g the sum of the row's gradient rows in the batch, t the step count:
        m += (1 - beta1) (g - m) ;  v += (1 - beta2) (g g - v) ;
        w -= lr sqrt(1 - beta2^t) / (1 - beta1^t) * m / (sqrt(v) + eps)
    Rows no lookup names keep all three parts.  Handing this object to embedding_bag is what says the weight has the
    layout, so the forward needs it too; lr=None leaves the forward working and makes a backward a RuntimeError.

    step: ONE int64 on the weight's device, zero before the first step; the first kernel of every backward adds 1 to it
    (a replayed graph counts on).  accumulator: "step" (the default: an fp32 accumulator of min(lookups of the step,
    rows) rows), "cache" (one row per row of the weight) or "sorted" (no accumulator and no atomics -- the
    step's lookups are sorted by slot and a row's gradient is folded in lookup order, so two runs of a job agree bit for
    bit; presorted keys are not needed and ignored).  lr may be a tensor, as for FusedSGD (check_lr), "sorted" included.

    weight_decay, weight_decay_mode, lazy like the moments (the rows a step looks up decay once, in that step):
    "l2" is torch.optim.Adam(weight_decay=) -- g + weight_decay * w feeds both moments --, "decoupled" torch.optim.AdamW
    -- w is scaled by 1 - lr * weight_decay (lr, not the bias-corrected step size) first.

    grad_clip, grad_clip_mode ("value" / "row_norm"; check_grad_clip): g is clipped first -- the decay
    and both moments see the clipped g --, as clip_grad_value_ / a per-row clip_grad_norm_ before optimizer.step().

    layout="partial_rowwise_adam" (FBGEMM's PARTIAL_ROWWISE_ADAM): the weight is [rows, 2 * D], every row
    w | m, and the second moment is ONE fp32 per table row -- exp_avg_sq, [v_rows] fp32 on the weight's device, indexed by
    row_of_slot[slot] (int32 [rows]; None: by slot), as FusedRowwiseAdagrad's momentum is:
        v[r] += (1 - beta2) (mean_d (g_d g_d) - v[r]) ;  w -= lr c_t * m / (sqrt(v[r]) + eps)
    A slot whose row_of_slot lies outside [0, v_rows) is left alone."""
    optimizer, _name, _cache_workspace = "adam", "Adam", "ce_bag_backward_adam_workspace"

    def __init__(self, lr: Union[float, torch.Tensor, None] = None, betas=(0.9, 0.999), eps: float = 1e-8,
                 accumulator: str = "step", step: Optional[torch.Tensor] = None, deterministic: bool = False, *,
                 weight_decay: float = 0.0, weight_decay_mode: str = "l2", layout: str = "adam",
                 exp_avg_sq: Optional[torch.Tensor] = None, row_of_slot: Optional[torch.Tensor] = None,
                 grad_clip: Optional[float] = None, grad_clip_mode: str = "value"):
        if layout not in ("adam", "partial_rowwise_adam"):
            raise ValueError(f"layout={layout!r}: 'adam' or 'partial_rowwise_adam'")
        self.layout, self.span = layout, _lib.LAYOUT_SPAN[layout]
        self.exp_avg_sq, self.row_of_slot = exp_avg_sq, row_of_slot        # (the partial layout only)
        self.lr = lr
        self.set(betas, eps, accumulator, deterministic, weight_decay=weight_decay, weight_decay_mode=weight_decay_mode,
                 grad_clip=grad_clip, grad_clip_mode=grad_clip_mode)
        self.step = step

    def set(self, betas, eps: float, accumulator: str, deterministic: bool = False, *, weight_decay: float = 0.0,
            weight_decay_mode: str = "l2", grad_clip: Optional[float] = None, grad_clip_mode: str = "value") -> None:
        wd, clip = self._set_head(deterministic, weight_decay, weight_decay_mode, grad_clip, grad_clip_mode)
        b1, b2 = (float(b) for b in betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas={tuple(betas)!r}: both must lie in [0, 1)")
        eps = _at_least_0("eps", eps)
        self._set_tail(accumulator, wd, weight_decay_mode, clip, grad_clip_mode)
        self.betas, self.eps = (b1, b2), eps

    def check_row_state(self, weight: torch.Tensor) -> None:
        """the partial layout's part of check(): the per-row second moment and its map"""
        v, ros = self.exp_avg_sq, self.row_of_slot
        if v is None or v.dtype != torch.float32 or v.device != weight.device or not v.is_contiguous() or \
                v.numel() == 0:
            raise ValueError("partial row-wise Adam needs exp_avg_sq: a contiguous fp32 tensor, one element per "
                             "table row, on the weight's device")
        if ros is not None and (ros.dtype != torch.int32 or ros.device != weight.device or not ros.is_contiguous()
                                or ros.numel() < weight.shape[0]):
            raise ValueError("row_of_slot: a contiguous int32 tensor of one element per row of the weight, on its "
                             "device")


class FusedAdagrad(_InRowSwitch):
    """Switch for the fused backward + element-wise Adagrad update (torch.optim.Adagrad; FBGEMM's EXACT_ADAGRAD) of one
    embedding module whose table carries its state: the weight the kernels see is [rows, 2 * D] fp32, every row w | h, h
    the per-element sums of squared gradients.  Per step and per UNIQUE row the step looks up, g the sum
    of the row's gradient rows in the batch, t the step count:
        clr = lr / (1 + (t - 1) lr_decay) ;  h += g g ;  w -= clr * g / (sqrt(h) + eps)
    Rows no lookup names keep both parts.  FusedRowwiseAdagrad keeps ONE sum per row and is an approximation of this.
    Handing this object to embedding_bag is what says the weight has the layout, so the forward needs it too; lr=None
    leaves the forward working and makes a backward a RuntimeError.  The defaults are torch.optim.Adagrad's.

    step, accumulator ("sorted" included: the deterministic fold) and a tensor lr: as for FusedAdam -- the step count is ONE int64 on the weight's device which the
    first kernel of every backward adds 1 to, so a replayed graph follows it, and a tensor lr, in clr.

    weight_decay, weight_decay_mode, lazy (the rows a step looks up decay once, in that step): "l2" is
    torch.optim.Adagrad(weight_decay=) -- g + weight_decay * w takes the place of g --, "decoupled" scales w by
    1 - clr * weight_decay first.  grad_clip, grad_clip_mode (check_grad_clip): g is clipped first."""

    optimizer, _name, _cache_workspace = "adagrad", "Adagrad", "ce_bag_backward_adagrad_workspace"
    layout, span = "adagrad", 2

    def __init__(self, lr: Union[float, torch.Tensor, None] = None, eps: float = 1e-10, lr_decay: float = 0.0,
                 accumulator: str = "step", step: Optional[torch.Tensor] = None, *, weight_decay: float = 0.0,
                 weight_decay_mode: str = "l2", grad_clip: Optional[float] = None, grad_clip_mode: str = "value",
                 deterministic: bool = False):
        self.lr = lr
        self.set(eps, lr_decay, accumulator, deterministic, weight_decay=weight_decay,
                 weight_decay_mode=weight_decay_mode, grad_clip=grad_clip, grad_clip_mode=grad_clip_mode)
        self.step = step

    def set(self, eps: float, lr_decay: float, accumulator: str, deterministic: bool = False, *,
            weight_decay: float = 0.0, weight_decay_mode: str = "l2", grad_clip: Optional[float] = None,
            grad_clip_mode: str = "value") -> None:
        wd, clip = self._set_head(deterministic, weight_decay, weight_decay_mode, grad_clip, grad_clip_mode)
        eps, lr_decay = _at_least_0("eps", eps), _at_least_0("lr_decay", lr_decay)
        self._set_tail(accumulator, wd, weight_decay_mode, clip, grad_clip_mode)
        self.eps, self.lr_decay = eps, lr_decay


def _refuse_for_table(table: str, mode, max_norm, sparse, per_sample_weights, more=()) -> None:
    """What only a plain fp32 table takes: mode='max', max_norm, sparse=True, and -- listed last -- a gradient w.r.t.
    per_sample_weights.  table: how the refusal names the table; more: the table kind's own rows, (what, is it on)."""
    what = "mode='max'" if mode == "max" else "max_norm" if max_norm is not None else "sparse=True" if sparse else None
    for row, on in more:
        if on and what is None:
            what = row
    if what is None and per_sample_weights is not None and per_sample_weights.requires_grad and torch.is_grad_enabled():
        what = "a gradient w.r.t. per_sample_weights"
    if what is not None:
        raise NotImplementedError(f"{what} with {table}")


def _check_lr_device(lr: torch.Tensor, weight) -> None:
    if lr.device != weight.device:
        raise ValueError(f"the learning-rate tensor is on {lr.device}, the weight on {weight.device}: the kernels read "
                         "it from device memory")


def check_front(fused, weight: torch.Tensor, mode: str, max_norm, sparse, per_sample_weights, output_dtype,
                quant_bits: int = 8):
    """Everything embedding_bag refuses for its switch and its table, before any kernel has run -- a refusal inside
    backward would leave the caller with an exception AND an updated table.  Host logic only.  Returns the output dtype
    the call resolves to.  Of two refusals the earlier stage wins (DESIGN.md 3.18 lists the stages and says where a new
    optimizer adds its rows); a switch is asked again here because its fields and the weight can change after it was
    built or set."""
    _lib.act_code(output_dtype)
    update = fused is not None and fused.lr is not None
    in_row = isinstance(fused, _IN_ROW)
    if in_row:
        # the switch is what says the rows carry state: [R, 3 * D] w | m | v, or [R, 2 * D] w | m or w | h
        fused.check(weight)
        _refuse_for_table(f"an {fused._name}-layout table", mode, max_norm, sparse, per_sample_weights)
        if isinstance(fused.lr, torch.Tensor):
            _check_lr_device(check_lr(fused.lr), weight)
    if weight.dtype == _lib.Q8:
        # a row-wise quantized table ([R, 16 + D] uint8 q8 rows, or [R, 16 + D / 2] q4 rows with quant_bits=4): forward
        # only, the output defaults to fp32
        name = "q4 (torch.quint4x2)" if _lib.check_quant_bits(quant_bits) == 4 else "q8 (torch.uint8)"
        if weight.dim() != 2:
            raise ValueError(f"a {name} weight is a [rows, 16 + embedding_dim{' / 2' if quant_bits == 4 else ''}] tensor")
        (_lib.check_q4_dim if quant_bits == 4 else _lib.check_q8_dim)(_quant_dim(weight.shape[1], quant_bits))
        _refuse_for_table(f"a {name} table: it is forward only", mode, max_norm, sparse, per_sample_weights,
                          (("a fused SGD / row-wise Adagrad update (a quantized table is never updated)", update),))
    elif update and not in_row:
        # fused SGD and row-wise Adagrad: what depends on the table's dtype and on the mode
        det = bool(fused.deterministic)
        check_accumulator(fused.optimizer, weight.dtype, fused.accumulator, det, fused.rounding)
        if fused.accumulator == "step" and mode == "max":
            raise NotImplementedError("accumulator='step' with mode='max'")
        check_weight_decay_path(fused.optimizer, weight.dtype, fused.weight_decay, det, fused.lr, mode)
        check_grad_clip_path(fused.optimizer, weight.dtype, fused.grad_clip, det, fused.lr, mode)
        if isinstance(fused.lr, torch.Tensor):
            check_lr_path(check_lr(fused.lr), det, mode)
            _check_lr_device(fused.lr, weight)
    if weight.dtype in _lib.W16_DTYPES:
        # a 16-bit table (bf16 / fp16 weight): rows up-converted exactly, fp32 sums, the output defaults to the
        # weight's dtype
        _lib.check_w16_dim(weight.shape[1])
        sorted16 = update and fused.deterministic and fused.optimizer
        _refuse_for_table(f"a 16-bit table ({weight.dtype})", mode, max_norm, sparse, per_sample_weights,
                          (("FusedSGD(deterministic=True)", sorted16 == "sgd"),
                           ("FusedRowwiseAdagrad(deterministic=True) with rounding='stochastic' (set rounding='nearest')",
                            sorted16 == "rowwise_adagrad" and fused.rounding == "stochastic")))
        if output_dtype is None:
            output_dtype = weight.dtype
    if mode not in _MODES and mode != "max":
        raise NotImplementedError(f"mode={mode!r}: 'sum', 'mean' and 'max' are implemented")
    if update and fused.optimizer == "rowwise_adagrad":
        if mode == "max":
            raise NotImplementedError("fused row-wise Adagrad with mode='max'")
        fused.check(weight)
    return torch.float32 if output_dtype is None else output_dtype


def embedding_bag(indices: torch.Tensor, weight: torch.Tensor, offsets: Optional[torch.Tensor] = None,
                  max_norm: Optional[float] = None, norm_type: float = 2.0, scale_grad_by_freq: bool = False,
                  mode: str = "mean", sparse: bool = False, per_sample_weights: Optional[torch.Tensor] = None,
                  include_last_offset: bool = False, padding_idx: Optional[int] = None, *,
                  hook_features: int = 0, fused_sgd: Union[FusedSGD, FusedRowwiseAdagrad, FusedAdam, FusedAdagrad, None] = None,
                  presorted: Union[torch.Tensor, SrcKeys, None] = None, masked_indices: bool = False,
                  out: Optional[torch.Tensor] = None, output_dtype: Optional[torch.dtype] = None,
                  quant_bits: int = 8) -> torch.Tensor:
    # quant_bits: looked at for a torch.uint8 weight only -- 8: q8 rows [R, 16 + D]; 4: q4 rows [R, 16 + D / 2] (a uint8
    # tensor's width cannot tell the two apart)
    # out: write the pooled output into this tensor (contiguous, of the output dtype and the shape the call would
    # allocate) and return it --
    # a static output buffer for steps replayed from a hipGraph, possibly one chosen by pick_fast_buffer
    # output_dtype: None / torch.float32 (the default), torch.bfloat16 or torch.float16 -- the dtype of the pooled output
    # and hence of the gradient autograd hands back; the weight, the sums and every update stay fp32, the kernels
    # round once on the store and read the 16-bit gradient in place.  out= must then have that dtype.
    output_dtype = check_front(fused_sgd, weight, mode, max_norm, sparse, per_sample_weights, output_dtype, quant_bits)
    q8 = weight.dtype == _lib.Q8
    # masked_indices: the caller already replaced ignored lookups (padding) by -1 -- the kernels skip them; the
    # sparse=True backward then parks their (zero) gradient rows at index 0 so the COO tensor stays valid
    if per_sample_weights is not None:
        if mode != "sum":
            raise NotImplementedError("embedding_bag: per_sample_weights was not None. per_sample_weights is "
                                      f"only supported for mode='sum' (got mode='{mode}').")
        if per_sample_weights.dtype != torch.float32 or not per_sample_weights.is_contiguous() or \
                per_sample_weights.dim() != 1:
            per_sample_weights = per_sample_weights.reshape(-1).float().contiguous()     # (keeps the autograd link)
    indices, offsets, include_last_offset, num_bags = _prep(indices, offsets, include_last_offset)
    if max_norm is not None:
        # F.embedding_bag renormalises the rows the input names, in place, before it looks them up
        renorm_rows_(weight.detach(), indices, max_norm, norm_type)
    if mode == "max":
        # torch: no per_sample_weights (above), no sparse gradient, no scale_grad_by_freq for 'max'
        if sparse:
            raise RuntimeError("embedding_bag: sparse gradients are not supported with mode='max'")
        if scale_grad_by_freq:
            raise RuntimeError("embedding_bag: scale_grad_by_freq is not supported with mode='max'")
        if presorted is not None:
            raise NotImplementedError("presorted keys serve the sum / mean backward only")
        if hook_features and num_bags % hook_features:
            raise ValueError("hook_features must divide the number of bags")
        if padding_idx is not None:
            if padding_idx < 0:
                padding_idx += weight.shape[0]
            indices = torch.where(indices == padding_idx, torch.full_like(indices, -1), indices)
        if out is not None:
            raise NotImplementedError("out= with mode='max'")
        res = _BagMaxFn.apply(weight, indices, offsets, bool(include_last_offset), int(hook_features), fused_sgd)
        # (off the hot path: the fp32 kernel and one cast behind it; autograd upcasts the gradient on the way back)
        return res if output_dtype == torch.float32 else res.to(output_dtype)
    if per_sample_weights is not None and per_sample_weights.numel() != indices.numel():
        raise ValueError("per_sample_weights must have the same number of elements as input")
    bwd_scale = None
    if mode == "mean" and (padding_idx is not None or masked_indices or scale_grad_by_freq):
        # 'mean' over the NON-padding entries of a bag (torch excludes padding from the sum and from the count), and
        # 'mean' with scale_grad_by_freq: the kernels' mean divides by the bag length, so these run as a 'sum' with
        # per-lookup weights 1 / (valid entries of the bag) -- a handful of torch ops, off the benchmarked path
        if presorted is not None:
            raise NotImplementedError("padding_idx / scale_grad_by_freq with mode='mean' cannot be combined with "
                                      "presorted keys")
        if padding_idx is not None:
            pi = padding_idx + weight.shape[0] if padding_idx < 0 else padding_idx
            indices = torch.where(indices == pi, torch.full_like(indices, -1), indices)
            padding_idx = None
            masked_indices = True
        nnz = indices.numel()
        ends = offsets[1:] if include_last_offset else torch.cat(
            [offsets[1:], torch.full((1,), nnz, dtype=offsets.dtype, device=offsets.device)])
        lens = (ends - offsets[:num_bags]).long()
        bag_of = torch.repeat_interleave(torch.arange(num_bags, device=indices.device), lens, output_size=nnz)
        valid = ((indices >= 0) & (indices < weight.shape[0])).to(torch.float32)
        cnt = torch.zeros(num_bags, device=indices.device, dtype=torch.float32).index_add_(0, bag_of, valid)
        per_sample_weights = valid / cnt.clamp_(min=1.0)[bag_of]
        mode = "sum"
    if scale_grad_by_freq:
        # torch: the gradient of a row is divided by the number of times the row occurs in the mini-batch
        if mode != "sum":
            raise NotImplementedError("scale_grad_by_freq is implemented for mode='sum' and 'mean'")
        if presorted is not None:
            raise NotImplementedError("scale_grad_by_freq cannot be combined with presorted keys")
        _, inv, cnt = torch.unique(indices, return_inverse=True, return_counts=True)
        bwd_scale = (1.0 / cnt.to(torch.float32))[inv]
        if per_sample_weights is not None:
            bwd_scale = bwd_scale * per_sample_weights
    if padding_idx is not None:
        # entries equal to padding_idx take no part in the reduction and receive no gradient: the kernels skip
        # out-of-range rows, so they are redirected to -1
        if mode != "sum":
            raise NotImplementedError("padding_idx is implemented for mode='sum' only (mean would need the "
                                      "per-bag count of non-padding entries)")
        if presorted is not None:
            # the keys hold the rows they were built from: mask the slots BEFORE presort_window instead
            raise NotImplementedError("padding_idx cannot be combined with presorted keys (mask the indices to -1 "
                                      "before building the keys)")
        if padding_idx < 0:
            padding_idx += weight.shape[0]
        indices = torch.where(indices == padding_idx, torch.full_like(indices, -1), indices)
    if hook_features and num_bags % hook_features:
        raise ValueError("hook_features must divide the number of bags")
    if isinstance(presorted, SrcKeys):
        if mode != "sum" or per_sample_weights is not None:
            raise ValueError("source-row keys (presort_window(..., offsets=...)) hold no per-lookup scale: they "
                             "need mode='sum' without per_sample_weights")
        if (presorted.num_bags, bool(presorted.include_last_offset), int(presorted.hook_features)) != \
                (num_bags, bool(include_last_offset), int(hook_features)):
            raise ValueError("source-row keys were built for another bag layout "
                             f"{tuple(presorted[1:4])} than this call's {(num_bags, include_last_offset, hook_features)}")
        k = presorted.keys
        if presorted.ranges is not None:
            r = presorted.ranges
            assert r.is_cuda and r.dtype == torch.int64 and r.is_contiguous() and \
                r.numel() == 2 * (k.numel() // 16384), "ranges must come from presort_window(..., ids=...)"
        assert k.is_cuda and k.dtype == torch.int64 and k.is_contiguous() and \
            k.numel() == lib.ce_bag_presort_len(indices.numel()), "keys must come from presort_window"
    elif presorted is not None:
        assert presorted.is_cuda and presorted.dtype == torch.int64 and presorted.is_contiguous() and \
            presorted.numel() == lib.ce_bag_presort_len(indices.numel()), "presorted must come from presort_slots"
    if masked_indices and mode != "sum":
        raise NotImplementedError("masked (padding) lookups are implemented for mode='sum' only (mean would need "
                                  "the per-bag count of non-padding entries)")
    if q8:
        return _forward_q8(weight, indices, offsets, per_sample_weights, _MODES[mode], bool(include_last_offset),
                           int(hook_features), presorted, out, output_dtype, quant_bits)
    return _BagFn.apply(weight, indices, offsets, per_sample_weights, _MODES[mode], bool(include_last_offset),
                        int(hook_features), bool(sparse), fused_sgd, presorted, bwd_scale,
                        padding_idx is not None or bool(masked_indices), None if out is None else [out], output_dtype)


def probe_rows(buf: torch.Tensor, fold: int, reps: int = 6):
    """(us per pass of row stores, us per pass of row loads) over buf [rows, dim] visited `fold` rows apart
    (ce_probe_rows); buf's contents are overwritten"""
    import ctypes
    assert buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous()
    flat = buf.view(-1, buf.shape[-1])
    w, r = ctypes.c_double(), ctypes.c_double()
    check(lib.ce_probe_rows(ptr(flat), flat.shape[0], flat.shape[1], int(fold), int(reps), ctypes.byref(w), ctypes.byref(r),
                            stream_ptr()))
    return w.value, r.value


def _time_work(work, buf: torch.Tensor, reps: int) -> float:
    """us per call of work(buf): `reps` calls enqueued while the GPU is kept busy by a spin kernel (so that they run
    back to back however long the host takes to launch them), timed by two events.  Deliberately NOT a captured
    hipGraph: two dozen capture / destroy cycles leave the runtime with a different assignment of streams to hardware
    queues for everything created afterwards (measured: a prefetch_num = 1 pipeline built after them ran 5 % slower)."""
    work(buf)                                    # once, untimed: lazy initialisation, first-touch of the candidate
    torch.cuda.synchronize(buf.device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(int(6e5) * reps)           # ~0.3 ms per call at 2 GHz: room for an autograd step's host time
    e0.record()
    for _ in range(reps):
        work(buf)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def pick_fast_buffer(shape, device, fold: int, candidates: int = 5, use: str = "write", work=None, reps: int = 8):
    """A contiguous fp32 tensor of `shape` ([..., D]) that is FAST for the hook-folded access pattern: rows visited
    `fold` rows apart, every row on another page -- what the forward's stores into a [B, F, D] output (fold = F) and the
    streaming backward's loads of the upstream gradient do.  How fast depends on how the allocation happens to be
    mapped, not on its address: the same forward launch takes 38 or 45 us on two buffers of one process
    (profiles/r05_alloc_lottery.txt), which is also why the same bench line differed by 15 % in its forward between
    processes.  So: allocate `candidates` buffers, time each, keep the fastest, give the others back.
    use = "write" (an output buffer) or "read" (a gradient buffer): what is timed is the pattern alone (ce_probe_rows,
    a few passes; the search stops at the first candidate clearly of the fast kind).  work = callable(buf): what is
    timed is the caller's own work on the candidate instead -- work(buf) enqueues it on the current stream, free of
    side effects; `reps` calls run back to back behind a spin kernel -- and every candidate is tried ("read"
    candidates are zero-filled first: a gradient buffer must not hold the allocator's leftovers).
    Returns (tensor, {"us": [...], "picked": i}).  For static buffers of graph-captured steps; torch decides where
    everything else lives."""
    assert use in ("write", "read")
    bufs, us, fresh = [], [], []
    for _ in range(max(1, int(candidates))):
        r0 = torch.cuda.memory_reserved(device)
        b = torch.empty(shape, dtype=torch.float32, device=device)       # (all candidates stay alive while the search runs:
        bufs.append(b)                                                  # every one is another allocation)
        fresh.append(int(torch.cuda.memory_reserved(device) > r0))
        if work is not None:
            if use == "read":
                b.zero_()
            us.append(_time_work(work, b, reps))
            continue
        w, r = probe_rows(b, fold)
        us.append(w if use == "write" else r)
        if len(us) >= 4:
            med = sorted(us)[len(us) // 2]
            if us[-1] < 0.94 * med:          # the fast kind is ~8 % faster than the common kind in this probe: found one
                break
    best = min(range(len(bufs)), key=lambda i: us[i])
    keep = bufs[best]
    del bufs, b
    # the losers go back to the DRIVER, not into torch's cache: whatever is allocated next would otherwise be carved
    # out of them (measured: a window object built after a 12-candidate search ran 7 % slower at prefetch_num = 1)
    torch.cuda.empty_cache()
    return keep, {"us": [round(u, 2) for u in us], "picked": best, "new_segment": fresh}


def is_identity_layout(offsets: torch.Tensor, include_last_offset: bool) -> bool:
    """True when the offsets describe one id per bag, in order (offsets == arange): ONE host comparison, meant for
    set-up time of a pipeline whose batches all share these offsets."""
    if offsets.dim() != 1:
        return False
    n = offsets.numel()
    return bool(torch.equal(offsets.long(), torch.arange(n, device=offsets.device)))


def presort_len(n: int) -> int:
    """elements of the key tensor presort_slots writes for n lookups (n rounded up to whole 16384-lookup segments)"""
    return int(lib.ce_bag_presort_len(int(n)))


def presort_slots(slots: torch.Tensor, num_rows: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Segment-sorted keys of one batch's slots for the fused backward (ce_bag_presort): int64 tensor holding the
    bits of uint64 keys, presort_len(n) long.  Run it once per prefetch window on the cache-op stream, then pass
    the batch's keys to embedding_bag(presorted=...)."""
    flat = slots.reshape(-1).contiguous()
    if out is None:
        out = torch.empty(presort_len(flat.numel()), dtype=torch.int64, device=flat.device)
    assert out.dtype == torch.int64 and out.numel() == presort_len(flat.numel()) and out.is_contiguous()
    check(lib.ce_bag_presort(ptr(flat), flat.numel(), int(num_rows), ptr(out), stream_ptr()))
    return out


def presort_window(slots: torch.Tensor, num_rows: int, keys_out: Optional[torch.Tensor] = None, *,
                   offsets: Optional[torch.Tensor] = None, include_last_offset: bool = False,
                   hook_features: int = 0, ids: Optional[torch.Tensor] = None,
                   ranges_out: Optional[torch.Tensor] = None, identity_bags: bool = False):
    """Grouped keys for the P equal-sized batches of a prefetch window in one launch (ce_bag_presort_window).
    slots: [P, n] int64 (the cache op's output) -> keys [P, presort_len(n)]; row b is what
    embedding_bag(presorted=...) takes for batch b.

    offsets given (1-D: shared by the batches, or [P, len]: one row per batch): source-row keys
    (ce_bag_presort_window_src) for mode='sum' without per-sample weights -- returns a list of P SrcKeys instead,
    which the backward streams over without touching offsets or indices again.  The keys ARE the batch as far as the
    backward is concerned: pass them only to the embedding_bag call that uses the same slots and the same offsets
    (the bag layout is checked, the contents cannot be).

    ids given as well ([P, n] int64: the ids `slots` was computed from, position by position): the keys also mark the
    rows a single lane group of the backward owns, and every SrcKeys carries the id range of its segments
    (ce_bag_presort_window_src_excl) -- the fused-SGD backward then updates those rows without atomics.

    identity_bags=True: the caller has checked that `offsets` is arange(n + 1) -- one id per bag, in order, what every
    Criteo / Avazu batch is (is_identity_layout) -- so the kernel need not read the offsets to establish it."""
    assert slots.dim() == 2 and slots.is_contiguous() and slots.dtype == torch.int64
    P, n = slots.shape
    klen = presort_len(n)
    if keys_out is None:
        keys_out = torch.empty(P, klen, dtype=torch.int64, device=slots.device)
    assert keys_out.is_contiguous() and keys_out.numel() == P * klen and keys_out.dtype == torch.int64
    if offsets is None:
        check(lib.ce_bag_presort_window(ptr(slots), n, P, int(num_rows), ptr(keys_out), stream_ptr()))
        return keys_out.view(P, klen)
    assert offsets.is_cuda and offsets.dtype in (torch.int32, torch.int64) and offsets.is_contiguous()
    assert offsets.dim() == 1 or (offsets.dim() == 2 and offsets.shape[0] == P)
    per = offsets.shape[-1]
    num_bags = per - 1 if include_last_offset else per
    if hook_features and num_bags % hook_features:
        raise ValueError("hook_features must divide the number of bags")
    kv = keys_out.view(P, klen)
    if identity_bags:
        assert num_bags == n, "identity_bags needs one id per bag"
    off_ptr = None if identity_bags else ptr(offsets)
    if ids is None:
        check(lib.ce_bag_presort_window_src(ptr(slots), n, P, int(num_rows), off_ptr,
                                            int(offsets.dtype == torch.int64), per if offsets.dim() == 2 else 0,
                                            num_bags, int(include_last_offset), int(hook_features), ptr(keys_out),
                                            stream_ptr()))
        return [SrcKeys(kv[b], num_bags, bool(include_last_offset), int(hook_features), None, bool(identity_bags))
                for b in range(P)]
    assert ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == P * n
    segs = klen // 16384
    if ranges_out is None:
        ranges_out = torch.empty(P, segs, 2, dtype=torch.int64, device=slots.device)
    assert ranges_out.is_contiguous() and ranges_out.dtype == torch.int64 and ranges_out.numel() == P * segs * 2
    check(lib.ce_bag_presort_window_src_excl(ptr(slots), n, P, int(num_rows), off_ptr,
                                             int(offsets.dtype == torch.int64), per if offsets.dim() == 2 else 0,
                                             num_bags, int(include_last_offset), int(hook_features), ptr(ids),
                                             ptr(keys_out), ptr(ranges_out), stream_ptr()))
    rv = ranges_out.view(P, segs, 2)
    return [SrcKeys(kv[b], num_bags, bool(include_last_offset), int(hook_features), rv[b], bool(identity_bags))
            for b in range(P)]
