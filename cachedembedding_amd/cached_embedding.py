"""CachedEmbeddingBag: nn.EmbeddingBag-compatible module whose table lives in pinned host
DRAM with a frequency-aware cache of hot rows in HBM.

Drop-in for ``colossalai.nn.parallel.layers.CachedEmbeddingBag`` as the reference uses it
(benchmark/benchmark_cache.py:39-40,62; benchmark/benchmark_fbgemm_uvm.py:98-105,148);
constructor order and forward signature per SURVEY.md 8(b) / Appendix A.7.
"""
from __future__ import annotations

from typing import Callable, Iterator, List, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import _lib
from .cache_mgr import CachedParamMgr, EvictionStrategy, HostTable
from .functional import (FusedAdagrad, FusedAdam, FusedRowwiseAdagrad, FusedSGD, _at_least_0, _refuse_for_table,
                         check_accumulator, check_grad_clip, check_grad_clip_path, check_lr, check_lr_path,
                         check_weight_decay, check_weight_decay_path, embedding_bag, quantize_rows_device,
                         refuse_grad_clip, refuse_weight_decay)


def _checked_decay_and_clip(module, optimizer: str, lr, deterministic: bool, weight_decay, weight_decay_mode, grad_clip,
                            grad_clip_mode) -> tuple:
    """the checked decay (a float) and clip (a float or None) of a set_fused_* call, with everything they are refused
    for known at that point; the module's table and mode are looked at only for one that is switched on"""
    who = getattr(module, "_no_weight_decay", None)
    wd = check_weight_decay(weight_decay, weight_decay_mode)
    refuse_weight_decay(who, wd)
    if lr is not None and wd:
        check_weight_decay_path(optimizer, module.table_dtype, wd, bool(deterministic), lr, module.mode)
    clip = check_grad_clip(grad_clip, grad_clip_mode)
    refuse_grad_clip(who, clip)
    if lr is not None and clip is not None:
        check_grad_clip_path(optimizer, module.table_dtype, clip, bool(deterministic), lr, module.mode)
    return wd, clip


def _checked_by_accumulator(module, setter: str, optimizer: str, lr, deterministic, accumulator: str, *decay_and_clip):
    """what set_fused_sgd and set_fused_rowwise_adagrad refuse alike, in this order; the checked (decay, clip)"""
    _refuse_q8_update(module, setter, lr)
    _refuse_adam_layout(module, setter, lr)
    checked = _checked_decay_and_clip(module, optimizer, lr, deterministic, *decay_and_clip)
    if isinstance(lr, torch.Tensor):                       # (a float or None: nothing new is looked at)
        check_lr_path(check_lr(lr), bool(deterministic), module.mode)
    if lr is not None or accumulator != "step":            # (an unknown value is refused whatever lr is)
        check_accumulator(optimizer, module.table_dtype, accumulator, bool(deterministic), module.weight_rounding)
    return checked


def _checked_in_row(module, optimizer: str, lr, *per_row) -> tuple:
    """what set_fused_adam and set_fused_adagrad refuse alike behind their layout check; the checked (decay, clip)"""
    if isinstance(lr, torch.Tensor):
        check_lr(lr)
    elif lr is not None:
        _at_least_0("lr", lr)
    return _checked_decay_and_clip(module, optimizer, lr, False, *per_row)


def _set_by_accumulator(switch, lr, deterministic, accumulator: str, wd, weight_decay_mode, clip, grad_clip_mode):
    switch.lr = lr
    switch.deterministic = deterministic
    switch.accumulator = accumulator
    switch.set_weight_decay(wd, weight_decay_mode)
    switch.set_grad_clip(clip, grad_clip_mode)


def _refuse_q8_update(module, what: str, lr) -> None:
    if lr is not None and getattr(module, "table_dtype", None) == _lib.Q8:
        raise NotImplementedError(f"{what}(lr) with a q8 (torch.uint8) table: a quantized table is never updated")
    if lr is not None and getattr(module, "table_dtype", None) == _lib.Q4:
        raise NotImplementedError(f"{what}(lr) with a q4 (torch.quint4x2) table: a quantized table is never updated")


def _refuse_adam_layout(module, what: str, lr) -> None:
    layout = getattr(module, "fused_optimizer", None)
    if lr is not None and layout == "adagrad":
        raise NotImplementedError(f"{what}(lr) on an Adagrad-layout module (fused_optimizer={layout!r}): its rows carry "
                                  "Adagrad's sums of squares, set_fused_adagrad(lr) is its fused update")
    if lr is not None and layout is not None:
        raise NotImplementedError(f"{what}(lr) on an Adam-layout module (fused_optimizer={layout!r}): its rows carry "
                                  "Adam's moments, set_fused_adam(lr) is its fused update")


def _quant_name(bits: int) -> str:
    return "q4 (torch.quint4x2)" if bits == 4 else "q8 (torch.uint8)"


def _refuse_sharded(module, what: str) -> None:
    """refresh_rows / current_rows are a single-process module's: one message for world_size > 1 and for a module that a
    sharded class owns (the table-wise class names itself in its shard modules' _no_weight_decay; they have no
    world_size of their own).  The column-wise class on ONE rank is a single-process module, as for quantized()."""
    who = getattr(module, "_no_weight_decay", None)
    world = getattr(module, "world_size", None)
    if (world or 1) > 1 or (who is not None and world is None):
        raise NotImplementedError(f"{what} on {who or type(module).__name__} ({world or 1} rank"
                                  f"{'s' if (world or 1) != 1 else ''}): rows are refreshed in, and read from, a "
                                  "single-process CachedEmbeddingBag")


def _check_row_ids(what: str, ids) -> None:
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or ids.dtype != torch.int64:
        raise ValueError(f"{what} takes ids as a 1-D torch.int64 tensor")


def _check_refresh_rows(module, ids, rows) -> None:
    """what refresh_rows refuses before the GPU is asked for (rows=None: refresh_from, whose rows current_rows makes)"""
    layout = getattr(module, "fused_optimizer", None)
    if layout is not None:
        raise NotImplementedError(f"refresh_rows on an in-row layout (fused_optimizer={layout!r}): a row there is weights "
                                  "plus optimizer state, and new weights alone do not make one")
    _refuse_sharded(module, "refresh_rows")
    _check_row_ids("refresh_rows", ids)
    if rows is None:
        return
    if not isinstance(rows, torch.Tensor) or rows.dtype not in _lib.ACT_DTYPES:
        raise NotImplementedError("refresh_rows takes rows as a torch.float32, torch.bfloat16 or torch.float16 tensor")
    if rows.dim() != 2 or tuple(rows.shape) != (ids.numel(), module.embedding_dim):
        raise ValueError(f"refresh_rows needs [{ids.numel()}, {module.embedding_dim}] rows for {ids.numel()} ids of a "
                         f"table with embedding_dim={module.embedding_dim} (got {tuple(rows.shape)})")


def _check_current_rows(module, ids) -> None:
    _lib.refuse_quantized("current_rows", getattr(module, "table_dtype", None))
    _refuse_sharded(module, "current_rows")
    _check_row_ids("current_rows", ids)


class CachedEmbeddingBag(nn.Module):
    def __init__(self, num_embeddings: int, embedding_dim: int, padding_idx: Optional[int] = None,
                 max_norm: Optional[float] = None, norm_type: float = 2.0, scale_grad_by_freq: bool = False,
                 sparse: bool = False, _weight: Optional[torch.Tensor] = None, mode: str = "mean",
                 include_last_offset: bool = False, dtype=None, device=None, cache_ratio: float = 0.01,
                 ids_freq_mapping=None, warmup_ratio: float = 0.7, buffer_size: int = 0, pin_weight: bool = False,
                 evict_strategy: EvictionStrategy = EvictionStrategy.DATASET, *, cuda_row_num: Optional[int] = None,
                 init_seed: int = 1024, strict: bool = True, output_dtype: Optional[torch.dtype] = None,
                 table_dtype: Optional[torch.dtype] = None, _table: Optional[HostTable] = None,
                 _idx_map: Optional[torch.Tensor] = None, fused_optimizer: Optional[str] = None,
                 initial_accumulator_value: float = 0.0):
        super().__init__()
        # fused_optimizer="adam" (addition): the host table AND the cache hold rows w | m | v of 3 * D floats -- Adam's
        # moments live where the table lives and travel with the rows through eviction and admission;
        # set_fused_adam(lr) then applies Adam inside backward.  An fp32 table only; embedding_dim keeps meaning D.
        # fused_optimizer="partial_rowwise_adam" (addition; FBGEMM's PARTIAL_ROWWISE_ADAM): rows w | m of
        # 2 * D floats -- the first moment travels with the row --, and the second moment is one fp32 per host-table row
        # in device memory (`.exp_avg_sq`, [N]), fed by the mean of the row's squared gradient.  Everything else is the
        # Adam layout's: set_fused_adam(lr), an fp32 table only, the same refusals.
        # fused_optimizer="adagrad" (addition; torch.optim.Adagrad, FBGEMM's EXACT_ADAGRAD): rows w | h of
        # 2 * D floats, h the per-element sums of squared gradients, every element initial_accumulator_value at first
        # (`.state_sum`, [N, D]); set_fused_adagrad(lr) applies the update inside backward.  The table rules and the
        # refusals are the Adam layouts'.
        if fused_optimizer not in _lib.LAYOUTS:
            raise ValueError(f"fused_optimizer={fused_optimizer!r}: {_lib.LAYOUT_NAMES}")
        _at_least_0("initial_accumulator_value", initial_accumulator_value)
        if initial_accumulator_value != 0.0 and fused_optimizer != "adagrad":
            raise ValueError(f"initial_accumulator_value={initial_accumulator_value!r} needs fused_optimizer='adagrad': "
                             "no other layout has an accumulator in its rows")
        self.fused_optimizer = fused_optimizer
        self.initial_accumulator_value = float(initial_accumulator_value)
        adam = fused_optimizer is not None
        elem = fused_optimizer == "adagrad"
        if adam:
            _lib.check_adam_table(embedding_dim, table_dtype, fused_optimizer)
            _refuse_for_table(f"an {'Adagrad' if elem else 'Adam'}-layout table (fused_optimizer={fused_optimizer!r})",
                              mode, max_norm, sparse, None)
        # output_dtype (addition): dtype of the pooled output and of the gradient coming back -- None / torch.float32,
        # torch.bfloat16 or torch.float16 (functional.embedding_bag(output_dtype=...)).  `dtype` is the TABLE's dtype.
        if dtype not in (None, torch.float32):
            raise NotImplementedError("only fp32 tables are implemented (dtype= is the table's dtype; a 16-bit "
                                      "pooled output is output_dtype=; for a 16-bit table see table_dtype=)")
        # table_dtype (addition): None / torch.float32 -- today's module -- or torch.bfloat16 / torch.float16: the host
        # table AND the cache hold 16-bit rows (half the host DRAM, half of every admission and write-back); sums and
        # updates stay fp32 and a row is rounded once per step (set_weight_rounding).  The pooled output then defaults
        # to the table's dtype.
        # table_dtype=torch.uint8 (addition): an 8-bit row-wise quantized table (q8: rows of 16 + D bytes)
        # for evaluation and serving -- built from trained rows (from_pretrained(..., table_dtype=torch.uint8) or
        # quantized() of a trained module: _table / _idx_map are theirs), never updated; the output defaults to fp32.
        # table_dtype=torch.quint4x2 (addition): the same with 4-bit codes (q4: rows of 16 + D / 2 bytes, DESIGN.md
        # 3.10; quantized(bits=4)).  torch.quint4x2 only spells the format: host table and cache are torch.uint8.
        bits = _lib.quant_bits_of(table_dtype)
        q8 = bits != 0                                      # a quantized table, of either width
        self.table_dtype = table_dtype if q8 else (
            torch.float32 if _lib.table_code(table_dtype) == _lib.CE_ACT_F32 else table_dtype)
        w16 = self.table_dtype in _lib.W16_DTYPES
        if q8:
            (_lib.check_q4_dim if bits == 4 else _lib.check_q8_dim)(embedding_dim)
            _refuse_for_table(f"a {_quant_name(bits)} table: it is forward only", mode, max_norm, sparse, None)
            if _weight is None and _table is None:
                raise NotImplementedError(f"a {_quant_name(bits)} table is built from trained rows, it cannot be "
                                          "initialised: CachedEmbeddingBag.from_pretrained(embeddings, "
                                          f"table_dtype={self.table_dtype}) or quantized({'bits=4' if bits == 4 else ''}) "
                                          "of a trained module")
        if w16:
            _lib.check_w16_dim(embedding_dim)
            _refuse_for_table(f"a 16-bit table (table_dtype={table_dtype})", mode, max_norm, sparse, None)
        self.set_output_dtype(self.table_dtype if (w16 and output_dtype is None) else output_dtype)
        self.weight_rounding, self.weight_rounding_seed = "stochastic", 0
        _lib.require_gpu()
        assert cache_ratio <= 1.0, f"cache ratio {cache_ratio} must less than 1.0"
        self.num_embeddings = num_embeddings
        self.embedding_dim = embedding_dim
        if padding_idx is not None:
            if padding_idx > 0:
                assert padding_idx < num_embeddings, "Padding_idx must be within num_embeddings"
            elif padding_idx < 0:
                assert padding_idx >= -num_embeddings, "Padding_idx must be within num_embeddings"
                padding_idx = num_embeddings + padding_idx
        self.padding_idx = padding_idx
        self.max_norm = max_norm
        self.norm_type = norm_type
        self.scale_grad_by_freq = scale_grad_by_freq
        self.sparse = sparse
        self.mode = mode
        self.include_last_offset = include_last_offset
        self.evict_strategy = evict_strategy
        self.cache_ratio = cache_ratio
        self.cuda_row_num = int(num_embeddings * cache_ratio) if cuda_row_num is None else int(cuda_row_num)
        self.pool_str = mode
        self.cache_op = True
        self.fused_sgd = FusedSGD(None)
        self.fused_adagrad = FusedRowwiseAdagrad(None)
        self.fused_adam = None
        self.fused_elementwise_adagrad = None

        if _table is not None:
            table = _table
            assert table.tensor.dtype == (torch.uint8 if q8 else self.table_dtype) and table.quant_bits == bits \
                and table.tensor.shape[0] == num_embeddings and table.layout == fused_optimizer
        elif adam:
            table = HostTable.allocate(num_embeddings, embedding_dim, layout=fused_optimizer,
                                       init_acc=self.initial_accumulator_value)
            if _weight is None:
                table.fill_uniform_(-1.0 / num_embeddings, 1.0 / num_embeddings, init_seed)
                if padding_idx is not None:                 # (the w part: the moments are zero, Adagrad's h stays)
                    table.tensor[padding_idx, :embedding_dim].zero_()
            else:
                assert tuple(_weight.shape) == (num_embeddings, embedding_dim)
                table.set_weight_(_weight)                  # zero moments (Adagrad's h: the initial value)
        elif q8:
            w = _weight.detach()
            if w.dtype == torch.uint8:                      # already q8 / q4 rows: pinned in place
                width = _lib.q4_row_bytes(embedding_dim) if bits == 4 else _lib.q8_row_bytes(embedding_dim)
                assert tuple(w.shape) == (num_embeddings, width)
                table = HostTable.wrap(w if w.device.type == "cpu" and w.is_contiguous() else w.cpu().contiguous(),
                                       quant_bits=bits)
            else:
                assert tuple(w.shape) == (num_embeddings, embedding_dim)
                if w.dtype not in _lib.ACT_DTYPES:
                    w = w.float()
                table = HostTable.allocate(num_embeddings, embedding_dim, dtype=self.table_dtype).quantize_from(
                    w.cpu().contiguous())
        elif _weight is None:
            table = HostTable.allocate(num_embeddings, embedding_dim, dtype=self.table_dtype)
            table.fill_uniform_(-1.0 / num_embeddings, 1.0 / num_embeddings, init_seed)
            if padding_idx is not None:
                table.tensor[padding_idx].zero_()
        else:
            w = _weight.detach()
            assert tuple(w.shape) == (num_embeddings, embedding_dim)
            # (a _weight of another dtype is cast once, to nearest; one of the table's dtype is pinned in place)
            if w.device.type != "cpu" or w.dtype != self.table_dtype or not w.is_contiguous():
                w = w.to("cpu", self.table_dtype).contiguous()
            table = HostTable.wrap(w)
        self.cache_weight_mgr = CachedParamMgr(table, self.cuda_row_num, buffer_size, pin_weight,
                                               evict_strategy=evict_strategy, device=device, strict=strict,
                                               use_idx_map=True if _idx_map is not None else None)
        if _idx_map is not None:                            # quantized(): the source module's id -> row map
            self.cache_weight_mgr._idx_map.copy_(_idx_map)
        self.cache_weight_mgr.reorder(ids_freq_mapping, warmup_ratio)
        if q8:
            self.eval()
        if w16:
            self.set_weight_rounding(self.weight_rounding, self.weight_rounding_seed)
        if elem:
            # the step count lr_decay reads: on the device, so that a replayed graph counts on
            self.adagrad_step = torch.zeros(1, dtype=torch.int64, device=self.cache_weight_mgr.device)
            self.fused_elementwise_adagrad = FusedAdagrad(None, step=self.adagrad_step)
        elif adam:
            # the step count Adam's bias correction reads: on the device, so that a replayed graph counts on
            self.adam_step = torch.zeros(1, dtype=torch.int64, device=self.cache_weight_mgr.device)
            mgr = self.cache_weight_mgr
            if fused_optimizer == "partial_rowwise_adam":
                # the rows' second moments: one fp32 per host-table row, resident in HBM like row-wise Adagrad's
                # momentum1, indexed through cached_idx_map and never moved by the cache
                mgr.exp_avg_sq = torch.zeros(mgr.num_embeddings, device=mgr.device, dtype=torch.float32)
                self.fused_adam = FusedAdam(None, step=self.adam_step, layout=fused_optimizer,
                                            exp_avg_sq=mgr.exp_avg_sq, row_of_slot=mgr.cached_idx_map)
            else:
                self.fused_adam = FusedAdam(None, step=self.adam_step)

    # -- the host table (upstream `.weight`) and the parameter protocol (A.7) ------------
    @property
    def weight(self) -> torch.Tensor:
        # (an Adam-layout table: the [N, D] view of the rows' w parts; current after flush(), like the moments)
        w = self.cache_weight_mgr.weight
        return w[:, :self.embedding_dim] if self.fused_optimizer is not None else w

    def _adam_part(self, k: int, name: str) -> torch.Tensor:
        if self.fused_optimizer in (None, "adagrad"):
            raise AttributeError(f"{name} exists on a module built with fused_optimizer='adam' or "
                                 "'partial_rowwise_adam'")
        d = self.embedding_dim
        return self.cache_weight_mgr.weight[:, k * d:(k + 1) * d]

    @property
    def exp_avg(self) -> torch.Tensor:
        """Adam's first moment, the [N, D] view of the host table's m parts (torch.optim's name); current after flush()"""
        return self._adam_part(1, "exp_avg")

    @property
    def exp_avg_sq(self) -> torch.Tensor:
        """Adam's second moment, the [N, D] view of the host table's v parts; current after flush().  Partial row-wise
        Adam: the [N] fp32 DEVICE tensor of the rows' second moments, indexed by host-table row (in row space, like
        cache_weight_mgr.momentum1; with ids_freq_mapping row = idx_map[id]); the kernels write it in place."""
        if self.fused_optimizer == "partial_rowwise_adam":
            return self.cache_weight_mgr.exp_avg_sq
        return self._adam_part(2, "exp_avg_sq")

    @property
    def state_sum(self) -> torch.Tensor:
        """Adagrad's per-element sums of squared gradients (torch.optim.Adagrad's state["sum"]), the [N, D] view of the
        host table's h parts, in row space like `.weight`; current after flush()"""
        if self.fused_optimizer != "adagrad":
            raise AttributeError("state_sum exists on a module built with fused_optimizer='adagrad'")
        return self.cache_weight_mgr.weight[:, self.embedding_dim:]

    def load_adagrad_state(self, state_sum: torch.Tensor, step: int) -> None:
        """Restore Adagrad's state, as read from `.state_sum` / `.adagrad_step` of a module with the same id -> row map:
        state_sum [N, D], step the step count.  Flushes first, then writes the host table's h parts and sets the step
        count; the weights are not touched."""
        if self.fused_optimizer != "adagrad":
            raise ValueError("load_adagrad_state needs a module built with fused_optimizer='adagrad'")
        n, d = self.num_embeddings, self.embedding_dim
        if tuple(state_sum.shape) != (n, d):
            raise ValueError(f"state_sum must be [{n}, {d}] (got {tuple(state_sum.shape)})")
        if int(step) < 0:
            raise ValueError(f"step={step!r}: must be >= 0")
        self.flush()
        self.cache_weight_mgr.writeback_wait()              # (the write-backs of the worker transport have landed)
        self.cache_weight_mgr._table.set_state_sum_(state_sum)
        self.adagrad_step.fill_(int(step))

    def load_adam_state(self, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int) -> None:
        """Restore Adam's state, as read from `.exp_avg` / `.exp_avg_sq` / `.adam_step` of a module with the same layout
        and the same id -> row map: exp_avg [N, D]; exp_avg_sq [N, D] (Adam layout) or [N] (partial row-wise Adam); step
        the step count.  Flushes first, then writes the host table's moment parts (the partial layout: the device
        tensor) and sets the step count; the weights are not touched."""
        if self.fused_optimizer in (None, "adagrad"):
            raise ValueError("load_adam_state needs a module built with fused_optimizer='adam' or 'partial_rowwise_adam'")
        n, d = self.num_embeddings, self.embedding_dim
        partial = self.fused_optimizer == "partial_rowwise_adam"
        if tuple(exp_avg.shape) != (n, d):
            raise ValueError(f"exp_avg must be [{n}, {d}] (got {tuple(exp_avg.shape)})")
        if tuple(exp_avg_sq.shape) != ((n,) if partial else (n, d)):
            raise ValueError(f"exp_avg_sq must be {[n] if partial else [n, d]} (got {tuple(exp_avg_sq.shape)})")
        if int(step) < 0:
            raise ValueError(f"step={step!r}: must be >= 0")
        self.flush()
        self.cache_weight_mgr.writeback_wait()              # (the write-backs of the worker transport have landed)
        self.cache_weight_mgr._table.set_moments_(exp_avg, None if partial else exp_avg_sq)
        if partial:
            self.cache_weight_mgr.exp_avg_sq.copy_(exp_avg_sq.detach().to(torch.float32))
        self.adam_step.fill_(int(step))

    def named_parameters(self, prefix: str = "", recurse: bool = True, remove_duplicate: bool = True
                         ) -> Iterator[Tuple[str, nn.Parameter]]:
        yield (prefix + ("." if prefix else "") + "weight", self.cache_weight_mgr.cuda_cached_weight)

    def parameters(self, recurse: bool = True) -> Iterator[nn.Parameter]:
        yield self.cache_weight_mgr.cuda_cached_weight

    def set_cache_op(self, cache_op: bool = True):
        self.cache_op = cache_op

    def set_cache_mgr_async_copy(self, flag: bool):
        self.cache_weight_mgr.set_async_copy(flag)

    # the sharded / table-wise modules name themselves here: their owner-side update (ce_rows_axpy) has no decay and no
    # gradient clipping
    _no_weight_decay: Optional[str] = None

    def set_fused_sgd(self, lr: Union[float, torch.Tensor, None], deterministic: bool = False,
                      accumulator: str = "cache", *, weight_decay: float = 0.0, weight_decay_mode: str = "l2",
                      grad_clip: Optional[float] = None, grad_clip_mode: str = "value"):
        """Apply SGD(lr) to the cache rows inside backward (K13+K14 fused).  lr=None restores
        the plain autograd behaviour (grad handed to torch.optim).  accumulator="step" (a 16-bit table only): the
        update's fp32 accumulator has a row per lookup of the step at most instead of one per cache row.
        lr may be a tensor (functional.check_lr: one fp32 element on the cache's device): it is kept by reference and
        read by the kernels when they run, so fill_ / copy_ into it changes the rate of the next step -- also of a
        step replayed from a hipGraph.  Not with deterministic=True.
        weight_decay / weight_decay_mode ("l2" or "decoupled"; functional.FusedSGD): lazy decay of the rows a step
        looks up.  An fp32 table takes it with deterministic=True only -- the atomic scatter has no per-row pass --,
        which is refused here, before the first step.
        grad_clip / grad_clip_mode ("value" or "row_norm"; functional.check_grad_clip): a row's folded gradient of the
        step is clipped before the decay and the step see it.  Taken where the decay is, refused where it is."""
        wd, clip = _checked_by_accumulator(self, "set_fused_sgd", "sgd", lr, deterministic, accumulator, weight_decay,
                                           weight_decay_mode, grad_clip, grad_clip_mode)
        if lr is not None and self.fused_adagrad.lr is not None:
            raise ValueError("fused row-wise Adagrad is set: set_fused_rowwise_adagrad(None) before set_fused_sgd(lr)")
        if lr is not None and deterministic and self.table_dtype != torch.float32:
            raise NotImplementedError("FusedSGD(deterministic=True) with a 16-bit table")
        _set_by_accumulator(self.fused_sgd, lr, deterministic, accumulator, wd, weight_decay_mode, clip, grad_clip_mode)

    def set_fused_rowwise_adagrad(self, lr: Union[float, torch.Tensor, None], eps: float = 1e-8,
                                  deterministic: bool = False, accumulator: str = "cache", *,
                                  weight_decay: float = 0.0, weight_decay_mode: str = "l2",
                                  grad_clip: Optional[float] = None, grad_clip_mode: str = "value"):
        """Apply exact row-wise Adagrad (FBGEMM's EXACT_ROWWISE_ADAGRAD; the reference's baseline --adagrad; with
        weight_decay / weight_decay_mode "l2" or "decoupled" FBGEMM's L2 / DECOUPLE, lazy: the rows a step looks up
        decay once, at that step, wherever they sit) to the cache rows inside backward.  The state is one fp32 accumulator per row of the host table,
        `cache_weight_mgr.momentum1` (device, zeroed when first enabled, indexed like `weight`); it stays in HBM and
        never moves with the cache.  lr=None turns the update off (the state is kept).  Exclusive with
        set_fused_sgd(lr).  deterministic=True: the sorted, bit-reproducible fold (FusedRowwiseAdagrad), fp32 and
        16-bit tables alike; the host table and the state then do not depend on the cache size or eviction strategy.
        A 16-bit table needs set_weight_rounding("nearest") with it: the sorted fold does not round stochastically.
        accumulator="step": the atomic update with an fp32 accumulator of min(lookups of a step, cache rows) rows
        instead of one as large as the cache (FusedRowwiseAdagrad); not with deterministic=True, and a 16-bit table
        needs set_weight_rounding("nearest") first.
        lr may be a tensor, as in set_fused_sgd; not with deterministic=True.
        grad_clip / grad_clip_mode ("value" or "row_norm"; functional.check_grad_clip): the row's folded gradient is
        clipped first; the decay, the sum of squares and the step see the clipped one.  Every path above takes it."""
        wd, clip = _checked_by_accumulator(self, "set_fused_rowwise_adagrad", "rowwise_adagrad", lr, deterministic,
                                           accumulator, weight_decay, weight_decay_mode, grad_clip, grad_clip_mode)
        if lr is not None and self.fused_sgd.lr is not None:
            raise ValueError("fused SGD is set: set_fused_sgd(None) before set_fused_rowwise_adagrad(lr)")
        mgr = self.cache_weight_mgr
        if lr is not None and getattr(mgr, "momentum1", None) is None:
            mgr.momentum1 = torch.zeros(mgr.num_embeddings, device=mgr.device, dtype=torch.float32)
        _set_by_accumulator(self.fused_adagrad, lr, bool(deterministic), accumulator, wd, weight_decay_mode, clip,
                            grad_clip_mode)
        self.fused_adagrad.eps = float(eps)
        self.fused_adagrad.momentum = getattr(mgr, "momentum1", None)
        self.fused_adagrad.row_of_slot = mgr.cached_idx_map

    def set_fused_adam(self, lr: Union[float, torch.Tensor, None], betas=(0.9, 0.999), eps: float = 1e-8,
                       accumulator: str = "step", deterministic: bool = False, *, weight_decay: float = 0.0,
                       weight_decay_mode: str = "l2", grad_clip: Optional[float] = None, grad_clip_mode: str = "value"):
        """Apply Adam (torch.optim.SparseAdam's arithmetic: only the rows a step looks up move) to the cache rows inside
        backward.  Needs a module built with fused_optimizer="adam": the moments are part of every row, in the host
        table and in the cache, `.exp_avg` / `.exp_avg_sq` after flush(); the step count is `.adam_step` (device).
        lr=None turns the update off (moments and step count are kept; a backward is then a RuntimeError).  lr may be
        a tensor, as in set_fused_sgd.  accumulator: "step" (default) or "cache" -- the size of the fp32 accumulator the
        step's gradient is folded into; both write the same bits given the same folded gradient -- or "sorted": no
        accumulator and no atomics, the step's lookups sorted by slot and every row's gradient folded in lookup order,
        so that two runs of a job agree bit for bit whatever the cache holds (this, not
        deterministic=True, is the switch of the deterministic fold here).  weight_decay with
        weight_decay_mode "l2" is torch.optim.Adam(weight_decay=), with "decoupled" torch.optim.AdamW, both lazy: the
        rows a step looks up decay once, at that step (functional.FusedAdam).  grad_clip / grad_clip_mode ("value" or
        "row_norm"; functional.check_grad_clip): the row's folded gradient is clipped before the decay and the moments
        see it -- clip_grad_value_ / a per-row clip_grad_norm_ in front of optimizer.step().  Exclusive with
        set_fused_sgd / set_fused_rowwise_adagrad: an Adam-layout module refuses those."""
        if self.fused_optimizer in (None, "adagrad"):
            raise ValueError("set_fused_adam needs a module built with fused_optimizer='adam' (or 'partial_rowwise_adam'): "
                             "Adam's moments live in the rows of the table")
        wd, clip = _checked_in_row(self, "adam", lr, weight_decay, weight_decay_mode, grad_clip, grad_clip_mode)
        self.fused_adam.set(betas, eps, accumulator, deterministic, weight_decay=wd,       # (deterministic=True: refused;
                            weight_decay_mode=weight_decay_mode, grad_clip=clip,           # accumulator="sorted")
                            grad_clip_mode=grad_clip_mode)
        self.fused_adam.lr = lr

    def set_fused_adagrad(self, lr: Union[float, torch.Tensor, None], eps: float = 1e-10, lr_decay: float = 0.0,
                          accumulator: str = "step", *, weight_decay: float = 0.0, weight_decay_mode: str = "l2",
                          grad_clip: Optional[float] = None, grad_clip_mode: str = "value"):
        """Apply element-wise Adagrad (torch.optim.Adagrad's arithmetic on the rows a step looks up; FBGEMM's
        EXACT_ADAGRAD) to the cache rows inside backward.  Needs a module built with fused_optimizer="adagrad": the sums
        of squared gradients are part of every row, in the host table and in the cache, `.state_sum` after flush(); the
        step count lr_decay reads is `.adagrad_step` (device).  lr=None turns the update off (state and step count are
        kept; a backward is then a RuntimeError).  lr may be a tensor, as in set_fused_sgd.  accumulator ("sorted"
        included: the deterministic fold), weight_decay
        ("l2": torch.optim.Adagrad(weight_decay=); "decoupled": w is scaled by 1 - clr * weight_decay first, clr the
        decayed rate) and grad_clip as in set_fused_adam (functional.FusedAdagrad).  Exclusive with the other
        set_fused_*: an Adagrad-layout module refuses those, every other module refuses this."""
        if self.fused_optimizer != "adagrad":
            raise ValueError("set_fused_adagrad needs a module built with fused_optimizer='adagrad': Adagrad's sums of "
                             "squares live in the rows of the table")
        wd, clip = _checked_in_row(self, "adagrad", lr, weight_decay, weight_decay_mode, grad_clip, grad_clip_mode)
        self.fused_elementwise_adagrad.set(eps, lr_decay, accumulator, weight_decay=wd,
                                           weight_decay_mode=weight_decay_mode, grad_clip=clip,
                                           grad_clip_mode=grad_clip_mode)
        self.fused_elementwise_adagrad.lr = lr

    def set_weight_rounding(self, rounding: str = "stochastic", seed: int = 0):
        """How the fused updates round a row of a 16-bit table: "nearest" (round-to-nearest-even) or "stochastic" (the
        default: one of the two 16-bit neighbours, with probabilities that make the rounding unbiased; the random bits
        are a hash of seed, step, host-table row and element).  A ValueError for an fp32 table."""
        if self.table_dtype not in _lib.W16_DTYPES:
            raise ValueError("set_weight_rounding is meaningful only with a 16-bit table (table_dtype=)")
        if rounding not in ("nearest", "stochastic"):
            raise ValueError(f"rounding={rounding!r}: 'nearest' or 'stochastic'")
        self.weight_rounding, self.weight_rounding_seed = rounding, int(seed)
        for f in (self.fused_sgd, self.fused_adagrad):
            f.rounding, f.seed = rounding, int(seed)
        # the random bits follow the host-table row, not the slot it happens to sit in
        self.fused_sgd.row_of_slot = self.cache_weight_mgr.cached_idx_map

    def set_output_dtype(self, dtype: Optional[torch.dtype]):
        """dtype of the pooled output, training and eval alike: None / torch.float32 (default), torch.bfloat16 or
        torch.float16.  The table, the sums and the fused updates stay fp32; the forward kernels round once on the
        store and the backward kernels read the 16-bit gradient autograd hands back in place."""
        _lib.act_code(dtype)                 # NotImplementedError for anything else
        self.output_dtype = torch.float32 if dtype is None else dtype

    def _fused(self):
        if self.fused_adam is not None:                     # an Adam-layout table: the forward needs the object too
            return self.fused_adam
        if self.fused_elementwise_adagrad is not None:      # an Adagrad-layout table: likewise
            return self.fused_elementwise_adagrad
        return self.fused_adagrad if self.fused_adagrad.lr is not None else self.fused_sgd

    def forward(self, input: torch.Tensor, offsets: Optional[torch.Tensor] = None,
                per_sample_weights: Optional[torch.Tensor] = None, shape_hook: Optional[Callable] = None,
                *, hook_features: int = 0, presorted: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        # out (addition): the pooled output is written into this tensor (functional.embedding_bag(out=...))
        masked = False
        if self.cache_op:
            with torch.no_grad():
                ids = input
                input = self.cache_weight_mgr.prepare_ids(ids)
                if self.padding_idx is not None:
                    if presorted is not None:
                        raise NotImplementedError("padding_idx cannot be combined with presorted keys: they were "
                                                  "built from slots that still hold the padding lookups")
                    masked = True
                    # nn.EmbeddingBag semantics in ID space (upstream hands padding_idx to F.embedding_bag in slot
                    # space, which is not meaningful): lookups of the padding id take no part in the
                    # reduction and get no gradient -- the kernels skip slot -1.  With cache_op=False the caller
                    # passes slots and masks them itself.
                    input = torch.where(ids == self.padding_idx, torch.full_like(input, -1), input)
        out = embedding_bag(input, self.cache_weight_mgr.cuda_cached_weight, offsets, self.max_norm,
                            self.norm_type, self.scale_grad_by_freq, self.mode, self.sparse, per_sample_weights,
                            self.include_last_offset, None, hook_features=hook_features,
                            fused_sgd=self._fused(), presorted=presorted, masked_indices=masked, out=out,
                            output_dtype=self.output_dtype, quant_bits=4 if self.table_dtype == _lib.Q4 else 8)
        if shape_hook is not None:
            out = shape_hook(out)
        return out

    # -- observability surface (recsys/dlrm_main.py:286-294) -----------------------------
    @property
    def num_hits_history(self) -> List[int]:
        self.cache_weight_mgr.sync_stats()
        return self.cache_weight_mgr.num_hits_history

    @property
    def num_miss_history(self) -> List[int]:
        self.cache_weight_mgr.sync_stats()
        return self.cache_weight_mgr.num_miss_history

    @property
    def num_write_back_history(self) -> List[int]:
        self.cache_weight_mgr.sync_stats()
        return self.cache_weight_mgr.num_write_back_history

    def print_comm_stats_(self):
        return self.cache_weight_mgr.print_comm_stats()

    def element_size(self) -> int:
        return self.weight.element_size()

    def flush(self):
        self.cache_weight_mgr.flush()

    # -- rows refreshed in place ------------------------------------------
    def refresh_rows(self, ids: torch.Tensor, rows: torch.Tensor) -> None:
        """Give the rows of `ids` new values in place, behind the cache: ids 1-D int64, DISTINCT, on any device; rows
        [n, D] fp32 / bf16 / fp16, on any device (moved to the GPU).  On a q8 / q4 module the rows are quantized on the
        GPU (functional.quantize_rows_device: the bytes quantize_rows gives) -- a row holding a NaN or an infinity raises
        and NOTHING is installed --, on an fp32 / bf16 / fp16 table they are cast to the table's dtype, to nearest.
        Every live copy of a row gets the new value: the host row and, where the row is resident, its cache slot
        (CachedParamMgr.install_rows); the cache stays as warm as it was -- nothing is admitted, evicted or counted.
        Returns when the rows are in place.  Optimizer state kept outside the rows -- the row-wise Adagrad accumulator
        `cache_weight_mgr.momentum1` -- is left alone.  Duplicate ids: ValueError; an id outside [0, num_embeddings):
        IndexError, nothing written; n == 0: nothing happens.  Refused before the GPU is asked for: an in-row layout
        (fused_optimizer=: a row there is weights plus state), the sharded classes, a wrong shape or dtype."""
        _check_refresh_rows(self, ids, rows)
        if ids.numel() == 0:
            return
        _lib.require_gpu()
        mgr = self.cache_weight_mgr
        with torch.no_grad(), torch.cuda.device(mgr.device):
            ids_d = ids.detach().to(mgr.device).contiguous()
            rows_d = rows.detach().to(mgr.device).contiguous()
            if torch.unique(ids_d).numel() != ids_d.numel():
                raise ValueError("refresh_rows needs distinct ids: with duplicates a row's new value is not defined")
            bits = _lib.quant_bits_of(self.table_dtype)
            packed = quantize_rows_device(rows_d, bits) if bits else rows_d.to(self.table_dtype)
            mgr.install_rows(ids_d, packed)

    def current_rows(self, ids: torch.Tensor) -> torch.Tensor:
        """The present value of the rows of `ids` (1-D int64, any device), [n, D] in the table's dtype on the GPU, WITHOUT
        a flush: a resident row is read from its cache slot, any other from the host table (through its device mapping)
        once the write-backs of the worker transport have landed.  The cache is left as it is.  An in-row layout gives
        the rows' w parts.  Not on a quantized table (dequantize_rows of `.weight` rows is its reading)."""
        _check_current_rows(self, ids)
        _lib.require_gpu()
        mgr = self.cache_weight_mgr
        with torch.no_grad(), torch.cuda.device(mgr.device):
            ids_d = ids.detach().to(mgr.device).contiguous()
            n = ids_d.numel()
            out = torch.empty(n, mgr._row_width, dtype=mgr._weight.dtype, device=mgr.device)
            if n:
                if int(((ids_d < 0) | (ids_d >= self.num_embeddings)).sum().item()):
                    raise IndexError(f"current_rows: an id is outside [0, {self.num_embeddings})")
                mgr.writeback_wait()
                mgr.wait_rows()                             # (deferred rows: the maps may name a slot whose row is still
                slots = mgr._id_to_cached_cuda_id(ids_d)    #  travelling on the library's admission stream)
                resident = slots >= 0
                host_rows = ids_d if mgr._idx_map is None else mgr._idx_map[ids_d].long()
                host_rows = torch.where(resident, torch.full_like(host_rows, -1), host_rows)     # (-1: a zero row)
                _lib.check(_lib.lib.ce_host_rows_gather(mgr._table.dev_ptr, mgr.num_embeddings, mgr._lib_dim,
                                                        _lib.ptr(host_rows), n, _lib.ptr(out), _lib.stream_ptr()))
                out[resident] = mgr.cuda_cached_weight.data[slots[resident]]
        return out[:, :self.embedding_dim].contiguous() if self.fused_optimizer is not None else out

    def refresh_from(self, source: "CachedEmbeddingBag", ids: torch.Tensor) -> None:
        """refresh_rows(ids, source.current_rows(ids)): the rows of `ids` as the module `source` -- the trainer -- holds
        them now reach this (served) module, with no flush of either.  Both modules must have the same num_embeddings,
        embedding_dim and id -> row map; quantized() carries the map over, so a module made by source.quantized()
        qualifies."""
        for name in ("num_embeddings", "embedding_dim"):
            if getattr(source, name, None) != getattr(self, name):
                raise ValueError(f"refresh_from needs a source with the same {name} ({getattr(self, name)}; the source "
                                 f"has {getattr(source, name, None)})")
        _check_refresh_rows(self, ids, None)
        _check_current_rows(source, ids)
        _lib.require_gpu()
        mine, theirs = self.cache_weight_mgr._idx_map, source.cache_weight_mgr._idx_map
        if (mine is None) != (theirs is None) or (mine is not None and not torch.equal(mine, theirs.to(mine.device))):
            raise ValueError("refresh_from needs a source with the same id -> row map (idx_map): a module made by "
                             "source.quantized() has it")
        self.refresh_rows(ids, source.current_rows(ids))

    @classmethod
    def from_pretrained(cls, embeddings: torch.Tensor, freeze: bool = True, **kwargs) -> "CachedEmbeddingBag":
        rows, cols = embeddings.shape
        bits = _lib.quant_bits_of(kwargs.get("table_dtype"))
        if bits:
            # table_dtype=torch.uint8: the fp32 / bf16 / fp16 rows are quantized (functional.quantize_rows), or q8 rows
            # ([rows, 16 + D] uint8) are taken as they are; the module is eval-only.  table_dtype=torch.quint4x2: the
            # same with q4 rows -- a uint8 tensor is then taken as [rows, 16 + D / 2] q4 rows
            if not freeze:
                raise NotImplementedError(f"from_pretrained(freeze=False) with a {_quant_name(bits)} table: a quantized "
                                          "table is never updated")
            if embeddings.dtype == torch.uint8:
                cols = 2 * (cols - _lib.CE_Q4_HEADER_BYTES) if bits == 4 else cols - _lib.CE_Q8_HEADER_BYTES
            return cls(rows, cols, _weight=embeddings, **kwargs)
        m = cls(rows, cols, _weight=embeddings, **kwargs)
        m.cache_weight_mgr.cuda_cached_weight.requires_grad_(not freeze)
        return m

    def quantized(self, bits: int = 8, **overrides) -> "CachedEmbeddingBag":
        """An eval-only module over the 8-bit row-wise quantized (q8) copy of this module's table: this module is
        flushed, its host table is quantized row by row -- in row space, so the id -> row map (idx_map) carries over --
        into a new pinned table, and the new module has this one's mode, include_last_offset, padding_idx, eviction
        strategy, cuda_row_num, output dtype and idx_map.  overrides: cuda_row_num (a q8 row of D elements is 16 + D
        bytes: the same HBM holds more rows), output_dtype, warmup_ratio, buffer_size, strict.  This module is left as it
        is and trains on.  bits=4: the 4-bit (q4) copy, rows of 16 + D / 2 bytes."""
        if self.table_dtype == _lib.Q8:
            raise NotImplementedError("quantized() of a q8 (torch.uint8) module: it is quantized already")
        if self.table_dtype == _lib.Q4:
            raise NotImplementedError("quantized() of a q4 (torch.quint4x2) module: it is quantized already")
        dtype = _lib.Q4 if _lib.check_quant_bits(bits) == 4 else _lib.Q8
        if getattr(self, "world_size", 1) > 1:
            _lib.refuse_quantized(f"{type(self).__name__}.quantized() on {self.world_size} ranks", dtype)
        bad = set(overrides) - {"cuda_row_num", "output_dtype", "warmup_ratio", "buffer_size", "strict"}
        if bad:
            raise TypeError(f"quantized() got unexpected overrides {sorted(bad)}")
        _refuse_for_table(f"a {_quant_name(bits)} table: it is forward only", self.mode, self.max_norm, False, None)
        (_lib.check_q4_dim if bits == 4 else _lib.check_q8_dim)(self.embedding_dim)
        mgr = self.cache_weight_mgr
        self.flush()
        src = self.weight                                   # (waits for the write-backs of the worker transport)
        if self.fused_optimizer is not None:
            src = src.contiguous()                          # the w parts alone: the moments are not quantized
        table = HostTable.allocate(self.num_embeddings, self.embedding_dim, dtype=dtype).quantize_from(src)
        kw = dict(cuda_row_num=self.cuda_row_num, output_dtype=self.output_dtype, warmup_ratio=0.7,
                  buffer_size=mgr.buffer_size, strict=mgr.strict)
        kw.update(overrides)
        return CachedEmbeddingBag(self.num_embeddings, self.embedding_dim, padding_idx=self.padding_idx, mode=self.mode,
                                  include_last_offset=self.include_last_offset, device=mgr.device,
                                  evict_strategy=self.evict_strategy, table_dtype=dtype, _table=table,
                                  _idx_map=mgr._idx_map, **kw)
