#!/usr/bin/env python
"""DLRM trainer around the MI355X-native cached EmbeddingBag -- the counterpart of the reference's
recsys/dlrm_main.py, with the reference's flag names for everything that touches the hot path
(recsys/dlrm_main.py:23-173) and its training-loop structure (`_train`, :206-297):

    every `--prefetch_num` iterations: pull P batches from the (side-stream) data iterator,
    ONE cache_weight_mgr.prepare_ids over their concatenated ids, slots split back per batch;
    every iteration: forward with cache_op=False, BCE-with-logits loss, backward, optimizer step.

Only the embedding operator is this repository's product; the dense part (bottom MLP, pairwise-dot
interaction, top MLP -- the standard DLRM arch the reference takes from torchrec) is stock torch.nn and the
data is synthetic by default (Criteo/Avazu-shaped KJT batches; no dataset exists on the box) or, with
`--dataset_dir`, the binary npy Criteo files the reference reads (cachedembedding_amd/datasets.py).  One process per GPU:
with WORLD_SIZE > 1 the embedding is column-sharded exactly like the reference's default
(ParallelCachedEmbeddingBag + dual_all_to_all) and the dense part is DDP.

  python examples/dlrm_main.py --dataset criteo_kaggle --use_cache --cache_ratio 0.05 --use_freq \
      --batch_size 16384 --prefetch_num 8 --use_overlap --use_sparse_embed_grad --limit_train_batches 200
"""
from __future__ import annotations

import argparse
import itertools
import os
import sys
import time
from pathlib import Path
from typing import List, Optional

import torch
import torch.distributed as dist
import torch.nn as nn

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from cachedembedding_amd import synthetic  # noqa: E402
from cachedembedding_amd.cache_mgr import EvictionStrategy  # noqa: E402
from cachedembedding_amd.modules import FiniteDataIter, FusedSparseModules  # noqa: E402
from cachedembedding_amd.pipeline import PrefetchWindow  # noqa: E402
from cachedembedding_amd.tracing import phase  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="DLRM on the cached EmbeddingBag (MI355X)")
    p.add_argument("--dataset", default="criteo_kaggle", choices=list(synthetic.TABLES))
    p.add_argument("--table_scale", type=float, default=1.0)
    # real data: directory of day_*_{dense,sparse,labels}.npy files (recsys/dlrm_main.py:81-101 flag names)
    p.add_argument("--dataset_dir", type=str, default=None)
    p.add_argument("--num_embeddings_per_feature", type=str, default=None)
    p.add_argument("--mmap_mode", action="store_true")
    p.add_argument("--shuffle_batches", action="store_true")
    p.add_argument("--epochs", type=int, default=1)
    p.add_argument("--limit_train_batches", type=int, default=200)
    p.add_argument("--limit_val_batches", type=int, default=None)       # recsys/dlrm_main.py:50-61
    p.add_argument("--limit_test_batches", type=int, default=None)
    p.add_argument("--eval_acc", action="store_true",
                   help="AUROC and accuracy over the val set after every epoch and over the test set at the end "
                        "(recsys/dlrm_main.py:168,358-371)")
    p.add_argument("--eval_q8", action="store_true",
                   help="with --eval_acc, one process, no --use_tablewise: after the final test evaluation the trained "
                        "table is quantized to 8-bit rows (CachedEmbeddingBag.quantized()), the test set is evaluated "
                        "again through it, and test_auroc_q8 / test_accuracy_q8 / the two table sizes are printed as "
                        "one JSON line (and merged into --json_out)")
    p.add_argument("--eval_q8_refresh", action="store_true",
                   help="with --eval_acc, one process, no --use_tablewise: a served 8-bit copy of the table is built ONCE, "
                        "before training (CachedEmbeddingBag.quantized()); the training loop marks the rows it looks up "
                        "in a device bitmap, and every evaluation first brings the served copy up to date with "
                        "served.refresh_from(trainer, marked ids) -- no flush, no rebuild, the served cache stays warm -- "
                        "and evaluates through it too: val_aurocs_q8_refresh, test_auroc_q8_refresh, refreshed_rows_q8")
    p.add_argument("--eval_q4_refresh", action="store_true",
                   help="like --eval_q8_refresh (and beside it, if both are given) with the 4-bit table")
    p.add_argument("--eval_q4", action="store_true",
                   help="like --eval_q8 (and beside it, if both are given) with the 4-bit row-wise quantized table "
                        "(CachedEmbeddingBag.quantized(bits=4)): test_auroc_q4 / test_accuracy_q4 / table_bytes_q4")
    p.add_argument("--batch_size", type=int, default=16384)
    p.add_argument("--num_dense_features", type=int, default=13)
    p.add_argument("--embedding_dim", type=int, default=128)
    p.add_argument("--dense_arch_layer_sizes", type=str, default="512,256,128")
    p.add_argument("--over_arch_layer_sizes", type=str, default="1024,1024,512,256,1")
    p.add_argument("--learning_rate", type=float, default=1.0)
    # baselines/dlrm_main.py:223-242, with the progress counted over the run's total iterations
    p.add_argument("--change_lr", action="store_true",
                   help="change the learning rate part way through training.  With --graph_step the captured step is "
                        "not captured again: the fused update and the dense step read the rate from one device tensor "
                        "that is rewritten at the change point")
    p.add_argument("--lr_change_point", type=float, default=0.80,
                   help="the point through the run's total iterations (all epochs) after which the rate changes")
    p.add_argument("--lr_after_change_point", type=float, default=0.20, help="learning rate after the change point")
    p.add_argument("--seed", type=int, default=1024)
    # hot-path flags, same names as recsys/dlrm_main.py:120-166
    p.add_argument("--use_cache", action="store_true")
    p.add_argument("--cache_ratio", type=float, default=0.01)
    p.add_argument("--use_freq", action="store_true")
    p.add_argument("--use_lfu", action="store_true")
    p.add_argument("--use_lru", action="store_true",
                   help="evict the least recently used rows (EvictionStrategy.LRU; not in the reference's cached "
                        "trainer, its baseline offers it as uvm_lru).  Exclusive with --use_lfu")
    p.add_argument("--warmup_ratio", type=float, default=0.7)
    p.add_argument("--buffer_size", type=int, default=0)
    p.add_argument("--prefetch_num", type=int, default=1)
    p.add_argument("--use_cache_mgr_async_copy", action="store_true")
    p.add_argument("--use_sparse_embed_grad", action="store_true")
    p.add_argument("--use_tablewise", action="store_true")
    p.add_argument("--use_distributed_dataloader", action="store_true")
    p.add_argument("--use_overlap", action="store_true")
    p.add_argument("--overlap_cache_op", action="store_true",
                   help="run the cache op of window k+1 on a side stream while window k trains (not in the reference)")
    p.add_argument("--arrangement", default="overlap", choices=["auto", "overlap", "interleaved"],
                   help="with --overlap_cache_op: where the next window's cache op runs -- on a side stream beside this "
                        "window's steps (overlap, the default of an eager trainer since round 6), in two halves on the "
                        "training stream around them (interleaved), or whichever of the two the library measures faster "
                        "while training (auto: pipeline.ArrangementTrial).  With eager steps the interleaved form costs "
                        "every later dispatch of the training stream ~40 us (217 -> 135 it/s at Criteo-1TB shapes, "
                        "profiles/r06_dlrm_interleaved_dispatch.md), and a trial that starts with it measures both "
                        "arrangements slow")
    p.add_argument("--arrangement_block_windows", type=int, default=8,
                   help="--arrangement auto: windows per block of the library's trial (3 blocks per arrangement; a window "
                        "of a whole model takes tens of milliseconds, so short blocks measure well)")
    # additions of this build
    p.add_argument("--fused_sgd", action="store_true", help="apply the embedding SGD inside backward")
    p.add_argument("--adagrad", action="store_true",
                   help="exact row-wise Adagrad for the embedding, fused into backward (FBGEMM's EXACT_ROWWISE_ADAGRAD, "
                        "as baselines/dlrm_main.py:698-702 maps --adagrad), torch.optim.Adagrad for the dense part "
                        "(:799-802); takes the place of --fused_sgd (one process)")
    p.add_argument("--adam", action="store_true",
                   help="Adam for the embedding, fused into backward, with the moments carried in the table's rows "
                        "(CachedEmbeddingBag(fused_optimizer='adam') + set_fused_adam: torch.optim.SparseAdam's "
                        "arithmetic; the moments travel with the rows between host table and cache), torch.optim.Adam "
                        "for the dense part.  One process, an fp32 table, without --use_tablewise; not with --adagrad or "
                        "--fused_sgd")
    p.add_argument("--adam_partial_rowwise", action="store_true",
                   help="with --adam: partial row-wise Adam (FBGEMM's PARTIAL_ROWWISE_ADAM; "
                        "CachedEmbeddingBag(fused_optimizer='partial_rowwise_adam')): the first moment travels in the "
                        "row, the second moment is one fp32 per table row in device memory -- rows of 2 * D floats "
                        "instead of 3 * D")
    p.add_argument("--adagrad_elementwise", action="store_true",
                   help="element-wise Adagrad for the embedding, fused into its backward (torch.optim.Adagrad's "
                        "arithmetic, FBGEMM's EXACT_ADAGRAD: one sum of squares per ELEMENT, carried in the row -- "
                        "CachedEmbeddingBag(fused_optimizer='adagrad') + set_fused_adagrad; rows of 2 * D floats), "
                        "torch.optim.Adagrad for the dense part.  One process, an fp32 table, without --use_tablewise; "
                        "not with --adagrad, --adam, --adam_partial_rowwise or --fused_sgd")
    p.add_argument("--adam_beta1", type=float, default=0.9, help="with --adam: beta1 of both Adams")
    p.add_argument("--adam_beta2", type=float, default=0.999, help="with --adam: beta2 of both Adams")
    p.add_argument("--eps", type=float, default=1e-8, help="with --adam: eps of both Adams")
    p.add_argument("--adagrad_deterministic", action="store_true",
                   help="with --adagrad: fold a row's gradient in lookup order over the step's sorted lookups instead "
                        "of by atomics -- bit-reproducible, and without the [cache rows, D] fp32 accumulator")
    p.add_argument("--embed_sorted_update", action="store_true",
                   help="with --adam, --adam_partial_rowwise or --adagrad_elementwise: fold a row's gradient in lookup "
                        "order over the step's sorted lookups instead of by atomics (accumulator='sorted') -- two runs "
                        "of a job agree bit for bit; the rate is read from device memory, so --graph_step --change_lr "
                        "work with it.  --adagrad has --adagrad_deterministic for this; not with --step_accumulator")
    p.add_argument("--step_accumulator", action="store_true",
                   help="with --adagrad, or with a 16-bit --table_dtype and --fused_sgd: the fused update's fp32 "
                        "accumulator has a row per lookup of a step at most instead of one per cache row "
                        "(accumulator='step'); not with --adagrad_deterministic, and --adagrad on a 16-bit table needs "
                        "--weight_rounding nearest with it")
    p.add_argument("--embed_weight_decay", type=float, default=0.0,
                   help="weight decay of the embedding's fused update (--adagrad, --adam or --fused_sgd), lazy: the "
                        "rows a step looks up decay once, in that step; the dense part is not touched.  --fused_sgd on "
                        "an fp32 table has no per-row pass and refuses it")
    p.add_argument("--embed_weight_decay_mode", choices=("l2", "decoupled"), default="l2",
                   help="l2: the decay joins the gradient (torch.optim.Adam / Adagrad / SGD weight_decay, FBGEMM L2); "
                        "decoupled: the row is scaled by 1 - lr * decay first (torch.optim.AdamW, FBGEMM DECOUPLE)")
    p.add_argument("--embed_grad_clip", type=float, default=None,
                   help="gradient clipping of the embedding's fused update (--adagrad, --adam or --fused_sgd): a row's "
                        "folded gradient of the step is clipped before the decay and the optimizer see it; the dense "
                        "part is not touched.  --fused_sgd on an fp32 table has no per-row pass and refuses it")
    p.add_argument("--embed_grad_clip_mode", choices=("value", "row_norm"), default="value",
                   help="value: every element is clamped to [-clip, clip] (torch clip_grad_value_, FBGEMM max_gradient); "
                        "row_norm: a row is scaled down to the 2-norm clip (clip_grad_norm_, every row its own parameter)")
    p.add_argument("--fold_hook", action="store_true", help="write [B,F,D] from the gather kernel")
    p.add_argument("--window_keys", action="store_true",
                   help="the window's cache op also groups every batch's slots by row (source-row keys): the forward "
                        "loads a cache row once per run, the fused backward streams over the keys (needs --fused_sgd "
                        "--fold_hook; one id per bag)")
    p.add_argument("--warmup_batches", type=int, default=16, help="iterations before the throughput clock starts "
                   "(library initialisation, GEMM algorithm search, pipeline fill)")
    p.add_argument("--graph_step", action="store_true",
                   help="one process, --fused_sgd --fold_hook: after --graph_after eager iterations the whole iteration -- "
                        "embedding forward, dense forward, loss, backward (with the embedding's fused update) and the dense "
                        "optimizer step -- is captured ONCE in a hipGraph (torch.cuda.graph, stock torch) and replayed on "
                        "static input buffers; the window's cache op stays outside it.  An iteration is ~60 kernels launched "
                        "from Python: on a host with a small CPU quota the launch thread, not the GPU, sets the pace "
                        "(VERDICT r5 #6)")
    p.add_argument("--graph_after", type=int, default=8, help="--graph_step: eager iterations before the capture (lazy "
                   "initialisation, GEMM algorithm selection / TunableOp tuning must be over)")
    p.add_argument("--tunable_gemm", action="store_true",
                   help="the dense part's GEMMs through torch's TunableOp (stock torch: every GEMM shape of the two MLPs and "
                        "of the interaction is timed once over the rocBLAS / hipBLASLt solutions and the fastest kept; fp32 "
                        "as before, nothing hand-written) -- VERDICT r5 #6")
    p.add_argument("--embedding_output_dtype", default="fp32", choices=["fp32", "bf16"],
                   help="dtype of the pooled embeddings (CachedEmbeddingBag(output_dtype=...)).  bf16: the embedding "
                        "kernels write bf16 and read the bf16 gradient in place (the table and its update stay fp32), "
                        "and the dense part's forward runs under torch.autocast('cuda', torch.bfloat16).  One process, "
                        "without --use_tablewise.  (fp16 is a library option only: a trainer would need loss scaling)")
    p.add_argument("--table_dtype", default="fp32", choices=["fp32", "bf16", "fp16"],
                   help="dtype of the embedding table's rows, in host DRAM and in the cache "
                        "(CachedEmbeddingBag(table_dtype=...)).  bf16 / fp16: half the host memory and half of every "
                        "admission and write-back; sums and updates stay fp32 and the fused update (--fused_sgd or "
                        "--adagrad) rounds a row once per step.  One process, without --use_tablewise; the pooled "
                        "embeddings keep --embedding_output_dtype")
    p.add_argument("--weight_rounding", default="stochastic", choices=["nearest", "stochastic"],
                   help="--table_dtype bf16 / fp16: how the fused update rounds a row (set_weight_rounding)")
    p.add_argument("--json_out", type=str, default=None, help="write the run's numbers as one JSON object")
    args = p.parse_args(argv)
    if args.use_lfu and args.use_lru:
        p.error("--use_lfu and --use_lru exclude each other")
    return args


_OUTPUT_DTYPES = {"fp32": None, "bf16": torch.bfloat16}
_TABLE_DTYPES = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}


def _fused_optimizer(args) -> Optional[str]:
    """the layout --adam / --adagrad_elementwise builds the table with"""
    if args.adagrad_elementwise:
        return "adagrad"
    if not args.adam:
        return None
    return "partial_rowwise_adam" if args.adam_partial_rowwise else "adam"


def check_output_dtype(args, world: int) -> None:
    """--embedding_output_dtype bf16 is refused, before anything is built, where the pooled output crosses ranks"""
    if args.embedding_output_dtype != "fp32" and (world > 1 or args.use_tablewise):
        raise NotImplementedError("--embedding_output_dtype bf16 is implemented for one process without "
                                  "--use_tablewise (the all-to-all of the pooled output is fp32)")
    if args.table_dtype != "fp32" and (world > 1 or args.use_tablewise):
        raise NotImplementedError(f"--table_dtype {args.table_dtype} is implemented for one process without "
                                  "--use_tablewise")
    if args.table_dtype != "fp32" and args.use_sparse_embed_grad:
        raise NotImplementedError(f"--table_dtype {args.table_dtype} with --use_sparse_embed_grad")


def mlp(sizes: List[int], last_activation: bool) -> nn.Sequential:
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(nn.Linear(sizes[i], sizes[i + 1]))
        if i + 2 < len(sizes) or last_activation:
            layers.append(nn.ReLU())
    return nn.Sequential(*layers)


class DenseModules(nn.Module):
    """bottom MLP -> pairwise dots of the F+1 vectors (upper triangle) -> top MLP"""

    def __init__(self, num_dense: int, num_sparse: int, dim: int, dense_sizes: List[int], over_sizes: List[int]):
        super().__init__()
        assert dense_sizes[-1] == dim
        self.bottom = mlp([num_dense] + dense_sizes, last_activation=True)
        n = num_sparse + 1
        self.register_buffer("tri", torch.triu_indices(n, n, offset=1), persistent=False)
        self.top = mlp([dim + n * (n - 1) // 2] + over_sizes, last_activation=False)

    def forward(self, dense: torch.Tensor, sparse: torch.Tensor) -> torch.Tensor:
        d = self.bottom(dense)                                   # [B, D]
        z = torch.cat([d.unsqueeze(1), sparse], dim=1)           # [B, F+1, D]
        inter = torch.bmm(z, z.transpose(1, 2))[:, self.tri[0], self.tri[1]]
        return self.top(torch.cat([d, inter], dim=1))


class HybridParallelDLRM(nn.Module):
    """model-parallel sparse part + data-parallel dense part (recsys/models/dlrm.py:144-235)"""

    def __init__(self, sizes, args, id_freq_map, device):
        super().__init__()
        self.sparse_modules = FusedSparseModules(
            sizes, args.embedding_dim, reduction_mode="sum", sparse=args.use_sparse_embed_grad,
            use_cache=args.use_cache, cache_ratio=args.cache_ratio, id_freq_map=id_freq_map,
            warmup_ratio=args.warmup_ratio, buffer_size=args.buffer_size,
            is_dist_dataloader=args.use_distributed_dataloader, use_lfu_eviction=args.use_lfu,
            evict_strategy=EvictionStrategy.LRU if args.use_lru else None,
            use_tablewise_parallel=args.use_tablewise, dataset=args.dataset, fold_hook=args.fold_hook,
            # (a 16-bit table's output would default to the table's dtype: the flag's fp32 stays fp32)
            output_dtype=_OUTPUT_DTYPES[args.embedding_output_dtype] or
            (torch.float32 if args.table_dtype != "fp32" else None),
            table_dtype=_TABLE_DTYPES[args.table_dtype], fused_optimizer=_fused_optimizer(args))
        self.autocast = args.embedding_output_dtype == "bf16"
        dense = DenseModules(args.num_dense_features, len(sizes), args.embedding_dim,
                             [int(x) for x in args.dense_arch_layer_sizes.split(",")],
                             [int(x) for x in args.over_arch_layer_sizes.split(",")]).to(device)
        if dist.is_initialized() and dist.get_world_size() > 1:
            dense = nn.parallel.DistributedDataParallel(dense, device_ids=[device.index], gradient_as_bucket_view=True,
                                                        broadcast_buffers=False, static_graph=True)
        self.dense_modules = dense
        self.dense_device = self.sparse_device = device

    def forward(self, dense, sparse, cache_op: bool = True, presorted=None):
        emb = self.sparse_modules(sparse, cache_op=cache_op, presorted=presorted)     # [B(/W), F, D]
        if self.autocast:
            # bf16 pooled embeddings: the dense part's GEMMs in bf16 too; the logits go back to fp32 for the loss
            with torch.autocast("cuda", torch.bfloat16):
                return self.dense_modules(dense, emb).float()
        return self.dense_modules(dense, emb)


class SyntheticLoader:
    """In-memory loader like the reference's npy pipe (recsys/datasets/criteo.py:38-249): all batches are
    materialised in pinned host memory up front -- dense fp32 [B, 13], KJT list [values, offsets, stride],
    labels -- so an iteration only pays the host->HBM copy (overlapped by FiniteDataIter)."""

    def __init__(self, sizes, batch_size, num_dense, n_batches, seed):
        gen = synthetic.SyntheticKJT(sizes, batch_size, 1, "power_law", 0.25, seed=seed, device="cuda")
        cpu_gen = torch.Generator().manual_seed(seed)
        offsets = gen.offsets.cpu().pin_memory()
        self.batches = []
        done = 0
        while done < n_batches:
            k = min(16, n_batches - done)
            vals = gen.next_values(k).cpu()
            for i in range(k):
                self.batches.append(dict(
                    dense=torch.rand(batch_size, num_dense, generator=cpu_gen).pin_memory(),
                    sparse=[vals[i].contiguous().pin_memory(), offsets, batch_size],
                    labels=None))
                # a learnable target: a function of one dense feature and of the parity of the first sparse id
                b = self.batches[-1]
                b["labels"] = ((b["dense"][:, 0] + (vals[i][:batch_size] % 2).float() * 0.5) > 0.75).float().pin_memory()
            done += k

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


class _Limit:
    """first n batches of a loader (--limit_train_batches)"""

    def __init__(self, loader, n):
        self.loader, self.n = loader, n

    def __len__(self):
        return min(self.n, len(self.loader))

    def __iter__(self):
        return itertools.islice(iter(self.loader), self.n)


def put_data_in_device(batch, device, is_dist, rank, world):
    """recsys/dlrm_main.py:195-203: with the non-distributed loader every rank holds the global batch and
    keeps its slice of dense/labels, the sparse part stays global"""
    dense, labels = batch["dense"].to(device), batch["labels"].to(device).float()
    sparse = [t.to(device) if torch.is_tensor(t) else t for t in batch["sparse"]]
    if not is_dist and world > 1:
        dense = torch.tensor_split(dense, world, dim=0)[rank]
        labels = torch.tensor_split(labels, world, dim=0)[rank]
    return dense, sparse, labels


def _window(data_iter, P, device, args, rank, world):
    """up to P batches of the next window (fewer at the end of the epoch; None when nothing is left)"""
    dense, sparse, labels = [], [], []
    for _ in range(P):
        try:
            d, s, l = put_data_in_device(next(data_iter), device, args.use_distributed_dataloader, rank, world)
        except StopIteration:
            break
        dense.append(d), sparse.append(s), labels.append(l)
    return (dense, sparse, labels) if dense else None


def _eager_step(model, optimizer, criterion, dense, sparse, labels, keys):
    with phase("forward pass"):                               # the reference's ranges: recsys/dlrm_main.py:268-278
        logits = model(dense, sparse, cache_op=False, presorted=keys).squeeze(-1)
        loss = criterion(logits, labels)
    with phase("backward pass"):
        optimizer.zero_grad()
        loss.backward()
    with phase("optimization"):
        optimizer.step()
    return loss


def lr_changes_after(it: int, total: int, point: float) -> bool:
    """baselines/dlrm_main.py:453-455: checked after iteration `it` (0-based, counted over the whole run) has trained;
    true = the iterations from `it + 1` on train with --lr_after_change_point"""
    return it / total > point


class DenseStep:
    """The dense optimizer step with the learning rate in a device tensor, for --graph_step --change_lr: stock
    torch.optim.SGD / Adagrad turn a tensor lr into a Python scalar (alpha=-lr), which a capture cannot record.  SGD:
    p -= lr * g.  Adagrad with torch's defaults (lr_decay 0, eps 1e-10, initial_accumulator_value 0): s += g * g ;
    p -= lr * g / (sqrt(s) + eps).  _foreach ops that read the tensor on the device; the embedding's fused update reads
    the same one."""

    def __init__(self, params, lr: torch.Tensor, adagrad: bool = False):
        self.params, self.lr = list(params), lr.view(())
        self.sums = [torch.zeros_like(p) for p in self.params] if adagrad else None

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            p.grad = None

    @torch.no_grad()
    def step(self):
        grads = [p.grad for p in self.params]
        if self.sums is not None:
            torch._foreach_addcmul_(self.sums, grads, grads)
            std = torch._foreach_sqrt(self.sums)
            torch._foreach_add_(std, 1e-10)
            grads = torch._foreach_div(grads, std)
        torch._foreach_sub_(self.params, torch._foreach_mul(grads, self.lr))


def _accumulator(args) -> str:
    """accumulator= of the embedding's fused update ("sorted": the in-row layouts' deterministic fold)"""
    if args.embed_sorted_update:
        return "sorted"
    return "step" if args.step_accumulator else "cache"


def check_embed_sorted_update(args):
    """--embed_sorted_update: refused here, before a device is touched"""
    if not args.embed_sorted_update:
        return
    if not (args.adam or args.adam_partial_rowwise or args.adagrad_elementwise):
        raise ValueError("--embed_sorted_update is the deterministic fold of the updates whose state is in the row: pass "
                         "--adam, --adam_partial_rowwise or --adagrad_elementwise (--adagrad has "
                         "--adagrad_deterministic for this)")
    if args.step_accumulator:
        raise ValueError("--embed_sorted_update has no accumulator: not with --step_accumulator")


def make_optimizer(model, args, device, world: int):
    """(optimizer, lr tensor or None): the embedding's fused update is switched on and the optimizer of everything else
    built.  --graph_step --change_lr: both read the rate from one device tensor (DenseStep, set_fused_*(tensor))."""
    embed = model.sparse_modules.embed
    acc = _accumulator(args)
    lr_t = None
    if args.change_lr and args.graph_step:
        lr_t = torch.full((1,), args.learning_rate, dtype=torch.float32, device=device)
    lr = args.learning_rate if lr_t is None else lr_t
    groups = [{"params": list(model.dense_modules.parameters()), "lr": args.learning_rate * world, "lr_scale": world}]
    if args.adam:
        embed.set_fused_adam(lr, betas=(args.adam_beta1, args.adam_beta2), eps=args.eps, accumulator=acc,
                             **_decay(args), **_clip(args))
        return torch.optim.Adam(groups, betas=(args.adam_beta1, args.adam_beta2), eps=args.eps), None
    if args.adagrad_elementwise:
        embed.set_fused_adagrad(lr, accumulator=acc, **_decay(args), **_clip(args))
    elif args.adagrad:
        embed.set_fused_rowwise_adagrad(lr, deterministic=args.adagrad_deterministic, accumulator=acc, **_decay(args),
                                        **_clip(args))
    elif args.fused_sgd:
        embed.set_fused_sgd(lr, accumulator=acc, **_decay(args), **_clip(args))
    else:
        groups.insert(0, {"params": list(model.sparse_modules.parameters()), "lr": args.learning_rate, "lr_scale": 1})
    if lr_t is not None:
        return DenseStep(groups[0]["params"], lr_t, adagrad=args.adagrad or args.adagrad_elementwise), lr_t
    adagrad = args.adagrad or args.adagrad_elementwise
    return (torch.optim.Adagrad(groups) if adagrad else torch.optim.SGD(groups)), None


class LrChange:
    """--change_lr: after the iteration at which lr_changes_after turns true, once -- the device tensor is rewritten
    (--graph_step: the captured step reads it, nothing is captured again), or the dense groups' lr is set in
    param_groups and the fused update set again by value."""

    def __init__(self, args, total: int, optimizer, embed, lr_tensor=None):
        self.args, self.total, self.optimizer, self.embed, self.lr_tensor = args, total, optimizer, embed, lr_tensor
        self.it, self.pending = 0, bool(args.change_lr)

    def after_iteration(self):
        it, self.it = self.it, self.it + 1
        if not self.pending or not lr_changes_after(it, self.total, self.args.lr_change_point):
            return
        self.pending = False
        new, args = self.args.lr_after_change_point, self.args
        print(f"Changing learning rate to: {new}")
        if self.lr_tensor is not None:
            self.lr_tensor.fill_(new)
            return
        for g in self.optimizer.param_groups:
            g["lr"] = new * g.get("lr_scale", 1)
        acc = _accumulator(args)
        if args.adam:
            self.embed.set_fused_adam(new, betas=(args.adam_beta1, args.adam_beta2), eps=args.eps, accumulator=acc,
                                      **_decay(args), **_clip(args))
        elif args.adagrad_elementwise:
            self.embed.set_fused_adagrad(new, accumulator=acc, **_decay(args), **_clip(args))
        elif args.adagrad:
            self.embed.set_fused_rowwise_adagrad(new, deterministic=args.adagrad_deterministic, accumulator=acc,
                                                 **_decay(args), **_clip(args))
        elif args.fused_sgd:
            self.embed.set_fused_sgd(new, accumulator=acc, **_decay(args), **_clip(args))


class _GraphedStep:
    """One training iteration captured in a hipGraph on static inputs (--graph_step): torch.cuda.graph around exactly the
    calls of _eager_step.  The embedding's kernels are launched through the C ABI on the current stream, so they are
    captured with everything else; the slots and the window keys of the batch are copied into static tensors first."""

    def __init__(self, model, optimizer, criterion, dense, sparse, labels, keys):
        from cachedembedding_amd.functional import SrcKeys
        self.dense, self.labels = dense.clone(), labels.clone()
        self.sparse = [sparse[0].clone(), sparse[1].clone(), sparse[2]]
        self.keys = None
        if keys is not None:
            self.keys = SrcKeys(keys.keys.clone(), keys.num_bags, keys.include_last_offset, keys.hook_features, None,
                                keys.identity) if isinstance(keys, SrcKeys) else keys.clone()
        self.model, self.optimizer, self.criterion = model, optimizer, criterion
        optimizer.zero_grad(set_to_none=True)
        # nothing of the pipeline may be in flight on the device while the step is captured, and what the library's swap
        # workers do on their own threads meanwhile (copies, event waits) must not count as part of the capture
        torch.cuda.synchronize()
        model.sparse_modules.embed.cache_weight_mgr.writeback_wait()
        self.graph = torch.cuda.CUDAGraph()
        # captured on the stream the eager iterations ran on (train() leaves the legacy default stream for --graph_step):
        # the gradient accumulators of the dense parameters were created there, and a capture must not wait for another
        # stream's past
        with torch.cuda.graph(self.graph, stream=torch.cuda.current_stream(), capture_error_mode="thread_local"):
            logits = model(self.dense, self.sparse, cache_op=False, presorted=self.keys).squeeze(-1)
            self.loss = criterion(logits, self.labels)
            self.loss.backward()
            optimizer.step()
        # (the capture recorded the step without running it: the caller's eager step on this batch has trained it)

    def step(self, dense, sparse, labels, keys):
        from cachedembedding_amd.functional import SrcKeys
        self.dense.copy_(dense)
        self.labels.copy_(labels)
        self.sparse[0].copy_(sparse[0])
        if self.keys is not None:
            (self.keys.keys if isinstance(self.keys, SrcKeys) else self.keys).copy_(keys.keys if isinstance(keys, SrcKeys) else keys)
        self.graph.replay()
        return self.loss


def train(model, optimizer, loader, args, device, rank, world, record=None, lr_change=None):
    """recsys/dlrm_main.py:206-297 (see _train); --graph_step: on a stream of its own.  lr_change: the run's LrChange"""
    if args.graph_step and torch.cuda.current_stream(device) == torch.cuda.default_stream(device):
        # a step can only be captured on a stream of its own: the whole loop runs there
        main = torch.cuda.Stream(device=device)
        main.wait_stream(torch.cuda.default_stream(device))
        with torch.cuda.stream(main):
            out = train(model, optimizer, loader, args, device, rank, world, record, lr_change)
        torch.cuda.default_stream(device).wait_stream(main)
        return out
    return _train(model, optimizer, loader, args, device, rank, world, record, lr_change)


def _train(model, optimizer, loader, args, device, rank, world, record=None, lr_change=None):
    """recsys/dlrm_main.py:206-297.  record: a list that receives every step's loss (as device scalars: no sync).  Default: the reference's window block (one synchronous prepare_ids per
    prefetch_num batches).  --overlap_cache_op: the cache op of window k+1 runs on a side stream while window k trains
    (pipeline.PrefetchWindow, protect_depth 1, swap traffic through the worker transport when the window is large)."""
    criterion = nn.BCEWithLogitsLoss()
    data_iter = FiniteDataIter(loader, device) if args.use_overlap else iter(loader)
    P = args.prefetch_num
    embed = model.sparse_modules.embed
    layout = None
    if args.window_keys:
        if not ((args.fused_sgd or args.adagrad or args.adam or args.adagrad_elementwise) and args.fold_hook) \
                or world > 1:
            raise ValueError("--window_keys needs --fused_sgd (or --adagrad, or --adam) --fold_hook (one process)")
        F = model.sparse_modules.sparse_feature_num
        offsets = torch.arange(F * args.batch_size + 1, dtype=torch.int32, device=device)     # one id per bag (KJT lengths = 1)
        layout = (offsets, True, F)
    win = PrefetchWindow(embed, P, overlap=args.overlap_cache_op, presort=layout is not None, bag_layout=layout,
                         arrangement=args.arrangement if args.overlap_cache_op else None,
                         arrangement_trial=dict(block_windows=args.arrangement_block_windows, settle=2)
                         if (args.overlap_cache_op and args.arrangement == "auto") else None)
    train.window = win
    graphed = None
    train.graph_captures = 0
    if args.graph_step and (world > 1 or not ((args.fused_sgd or args.adagrad or args.adam or args.adagrad_elementwise)
                                              and args.fold_hook)):
        raise ValueError("--graph_step needs --fused_sgd (or --adagrad) --fold_hook and one process (DDP's bucket hooks "
                         "and the sparse "
                         "COO gradient of the unfused path are not captured)")
    elapsed, done, loss = 0.0, 0, None
    steady = {"t0": None, "done0": 0}
    model.train()
    start = time.time()
    touched = getattr(train, "touched", None)

    def ids_of(window):
        """the window's id tensors, as every form of the cache op below is handed them; --eval_q8_refresh /
        --eval_q4_refresh: they are also marked in the bitmap of the rows looked up since the last evaluation (a row is
        updated only if it was looked up, so these are the rows a served copy has to be given again)"""
        ids = [s[0] for s in window[1]]
        if touched is not None:
            for t in ids:
                touched[t.reshape(-1).long()] = True
        return ids

    cur = _window(data_iter, P, device, args, rank, world)
    if cur is not None and args.overlap_cache_op:
        win.submit(ids_of(cur))
    while cur is not None:
        dense_l, sparse_l, labels_l = cur
        nxt = None
        if args.overlap_cache_op:
            slots = win.collect()
            nxt = _window(data_iter, P, device, args, rank, world)
            if nxt is not None:
                win.submit(ids_of(nxt))
        else:
            slots = win.prepare(ids_of(cur))
        for k in range(len(dense_l)):
            sparse_l[k][0] = slots[k]
            keys_k = win.keys[k] if layout is not None else None
            if graphed is not None and dense_l[k].shape[0] == args.batch_size:
                with phase("forward + backward + optimization (one hipGraph replay)"):
                    loss = graphed.step(dense_l[k], sparse_l[k], labels_l[k], keys_k)
            else:
                loss = _eager_step(model, optimizer, criterion, dense_l[k], sparse_l[k], labels_l[k], keys_k)
                if args.graph_step and graphed is None and done + 1 >= args.graph_after \
                        and dense_l[k].shape[0] == args.batch_size:
                    graphed = _GraphedStep(model, optimizer, criterion, dense_l[k], sparse_l[k], labels_l[k], keys_k)
                    train.graph_captures += 1
            if record is not None:
                record.append(loss.detach().clone() if graphed is not None else loss.detach())
            done += 1
            if lr_change is not None:
                lr_change.after_iteration()
        elapsed += time.time() - start
        start = time.time()
        if steady["t0"] is None and done >= args.warmup_batches:
            torch.cuda.synchronize()                          # the throughput clock starts on an idle GPU
            steady["t0"], steady["done0"] = time.time(), done
            start = steady["t0"]
        cur = nxt if args.overlap_cache_op else _window(data_iter, P, device, args, rank, world)
    torch.cuda.synchronize()
    t_end = time.time()
    if steady["t0"] is not None and done > steady["done0"]:
        train.steady_it_per_s = (done - steady["done0"]) / (t_end - steady["t0"])
        train.steady_iterations = done - steady["done0"]
    else:
        train.steady_it_per_s, train.steady_iterations = float("nan"), 0
    return done, elapsed, float(loss.detach()) if done else float("nan")


class BinaryMetrics:
    """AUROC + accuracy accumulated over an evaluation pass and computed once at its end -- what the reference takes
    from torchmetrics (`metrics.AUROC(compute_on_step=False)`, `metrics.Accuracy(compute_on_step=False)`,
    recsys/dlrm_main.py:303-304), written out because torchmetrics is not part of this image.  Stock torch on whatever
    device the predictions live on; one process-group gather at compute() when there are several ranks."""

    def __init__(self, threshold: float = 0.5):
        self.threshold = threshold
        self.preds: List[torch.Tensor] = []
        self.labels: List[torch.Tensor] = []

    def __call__(self, preds: torch.Tensor, labels: torch.Tensor) -> None:
        self.preds.append(preds.detach().reshape(-1).float())
        self.labels.append(labels.detach().reshape(-1).to(torch.int32))

    @staticmethod
    def auroc(preds: torch.Tensor, labels: torch.Tensor) -> float:
        """Area under the ROC curve with tied scores joined by straight segments (the trapezoid torchmetrics / sklearn
        integrate) = the Mann-Whitney statistic with AVERAGE ranks over ties: (sum of the positives' ranks -
        P (P + 1) / 2) / (P N).  NaN when one class is absent."""
        n = preds.numel()
        pos = int((labels != 0).sum())
        if n == 0 or pos == 0 or pos == n:
            return float("nan")
        order = torch.argsort(preds)
        p, y = preds[order], (labels[order] != 0).double()
        new = torch.ones(n, dtype=torch.bool, device=p.device)
        new[1:] = p[1:] != p[:-1]
        gid = torch.cumsum(new, 0) - 1                                  # tie group of every sorted position
        ranks = torch.arange(1, n + 1, dtype=torch.float64, device=p.device)
        gsum = torch.zeros(int(gid[-1]) + 1, dtype=torch.float64, device=p.device).index_add_(0, gid, ranks)
        avg = (gsum / torch.bincount(gid).double())[gid]
        return float(((avg * y).sum() - pos * (pos + 1) / 2.0) / (float(pos) * float(n - pos)))

    def gathered(self):
        """every rank's predictions and labels (the ranks evaluate different slices of a batch / of the set)"""
        preds = torch.cat(self.preds) if self.preds else torch.zeros(0)
        labels = torch.cat(self.labels) if self.labels else torch.zeros(0, dtype=torch.int32)
        if dist.is_initialized() and dist.get_world_size() > 1:
            W = dist.get_world_size()
            cnt = torch.tensor([preds.numel()], dtype=torch.int64, device=preds.device)
            cnts = [torch.zeros_like(cnt) for _ in range(W)]
            dist.all_gather(cnts, cnt)
            cap = max(int(c) for c in cnts)
            pp = torch.zeros(cap, dtype=torch.float32, device=preds.device)
            ll = torch.zeros(cap, dtype=torch.int32, device=preds.device)
            pp[:preds.numel()], ll[:labels.numel()] = preds, labels
            gp = [torch.zeros_like(pp) for _ in range(W)]
            gl = [torch.zeros_like(ll) for _ in range(W)]
            dist.all_gather(gp, pp)
            dist.all_gather(gl, ll)
            preds = torch.cat([g[:int(c)] for g, c in zip(gp, cnts)])
            labels = torch.cat([g[:int(c)] for g, c in zip(gl, cnts)])
        return preds, labels

    def compute(self):
        preds, labels = self.gathered()
        if preds.numel() == 0:
            return float("nan"), float("nan")
        acc = float(((preds >= self.threshold) == (labels != 0)).double().mean())
        return self.auroc(preds, labels), acc


def _evaluate(model, loader, stage, args, device, rank, world):
    """recsys/dlrm_main.py:300-333: model.eval(), no gradients, the module's own cache op per batch (`model(dense,
    sparse)`: prepare_ids on the batch's ids, then the gather -- evaluation rows are admitted and evicted like training
    rows, nothing is updated), sigmoid of the logits into AUROC and accuracy.  Returns (auroc, accuracy)."""
    model.eval()
    meter = BinaryMetrics()
    data_iter = FiniteDataIter(loader, device) if args.use_overlap else iter(loader)
    n = 0
    with torch.no_grad():
        for batch in data_iter:
            dense, sparse, labels = put_data_in_device(batch, device, args.use_distributed_dataloader, rank, world)
            logits = model(dense, sparse).squeeze(-1)
            meter(torch.sigmoid(logits), labels.int())
            n += 1
    auroc, acc = meter.compute()
    if rank == 0:
        print(f"AUROC over {stage} set: {auroc}")
        print(f"Accuracy over {stage} set: {acc}")
    _evaluate.batches = n
    return auroc, acc


def _decay(args) -> dict:
    """the keywords every set_fused_* takes for --embed_weight_decay / --embed_weight_decay_mode"""
    return {"weight_decay": args.embed_weight_decay, "weight_decay_mode": args.embed_weight_decay_mode}


def _clip(args) -> dict:
    """the keywords every set_fused_* takes for --embed_grad_clip / --embed_grad_clip_mode"""
    return {"grad_clip": args.embed_grad_clip, "grad_clip_mode": args.embed_grad_clip_mode}


def _fused_update(args) -> tuple:
    """(the name the library's check_* functions know the chosen fused update by, the table's dtype).  The updates
    whose state travels in the row (--adam, --adagrad_elementwise) go by the Adam entries' rules."""
    table = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[args.table_dtype]
    in_row = args.adam or args.adagrad_elementwise
    return "adam" if in_row else "rowwise_adagrad" if args.adagrad else "sgd", table


def check_embed_weight_decay(args):
    """--embed_weight_decay: refused here, before a device is touched, with the library's own refusals"""
    from cachedembedding_amd.functional import check_weight_decay, check_weight_decay_path
    wd = check_weight_decay(args.embed_weight_decay, args.embed_weight_decay_mode)
    if not wd:
        return
    if not (args.adagrad or args.adam or args.fused_sgd or args.adagrad_elementwise):
        raise ValueError("--embed_weight_decay decays the rows inside a fused update: pass --adagrad, --adam or "
                         "--fused_sgd")
    check_weight_decay_path(*_fused_update(args), wd, bool(args.adagrad_deterministic))


def check_embed_grad_clip(args):
    """--embed_grad_clip: refused here, before a device is touched, with the library's own refusals"""
    from cachedembedding_amd.functional import check_grad_clip, check_grad_clip_path
    clip = check_grad_clip(args.embed_grad_clip, args.embed_grad_clip_mode)
    if clip is None:
        return
    if not (args.adagrad or args.adam or args.fused_sgd or args.adagrad_elementwise):
        raise ValueError("--embed_grad_clip clips a row's gradient inside a fused update: pass --adagrad, --adam or "
                         "--fused_sgd")
    check_grad_clip_path(*_fused_update(args), clip, bool(args.adagrad_deterministic))


def check_step_accumulator(args):
    """--step_accumulator: refused here, before a device is touched, with the library's own refusals"""
    from cachedembedding_amd.functional import check_accumulator
    if args.adam or args.adagrad_elementwise:
        return                                      # (both accumulators serve the updates whose state is in the row)
    if not (args.adagrad or args.fused_sgd):
        raise ValueError("--step_accumulator sizes the accumulator of a fused update: pass --adagrad, or --fused_sgd "
                         "with a 16-bit --table_dtype")
    check_accumulator(*_fused_update(args), "step", bool(args.adagrad_deterministic), args.weight_rounding)


def main(argv=None):
    args = parse_args(argv)
    if args.adagrad_deterministic and not args.adagrad:
        raise ValueError("--adagrad_deterministic chooses how --adagrad folds the gradient: pass --adagrad as well")
    if args.adagrad_deterministic and args.table_dtype != "fp32" and args.weight_rounding == "stochastic":
        raise NotImplementedError("--adagrad_deterministic rounds a 16-bit table to nearest: pass --weight_rounding nearest")
    check_embed_sorted_update(args)
    if args.step_accumulator:
        check_step_accumulator(args)
    check_embed_weight_decay(args)
    check_embed_grad_clip(args)
    if args.change_lr and args.graph_step and args.adagrad_deterministic:
        raise NotImplementedError("--graph_step --change_lr keeps the learning rate in a device tensor, which the "
                                  "sorted update (--adagrad_deterministic) does not read")
    if not args.use_cache:
        raise NotImplementedError("Other EmbeddingBags are under development")   # recsys/models/dlrm.py:83-84
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    check_output_dtype(args, world)
    if args.eval_q8:
        if not args.eval_acc:
            raise ValueError("--eval_q8 needs --eval_acc: it evaluates the test set a second time, through the "
                             "quantized table")
        if world > 1 or args.use_tablewise:
            raise NotImplementedError("--eval_q8 is implemented for one process without --use_tablewise (the sharded "
                                      "classes do not take a q8 table)")
    if args.eval_q4:
        if not args.eval_acc:
            raise ValueError("--eval_q4 needs --eval_acc: it evaluates the test set once more, through the "
                             "quantized table")
        if world > 1 or args.use_tablewise:
            raise NotImplementedError("--eval_q4 is implemented for one process without --use_tablewise (the sharded "
                                      "classes do not take a q4 table)")
    for flag, on in (("--eval_q8_refresh", args.eval_q8_refresh), ("--eval_q4_refresh", args.eval_q4_refresh)):
        if on and not args.eval_acc:
            raise ValueError(f"{flag} needs --eval_acc: it evaluates the validation and the test set once more, through "
                             "the served quantized table")
        if on and (world > 1 or args.use_tablewise):
            raise NotImplementedError(f"{flag} is implemented for one process without --use_tablewise (rows are "
                                      "refreshed in, and read from, a single-process CachedEmbeddingBag)")
    if args.adam_partial_rowwise and not args.adam:
        raise ValueError("--adam_partial_rowwise chooses the layout of --adam: pass --adam with it")
    if args.adagrad_elementwise:
        if args.adagrad or args.adam or args.fused_sgd:
            raise ValueError("--adagrad_elementwise takes the place of --adagrad, of --adam and of --fused_sgd: pass one "
                             "of them")
        if world > 1 or args.use_tablewise:
            raise NotImplementedError("--adagrad_elementwise is implemented for one process without --use_tablewise "
                                      "(the sharded classes do not take a table whose rows carry optimizer state)")
        if args.table_dtype != "fp32":
            raise NotImplementedError("--adagrad_elementwise needs --table_dtype fp32: the rows carry fp32 sums of "
                                      "squares")
        if args.use_sparse_embed_grad:
            raise NotImplementedError("--adagrad_elementwise with --use_sparse_embed_grad: the fused update hands torch "
                                      "no gradient")
    if args.adam:
        if args.adagrad or args.fused_sgd:
            raise ValueError("--adam takes the place of --adagrad and of --fused_sgd: pass one of them")
        if world > 1 or args.use_tablewise:
            raise NotImplementedError("--adam is implemented for one process without --use_tablewise (the sharded "
                                      "classes do not take an Adam-layout table)")
        if args.table_dtype != "fp32":
            raise NotImplementedError("--adam needs --table_dtype fp32: the Adam layout is an fp32 table")
        if args.use_sparse_embed_grad:
            raise NotImplementedError("--adam with --use_sparse_embed_grad: the fused update hands torch no gradient")
        if args.graph_step and args.change_lr:
            raise NotImplementedError("--adam with --graph_step --change_lr: torch.optim.Adam of the dense part reads "
                                      "its rate on the host")
    if args.adagrad:
        if args.fused_sgd:
            raise ValueError("--adagrad takes the place of --fused_sgd: pass one of them")
        if world > 1 or args.use_tablewise:
            # the row-wise accumulator needs the whole row's gradient on one device: the model-parallel layouts of
            # this trainer split the rows' columns over the ranks (or the tables over them)
            raise NotImplementedError("--adagrad is implemented for one process without --use_tablewise (sharded "
                                      "embeddings keep the fused SGD only)")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device)
    torch.manual_seed(args.seed)
    if args.tunable_gemm:
        import torch.cuda.tunable as tunable
        tunable.enable(True)
        tunable.tuning_enable(True)
        tunable.set_max_tuning_duration(50)                   # ms per solution: a dozen shapes, seconds in all
        tunable.set_filename(os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ce_dlrm_tunableop_{rank}.csv"))
    sizes = synthetic.TABLES[args.dataset]
    if args.num_embeddings_per_feature:
        sizes = [int(x) for x in args.num_embeddings_per_feature.split(",")]
    if args.table_scale != 1.0:
        sizes = synthetic.scale_tables(sizes, args.table_scale)
    freq = None
    loader = None
    if args.dataset_dir:
        from cachedembedding_amd.datasets import BinaryCriteoNpy, criteo_files, get_id_freq_map
        if args.use_tablewise:
            raise NotImplementedError("--dataset_dir with --use_tablewise: pass assigned_tables per rank")
        dense_f, sparse_f, labels_f = criteo_files(args.dataset_dir, "train")
        dist_loader = args.use_distributed_dataloader
        loader = BinaryCriteoNpy(dense_f, sparse_f, labels_f, args.batch_size, rank if dist_loader else 0,
                                 world if dist_loader else 1, shuffle_batches=args.shuffle_batches,
                                 mmap_mode=args.mmap_mode, hashes=sizes, seed=args.seed)
        if args.use_freq:
            freq = get_id_freq_map(sparse_f, sizes, os.path.join(args.dataset_dir, "id_freq_map.pt"))
    elif args.use_freq:
        freq = synthetic.SyntheticKJT(sizes, args.batch_size, 1, "power_law", 0.25, seed=args.seed + 1,
                                      device=device).id_freq_map(32)
    model = HybridParallelDLRM(sizes, args, freq, device)
    embed = model.sparse_modules.embed
    embed.set_cache_mgr_async_copy(args.use_cache_mgr_async_copy)
    if args.table_dtype != "fp32":
        embed.set_weight_rounding(args.weight_rounding, seed=args.seed)
    optimizer, lr_tensor = make_optimizer(model, args, device, world)
    if loader is None:
        loader = SyntheticLoader(sizes, args.batch_size, args.num_dense_features, args.limit_train_batches,
                                 args.seed + 17)
    elif args.limit_train_batches:
        loader = _Limit(loader, args.limit_train_batches)
    val_loader = test_loader = None
    if args.eval_acc:
        # recsys/dlrm_main.py:411-412 + recsys/datasets/criteo.py:386-391: val = the first half of the held-out day,
        # test = the other half (rank r of 2W and rank r + W of 2W); synthetic: two more seeded streams of the same tables
        if args.dataset_dir:
            held = criteo_files(args.dataset_dir, "val")
            r, w = (rank, world) if args.use_distributed_dataloader else (0, 1)
            val_loader, test_loader = (BinaryCriteoNpy(*held, args.batch_size, rr, 2 * w, mmap_mode=args.mmap_mode,
                                                       hashes=sizes, seed=args.seed) for rr in (r, r + w))
        else:
            val_loader, test_loader = (SyntheticLoader(sizes, args.batch_size, args.num_dense_features, n or 8,
                                                       args.seed + off)
                                       for n, off in ((args.limit_val_batches, 29), (args.limit_test_batches, 43)))
        if args.limit_val_batches:
            val_loader = _Limit(val_loader, args.limit_val_batches)
        if args.limit_test_batches:
            test_loader = _Limit(test_loader, args.limit_test_batches)
    results = {"val_aurocs": [], "val_accuracies": [], "test_auroc": None, "test_accuracy": None}   # TrainValTestResults
    main.results, main.model, main.val_loader, main.test_loader = results, model, val_loader, test_loader
    lr_change = LrChange(args, len(loader) * args.epochs, optimizer, embed, lr_tensor) if args.change_lr else None
    # --eval_q8_refresh / --eval_q4_refresh: the served copies are built once, here, from the untrained table; from then
    # on they only ever receive the rows the training loop marked (train.touched, one bool per id, on the device)
    served = {bits: embed.quantized(bits=bits)
              for bits, on in ((8, args.eval_q8_refresh), (4, args.eval_q4_refresh)) if on}
    train.touched = torch.zeros(embed.num_embeddings, dtype=torch.bool, device=device) if served else None
    main.served = served

    def evaluate_served(loader_, stage, into):
        """bring every served copy up to date with the rows marked since the last evaluation, then evaluate through it"""
        ids = torch.nonzero(train.touched).view(-1)
        train.touched.zero_()
        sparse = model.sparse_modules
        for bits, module in served.items():
            module.refresh_from(embed, ids)
            sparse.embed = module
            try:
                auroc, acc = _evaluate(model, loader_, f"{stage} (q{bits} table, refreshed)", args, device, rank, world)
            finally:
                sparse.embed = embed
            into(bits, auroc, acc, int(ids.numel()))

    for bits in served:
        results.update({f"val_aurocs_q{bits}_refresh": [], f"refreshed_rows_q{bits}": []})
    for epoch in range(args.epochs):
        rec = []
        done, elapsed, loss = train(model, optimizer, loader, args, device, rank, world, record=rec,
                                    lr_change=lr_change)
        if args.eval_acc:                                        # recsys/dlrm_main.py:358-363
            auroc, acc = _evaluate(model, val_loader, "val", args, device, rank, world)
            results["val_aurocs"].append(auroc)
            results["val_accuracies"].append(acc)
            if served:
                evaluate_served(val_loader, "val", lambda bits, auroc_q, _acc, n: (
                    results[f"val_aurocs_q{bits}_refresh"].append(auroc_q), results[f"refreshed_rows_q{bits}"].append(n)))
        if rank == 0:
            lookups = done * args.batch_size * len(sizes)
            q = max(1, len(rec) // 4)
            head = float(torch.stack(rec[:q]).mean()) if rec else float("nan")
            tail = float(torch.stack(rec[-q:]).mean()) if rec else float("nan")
            print(f"epoch {epoch}: {done} iterations, average throughput: {done / max(elapsed, 1e-9):.2f} it/s, "
                  f"{lookups / max(elapsed, 1e-9) / 1e6:.1f} M lookups/s, last loss {loss:.4f}, "
                  f"mean loss first quarter {head:.4f} last quarter {tail:.4f}")
            print(f"         steady state (after {args.warmup_batches} iterations, GPU-synchronised at both ends): "
                  f"{train.steady_it_per_s:.2f} it/s over {train.steady_iterations} iterations, "
                  f"{train.steady_it_per_s * args.batch_size * len(sizes) / 1e6:.1f} M lookups/s")
            embed.print_comm_stats_()
            if args.json_out:
                import json
                mgr = embed.cache_weight_mgr
                Path(args.json_out).write_text(json.dumps({
                    "script": "examples/dlrm_main.py", "dataset": args.dataset, "table_scale": args.table_scale,
                    "num_embeddings": int(sum(sizes)), "embedding_dim": args.embedding_dim, "features": len(sizes),
                    "batch_size": args.batch_size, "prefetch_num": args.prefetch_num, "cache_ratio": args.cache_ratio,
                    "cuda_row_num": int(mgr.cuda_row_num), "dense_arch": args.dense_arch_layer_sizes,
                    "over_arch": args.over_arch_layer_sizes, "dtype": "f32", "embedding_output_dtype": args.embedding_output_dtype,
                    "table_dtype": args.table_dtype,
                    "data": "synthetic",
                    "surface": {k: bool(getattr(args, k)) for k in ("use_overlap", "overlap_cache_op", "fused_sgd",
                                                                    "adagrad", "fold_hook", "window_keys", "tunable_gemm", "graph_step",
                                                                    "use_sparse_embed_grad", "use_lfu", "use_lru", "use_freq")},
                    "transport": mgr.transport_name, "iterations": done, "warmup_iterations": args.warmup_batches,
                    "it_per_s": train.steady_it_per_s, "it_per_s_scope": "whole model: data iterator + cache op + "
                    "embedding forward + dense forward + loss + backward + optimizer step",
                    "lookups_per_s": train.steady_it_per_s * args.batch_size * len(sizes),
                    "ms_per_iteration": 1e3 / train.steady_it_per_s,
                    "arrangement": (train.window.trial.report() | {"mode": train.window.arrangement}
                                    if train.window.trial is not None else {"mode": train.window.arrangement}),
                    # the reference's own "average throughput" print (recsys/dlrm_main.py:297): iterations over the
                    # HOST time of the whole epoch, i.e. including the first `warmup_iterations` iterations (library
                    # initialisation, GEMM algorithm search, pipeline fill -- seconds, for a run of a few hundred
                    # iterations) and without a GPU synchronisation at the end.  Not comparable with it_per_s, which
                    # is bracketed by synchronisation and starts after the warm-up; kept because the reference prints it.
                    "it_per_s_reference_print_host_clock_incl_warmup": done / max(elapsed, 1e-9),
                    "loss_first_quarter": head, "loss_last_quarter": tail,
                    "eval": ({"val_auroc": results["val_aurocs"][-1], "val_accuracy": results["val_accuracies"][-1],
                              "val_batches": _evaluate.batches} if args.eval_acc else None)}, indent=1))
    if args.eval_acc:                                            # recsys/dlrm_main.py:365-369
        results["test_auroc"], results["test_accuracy"] = _evaluate(model, test_loader, "test", args, device, rank, world)
        if served:
            import json
            evaluate_served(test_loader, "test", lambda bits, auroc_q, acc_q, n: (
                results.update({f"test_auroc_q{bits}_refresh": auroc_q, f"test_accuracy_q{bits}_refresh": acc_q}),
                results[f"refreshed_rows_q{bits}"].append(n)))
            print(json.dumps({"script": "examples/dlrm_main.py", "test_auroc": results["test_auroc"]} | {
                k: v for k, v in results.items() if k.endswith("_refresh") or k.startswith("refreshed_rows")}))
    for bits in [b for b, on in ((8, args.eval_q8), (4, args.eval_q4)) if on]:
        # serve what was trained at a quarter (q8) or a sixth (q4, D = 128) of the memory: the same dense weights over
        # the row-wise quantized copy of the table (a new pinned table and a cache of its own; the trained module is
        # only flushed)
        import json
        sparse = model.sparse_modules
        tag = f"q{bits}"
        quant = embed.quantized() if bits == 8 else embed.quantized(bits=bits)
        sparse.embed = quant
        try:
            auroc, acc = _evaluate(model, test_loader, f"test ({tag} table)", args, device, rank, world)
        finally:
            sparse.embed = embed
        table, table_q = embed.weight, quant.weight
        extra = {f"test_auroc_{tag}": auroc, f"test_accuracy_{tag}": acc,
                 "table_bytes": table.numel() * table.element_size(), f"table_bytes_{tag}": table_q.numel()}
        results.update(extra)
        print(json.dumps({"script": "examples/dlrm_main.py", "test_auroc": results["test_auroc"],
                          "test_accuracy": results["test_accuracy"], **extra}))
        if args.json_out and Path(args.json_out).exists():
            Path(args.json_out).write_text(json.dumps(json.loads(Path(args.json_out).read_text()) | extra, indent=1))
        del quant
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
