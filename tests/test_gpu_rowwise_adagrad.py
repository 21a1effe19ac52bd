"""GPU tests of the fused exact row-wise Adagrad (ce_bag_adagrad.hip) against the numpy reference
(tests/rowwise_adagrad_ref.py): the kernels alone, through the cache while it evicts, under the prefetch windows and a
hipGraph replay, and the example trainer's --adagrad against a torch-CPU model."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))

import rowwise_adagrad_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
U = np.finfo(np.float32).eps / 2


def _bounds(rows, grads, R):
    """per row: lookups in the step, sum |terms| and |folded g| (max over d) -- the fp32 accumulation bound's inputs"""
    cnt = np.bincount(rows, minlength=R)
    s = np.zeros((R, grads.shape[1]))
    np.add.at(s, rows, np.abs(grads))
    g = np.zeros((R, grads.shape[1]))
    np.add.at(g, rows, grads)
    return cnt, s.max(axis=1), np.abs(g).max(axis=1)


class _Track:
    """fp64 reference state + per-row tolerances accumulated over the steps"""

    def __init__(self, W0, N, lr, eps=1e-8, row_of=None):
        self.W, self.M = W0.astype(np.float64).copy(), np.zeros(N)
        self.lr, self.eps, self.row_of = lr, eps, row_of
        R = W0.shape[0]
        self.tol_w, self.tol_m = np.zeros(R), np.zeros(N)
        self.multi = np.zeros(R, bool)
        self.touched = np.zeros(R, bool)

    def step(self, rows, grads):
        R = self.W.shape[0]
        D = self.W.shape[1]
        cnt, s, gmax = _bounds(rows, grads, R)
        ref.step(self.W, self.M, rows, grads, self.lr, self.eps)
        idx = np.arange(R) if self.row_of is None else self.row_of
        m_now = np.maximum(self.M[idx], 1e-30)
        t = cnt > 0
        self.touched |= t
        self.multi |= cnt > 1
        # |fp32 fold - exact| <= (n - 1) u S per element (recursive summation): it moves m by <= 2 |g| e (+ the
        # rounding of a D-term sum of squares and of the add), and the update lr g / sqrt(m) by <= lr e / sqrt(m) plus
        # |update| * dm / (2 m), |update| <= lr sqrt(D)
        e = np.maximum(cnt - 1, 0) * U * s
        dm = 2 * gmax * e * 2 + 4 * (D + 2) * U * m_now
        dw = 2 * self.lr * e / np.sqrt(m_now) + self.lr * np.sqrt(D) * dm / m_now + 8 * self.lr * U * np.sqrt(D)
        self.tol_w += np.where(t, dw, 0)
        self.tol_m[idx[t]] += dm[t]

    def check(self, W, M):
        W, M = np.asarray(W, np.float64), np.asarray(M, np.float64)
        once = self.touched & ~self.multi
        np.testing.assert_allclose(W[once], self.W[once], rtol=1e-5, atol=1e-6)
        err = np.abs(W - self.W)
        lim = self.tol_w[:, None] + 1e-5 * np.abs(self.W) + 1e-6
        bad = np.nonzero(self.touched & (err > lim).any(1))[0]
        assert bad.size == 0, (bad[:5], err[bad[:5]].max(1), lim[bad[:5]].min(1))
        bad = np.nonzero(np.abs(M - self.M) > self.tol_m + 1e-6 * np.abs(self.M))[0]
        assert bad.size == 0, (bad[:5], M[bad[:5]], self.M[bad[:5]], self.tol_m[bad[:5]])


@pytest.mark.parametrize("D", [128, 6])
@pytest.mark.parametrize("form", ["sum", "mean", "psw", "padding", "src"])
def test_kernels_against_fp64_reference(form, D):
    """nnz = 4 segments of 16384 lookups; rows 0..7 hot (in every segment), 8000 rows seen once, 1000 never looked up"""
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, embedding_bag, presort_window
    rng = np.random.default_rng(7)
    R, K, lr, F = 60000, 3, 0.05, 4
    nnz = 4 * 16384
    W0 = rng.standard_normal((R, D)).astype(np.float32)
    w = torch.from_numpy(W0).cuda()
    mom = torch.zeros(R, device="cuda")
    fused = FusedRowwiseAdagrad(lr, momentum=mom)
    track = _Track(W0, R, lr)
    never = np.arange(R - 1000, R)
    for k in range(K):
        ids = rng.integers(8, R - 1000, nnz)
        hot = rng.random(nnz) < 0.25
        ids[hot] = rng.integers(0, 8, int(hot.sum()))
        psw = None
        if form in ("sum", "psw", "src", "padding"):
            off = np.arange(nnz + 1)                                 # one id per bag, [B, F] output
            hook = F
        else:
            off = np.concatenate([np.sort(rng.choice(np.arange(1, nnz), nnz // 3 - 1, replace=False)), [0, nnz]])
            off = np.unique(off)
            hook = 0
        nb = len(off) - 1
        go = rng.standard_normal((nb // F, F, D) if hook else (nb, D)).astype(np.float32)
        if form == "psw":
            psw = rng.random(nnz).astype(np.float32)
        slots = ids.copy()
        if form == "padding":
            slots[rng.random(nnz) < 0.1] = -1                         # ignored lookups
        kw = dict(mode="mean" if form == "mean" else "sum", include_last_offset=True, hook_features=hook)
        rows, grads = ref.lookup_grads(slots, off, go, R, psw=psw, **kw)
        idx = torch.from_numpy(slots).cuda()
        offs = torch.from_numpy(off).cuda()
        pre = None
        if form == "src":
            pre = presort_window(idx.view(1, -1), R, offsets=offs.to(torch.int32), include_last_offset=True,
                                 hook_features=hook, identity_bags=True)[0]
        w.requires_grad_(True)
        o = embedding_bag(idx, w, offs, mode=kw["mode"], include_last_offset=True,
                          per_sample_weights=None if psw is None else torch.from_numpy(psw).cuda(),
                          hook_features=hook, fused_sgd=fused, presorted=pre, masked_indices=form == "padding")
        o.backward(torch.from_numpy(go).cuda().view_as(o))
        assert w.grad is None                                         # the update happened inside backward
        w.requires_grad_(False)
        track.step(rows, grads)
    torch.cuda.synchronize()
    Wg, Mg = w.cpu().numpy(), mom.cpu().numpy()
    assert np.array_equal(Wg[never], W0[never]) and np.all(Mg[never] == 0)
    assert track.multi[:8].all() and (track.touched & ~track.multi).sum() > 1000
    track.check(Wg, Mg)
    ws = fused._ws
    assert int(torch.count_nonzero(ws)) == 0, "the workspace must be left zero-filled"


def _cached(N, D, C, strategy, freq, W0):
    import cachedembedding_amd as ce
    emb = ce.CachedEmbeddingBag(N, D, sparse=True, _weight=torch.from_numpy(W0.copy()), mode="sum",
                                include_last_offset=True, cuda_row_num=C, ids_freq_mapping=freq, warmup_ratio=0.5,
                                evict_strategy=strategy, strict=False)
    return emb


@pytest.mark.parametrize("strategy", ["dataset_freq", "lfu"])
def test_through_cache_that_evicts(strategy):
    """3 % cache, 24 steps, then flush(): host table and momentum1 equal a full-table run of the reference"""
    import cachedembedding_amd as ce
    rng = np.random.default_rng(11)
    N, D, F, B, lr = 20000, 32, 4, 128, 0.1
    C = int(0.03 * N)
    W0 = rng.standard_normal((N, D)).astype(np.float32)
    freq = rng.integers(0, 100, N) if strategy == "dataset_freq" else None
    st = ce.EvictionStrategy.DATASET if strategy == "dataset_freq" else ce.EvictionStrategy.LFU
    emb = _cached(N, D, C, st, freq, W0)
    mgr = emb.cache_weight_mgr
    emb.set_fused_sgd(lr)
    with pytest.raises(ValueError):
        emb.set_fused_rowwise_adagrad(lr)
    emb.set_fused_sgd(None)
    emb.set_fused_rowwise_adagrad(lr)
    with pytest.raises(ValueError):
        emb.set_fused_sgd(lr)
    assert mgr.momentum1.shape == (N,) and int(torch.count_nonzero(mgr.momentum1)) == 0
    # the state of id i lives in host-table row idx_map[i] (cpu_row_idx), the weight's and momentum1's common index;
    # the reference runs in that row space over the table as constructed
    imap = mgr.idx_map.cpu().numpy().astype(np.int64)
    track = _Track(W0, N, lr)
    off = torch.arange(F * B + 1, device="cuda")
    for it in range(24):
        ids = (rng.random(F * B) ** 2 * N).astype(np.int64)
        go = rng.standard_normal((B, F, D)).astype(np.float32)
        out = emb(torch.from_numpy(ids).cuda(), off, hook_features=F)
        out.backward(torch.from_numpy(go).cuda())
        rows, grads = ref.lookup_grads(ids, np.arange(F * B + 1), go, N, hook_features=F)
        track.step(imap[rows], grads)
    torch.cuda.synchronize()
    assert mgr.cuda_cached_weight.grad is None
    assert sum(emb.num_write_back_history) > 0, "the cache never evicted"
    if strategy == "dataset_freq":
        assert not np.array_equal(imap, np.arange(N))
    emb.flush()
    track.check(mgr.weight.numpy(), mgr.momentum1.cpu().numpy())


@pytest.mark.parametrize("mode", ["overlap", "interleaved", "graph"])
def test_prefetch_and_graphed_windows(mode):
    """PrefetchWindow (both arrangements, source-row keys: the streaming form) and GraphedWindow (hipGraph replay) on a
    cache that evicts between windows: the same trajectory as the reference over the full table"""
    import cachedembedding_amd as ce
    from cachedembedding_amd.pipeline import GraphedWindow, PrefetchWindow
    rng = np.random.default_rng(5)
    N, D, F, B, P, lr, nwin = 20000, 64, 4, 64, 4, 0.05, 6
    W0 = rng.standard_normal((N, D)).astype(np.float32)
    emb = ce.CachedEmbeddingBag(N, D, sparse=True, _weight=torch.from_numpy(W0.copy()), mode="sum",
                                include_last_offset=True, cuda_row_num=2 * F * B * P, warmup_ratio=0.5, strict=False)
    emb.set_fused_rowwise_adagrad(lr)
    emb.set_cache_op(False)
    off = torch.arange(F * B + 1, dtype=torch.int32, device="cuda")
    layout = (off, True, F)
    go = (rng.standard_normal((B, F, D)) * 0.1).astype(np.float32)
    grad = torch.from_numpy(go).cuda()
    windows = [[(torch.from_numpy(rng.random(F * B) ** 3 * N).long().clamp_(0, N - 1)) for _ in range(P)]
               for _ in range(nwin)]
    track = _Track(W0, N, lr)
    offs_np = np.arange(F * B + 1)

    def ref_batch(v):
        rows, grads = ref.lookup_grads(v.numpy(), offs_np, go, N, hook_features=F)
        track.step(rows, grads)

    def step(slots, i, keys=None):
        out = emb(slots, off, hook_features=F, presorted=keys)
        out.backward(grad)

    if mode == "graph":
        gw = GraphedWindow(emb, P, F * B, step, overlap=True, warmup_values=[v.cuda() for v in windows[0]],
                           presort=True, transport="worker", bag_layout=layout, arrangement="overlap")
        for v in windows[0]:                     # the capture's eager warm-up trained on window 0 once
            ref_batch(v)
        gw.submit([v.cuda() for v in windows[0]], 0)
        for w in range(nwin):
            if w + 1 < nwin:
                gw.submit([v.cuda() for v in windows[w + 1]], (w + 1) % 2)
            gw.run(w % 2)
    else:
        win = PrefetchWindow(emb, P, overlap=True, presort=True, transport="worker", bag_layout=layout,
                             arrangement=mode)
        win.submit([v.cuda() for v in windows[0]])
        for w in range(nwin):
            slots = win.collect()
            if w + 1 < nwin:
                win.submit([v.cuda() for v in windows[w + 1]])
            for i in range(P):
                step(slots[i], i, win.keys[i])
    for w in range(nwin):
        for v in windows[w]:
            ref_batch(v)
    torch.cuda.synchronize()
    mgr = emb.cache_weight_mgr
    assert mgr.sync_stats().status == 0
    assert sum(emb.num_write_back_history) > 0, "the cache never evicted"
    emb.flush()
    assert np.array_equal(mgr.idx_map.cpu().numpy(), np.arange(N))        # no frequency map: rows are ids
    track.check(mgr.weight.numpy(), mgr.momentum1.cpu().numpy())


def test_refusals_on_the_device():
    import cachedembedding_amd as ce
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, embedding_bag
    N, D = 1000, 16
    emb = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=100)
    emb.set_fused_rowwise_adagrad(0.1)
    ids = torch.arange(8, device="cuda")
    off = torch.arange(9, device="cuda")
    before = emb.cache_weight_mgr.cuda_cached_weight.detach().clone()
    psw = torch.ones(8, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="per_sample_weights"):
        emb(ids, off, per_sample_weights=psw)
    emb.set_cache_op(False)
    tail = emb.cache_weight_mgr.reserve_tail(16)
    big = emb.cache_weight_mgr.cache_with_tail
    with pytest.raises(NotImplementedError, match=r"outside \[0, C\)"):
        embedding_bag(ids, big, off, mode="sum", include_last_offset=True, fused_sgd=emb.fused_adagrad)
    emb.set_fused_rowwise_adagrad(None)
    emb.set_fused_sgd(0.1)
    assert tail.shape == (16, D) and before.shape == (100, D)
    assert isinstance(emb.fused_adagrad, FusedRowwiseAdagrad)


# ---- the example trainer: --adagrad against a torch-CPU model ------------------------------------------------------

_VARIANTS = {"eager": [], "window_keys": ["--overlap_cache_op", "--fold_hook", "--window_keys"],
             "graph_step": ["--overlap_cache_op", "--fold_hook", "--window_keys", "--graph_step", "--graph_after", "3"]}


def _child(variant: str, out: str) -> None:
    """runs in a child process: the toy DLRM of tests/golden/dlrm_toy.npz trained by examples/dlrm_main.py's loop"""
    sys.path.insert(0, str(ROOT / "examples"))
    sys.path.insert(0, str(ROOT))
    import importlib
    dm = importlib.import_module("dlrm_main")
    gold = np.load(ROOT / "tests" / "golden" / "dlrm_toy.npz")
    sizes = [int(x) for x in gold["sizes"]]
    steps, B = gold["dense_x"].shape[0], gold["dense_x"].shape[1]
    D = gold["table"].shape[1]
    lr = float(gold["lr"])
    args = dm.parse_args(["--use_cache", "--cache_ratio", "0.4", "--prefetch_num", "4", "--use_sparse_embed_grad",
                          "--embedding_dim", str(D), "--batch_size", str(B), "--learning_rate", str(lr), "--adagrad",
                          "--dense_arch_layer_sizes", ",".join(str(int(x)) for x in gold["dense_arch"]),
                          "--over_arch_layer_sizes", ",".join(str(int(x)) for x in gold["over_arch"])]
                         + _VARIANTS[variant])
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = dm.HybridParallelDLRM(sizes, args, None, dev)
    embed = model.sparse_modules.embed
    embed.flush()
    embed.weight.copy_(torch.from_numpy(gold["table"]))
    model.dense_modules.load_state_dict({k[len("dense."):]: torch.from_numpy(gold[k]) for k in gold.files
                                         if k.startswith("dense.")})
    embed.set_fused_rowwise_adagrad(lr)                      # what main() does for --adagrad
    opt = torch.optim.Adagrad([{"params": list(model.dense_modules.parameters()), "lr": lr}])
    offsets = torch.arange(len(sizes) * B + 1, dtype=torch.int32)
    loader = [dict(dense=torch.from_numpy(gold["dense_x"][i]), labels=torch.from_numpy(gold["labels"][i]),
                   sparse=[torch.from_numpy(gold["values"][i]), offsets, B]) for i in range(steps)]
    rec = []
    done, _, _ = dm.train(model, opt, loader, args, dev, 0, 1, record=rec)
    assert done == steps
    torch.cuda.synchronize()
    embed.flush()
    mgr = embed.cache_weight_mgr
    assert np.array_equal(mgr.idx_map.cpu().numpy(), np.arange(mgr.num_embeddings))     # no frequency map
    np.savez(out, losses=torch.stack(rec).double().cpu().numpy(), table=mgr.weight.numpy(),
             momentum=mgr.momentum1.cpu().numpy())


@pytest.mark.parametrize("variant", list(_VARIANTS))
def test_example_adagrad_matches_torch_cpu(variant, tmp_path):
    import copy
    gold = np.load(ROOT / "tests" / "golden" / "dlrm_toy.npz")
    out = tmp_path / "child.npz"
    code = (f"import sys; sys.path.insert(0, {str(HERE)!r}); import test_gpu_rowwise_adagrad as t; "
            f"t._child({variant!r}, {str(out)!r})")
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = np.load(out)
    # the torch-CPU model: one full fp32 table with the reference update, the dense part under torch.optim.Adagrad
    sys.path.insert(0, str(ROOT / "examples"))
    import importlib
    dm = importlib.import_module("dlrm_main")
    sizes = [int(x) for x in gold["sizes"]]
    steps, B = gold["dense_x"].shape[0], gold["dense_x"].shape[1]
    D, lr, F = gold["table"].shape[1], float(gold["lr"]), len(sizes)
    dense = dm.DenseModules(gold["dense_x"].shape[2], F, D, [int(x) for x in gold["dense_arch"]],
                            [int(x) for x in gold["over_arch"]])
    dense.load_state_dict({k[len("dense."):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("dense.")})
    dense = copy.deepcopy(dense).float()
    opt = torch.optim.Adagrad(dense.parameters(), lr=lr)
    table = gold["table"].astype(np.float32).copy()
    mom = np.zeros(table.shape[0], np.float32)
    crit = torch.nn.BCEWithLogitsLoss()
    losses = []
    for i in range(steps):
        values = gold["values"][i].astype(np.int64)
        pooled = torch.from_numpy(table[values]).view(F, B, D).transpose(0, 1).contiguous().requires_grad_(True)
        loss = crit(dense(torch.from_numpy(gold["dense_x"][i]), pooled).squeeze(-1), torch.from_numpy(gold["labels"][i]))
        opt.zero_grad()
        loss.backward()
        opt.step()
        go = pooled.grad.numpy()                               # [B, F, D]
        rows, grads = ref.lookup_grads(values, np.arange(F * B + 1), go, table.shape[0], hook_features=F,
                                       dtype=np.float32)
        ref.step(table, mom, rows, grads, lr, dtype=np.float32)
        losses.append(float(loss))
    np.testing.assert_allclose(got["losses"], losses, rtol=0, atol=1e-4)
    np.testing.assert_allclose(got["table"], table, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got["momentum"], mom, rtol=1e-4, atol=1e-9)
