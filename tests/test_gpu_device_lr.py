"""The learning rate from device memory on the GPU: a fused update whose `lr` is a one-element fp32
tensor goes to the ce_*_lrdev entries, whose kernels read the value when they run.  Held here: the new route computes the
old arithmetic (the recorded bits of tests/golden/fused_update_bits.npz); a schedule written into the tensor between
steps -- or between replays of a captured step -- gives, bit for bit, what the by-value twin gives for the same floats;
modules, GraphedWindow and the example trainer follow a schedule; what is refused is refused before any kernel runs.

Shapes are those the suite already runs (40 rows, 48 lookups, a row at most twice per step so the atomics cannot
reorder a sum; the GraphedWindow shape of test_prefetch_window_modes_train_identically_to_plain_embedding_bag)."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))

import fused_update_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = fc.cases()
R, F = fc.R, fc.F
LRS = [0.05, 0.0125, 0.2, 0.05]
DT = fc.DT


# ---- 1. golden replay ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    with np.load(HERE / "golden" / "fused_update_bits.npz") as z:
        g = {k: z[k] for k in z.files}
    assert [str(n) for n in g["names"]] == [c.name for c in CASES], "the fixture was recorded for another case list"
    return g


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.name for c in CASES])
def test_device_lr_gives_the_recorded_bits(golden, index, monkeypatch):
    """every case of tests/fused_update_cases.py, both accumulators, with the learning rate as a device tensor holding
    LR: the bits of the by-value library the fixture was recorded from"""
    made = []
    by_value = fc._fused

    def from_device(case, path):
        f = by_value(case, path)
        f.lr = torch.full((1,), fc.LR, dtype=torch.float32, device="cuda")
        made.append(f)
        return f

    monkeypatch.setattr(fc, "_fused", from_device)
    case = CASES[index]
    for path in case.paths:
        crc, mom = fc.run(case, index, path)
        if mom is not None:
            bad = fc.differing_rows(mom, golden["momentum"][index])
            assert not bad, (case.name, path, "momentum (step, row)", bad[:8])
        bad = fc.differing_rows(crc, golden["crc"][index])
        assert not bad, (case.name, path, "weight (step, row)", bad[:8])
    assert len(made) == 2 and all(isinstance(f.lr, torch.Tensor) for f in made)


# ---- 2. / 3. a schedule, eager and replayed --------------------------------------------------------------------------

def _mk_fused(kind, acc, lr):
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD
    parts = kind.split("-")
    if parts[1] == "adagrad":
        f = FusedRowwiseAdagrad(lr, momentum=torch.zeros(R, device="cuda"), accumulator=acc)
    else:
        f = FusedSGD(lr, accumulator=acc)
    f.rounding, f.seed = ("stochastic" if parts[-1] == "stoch" else "nearest"), fc.SEED
    return f


def _bits(t):
    if t is None:
        return None
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().clone()


def _batch(rng, form, D, into_rows=False):
    """(idx, offsets, grad_out, presorted) of one step: 48 lookups, 12 rows twice, 16 once, eight -1.
    into_rows (fp32 SGD): that update adds every partial sum straight into the live row, not into a zeroed accumulator,
    so a row looked up twice is a sum of THREE terms (w, a, b) whenever its two lookups are not folded by one lane group,
    and the order of the two atomics -- which no launch fixes -- shows in the last bit: (w + a) + b != (w + b) + a.  The
    two lookups of a row then carry the same gradient row (a == b): either order gives the same bits, and whether they
    are folded depends on the key positions alone, which the twin shares."""
    from cachedembedding_amd.functional import presort_slots, presort_window
    ids = fc._ids(rng, form)
    nnz = len(ids)
    go = rng.standard_normal((nnz // F, F, D)).astype(np.float32)
    if into_rows:
        flat, first = go.reshape(-1, D), {}
        for j, r in enumerate(ids):
            f, b = divmod(j, nnz // F)                         # lookup j = bag j reads row b * F + f of grad_out
            if r >= 0 and first.setdefault(int(r), b * F + f) != b * F + f:
                flat[b * F + f] = flat[first[int(r)]]
    go = torch.from_numpy(go).cuda()
    idx = torch.from_numpy(ids).cuda()
    offs = torch.arange(nnz + 1, device="cuda")
    pre = None
    if form == "presorted":
        pre = presort_slots(idx, R)
    elif form in ("src", "src_excl"):
        pre = presort_window(idx.view(1, -1), R, offsets=offs.to(torch.int32), include_last_offset=True,
                             hook_features=F, identity_bags=True,
                             ids=idx.view(1, -1).contiguous() if form == "src_excl" else None)[0]
        assert (pre.ranges is not None) == (form == "src_excl")
    return idx, offs, go, pre


def _step(w, fused, idx, offs, go, pre, out_dtype=torch.float32):
    from cachedembedding_amd.functional import embedding_bag
    w.requires_grad_(True)
    o = embedding_bag(idx, w, offs, mode="sum", include_last_offset=True, hook_features=F, fused_sgd=fused,
                      presorted=pre, masked_indices=True, output_dtype=out_dtype)
    o.backward(go.view_as(o).to(out_dtype))
    assert w.grad is None                                     # the update happened inside backward
    w.requires_grad_(False)


def _schedule(kind, acc, form, D, from_device, out_dtype=torch.float32):
    """[(weight bits, momentum bits)] after each of the four steps"""
    rng = np.random.default_rng(4242)
    w = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(DT[kind.split("-")[0]]).cuda()
    lr_src = torch.tensor(LRS, dtype=torch.float32, device="cuda")
    lr_t = torch.zeros(1, dtype=torch.float32, device="cuda")
    fused = _mk_fused(kind, acc, lr_t if from_device else LRS[0])
    out = []
    for k in range(len(LRS)):
        idx, offs, go, pre = _batch(rng, form, D, into_rows=kind == "fp32-sgd")
        if from_device:
            lr_t.copy_(lr_src[k:k + 1])                       # stream-ordered, nothing waits for it
        else:
            fused.lr = LRS[k]
        _step(w, fused, idx, offs, go, pre, out_dtype)
        out.append((_bits(w), _bits(getattr(fused, "momentum", None))))
    if from_device:
        assert fused.lr is lr_t
    return out


def _routes():
    out = []
    for form in ("slots", "presorted", "src", "src_excl"):                 # fp32 SGD: k_bag_bwd_tile / k_bag_bwd_stream
        for D in (8, 128, 6):
            out.append(("fp32-sgd", "cache", form, D, torch.float32))
    out += [("fp32-sgd", "cache", "slots", 512, torch.float32), ("fp32-sgd", "cache", "src", 512, torch.float32)]
    out.append(("fp32-sgd", "cache", "src", 128, torch.bfloat16))           # the pair form of k_bag_bwd_stream
    for acc in ("cache", "step"):                                          # k_rows_apply / k_compact_apply
        for form in ("slots", "src"):
            for D in (8, 128, 6):
                out.append(("fp32-adagrad", acc, form, D, torch.float32))
        out.append(("fp32-adagrad", acc, "slots", 512, torch.float32))
        for kind in ("bf16-sgd", "fp16-sgd", "bf16-sgd-stoch", "fp16-sgd-stoch", "bf16-adagrad"):
            for D in (8, 128):
                out.append((kind, acc, "slots", D, torch.float32))
        out.append(("bf16-sgd-stoch", acc, "src", 128, torch.float32))
    return out


ROUTES = _routes()


@pytest.mark.parametrize("kind, acc, form, D, out_dtype", ROUTES,
                         ids=["/".join(map(str, r[:4])) + ("/bf16-out" if r[4] != torch.float32 else "") for r in ROUTES])
def test_schedule_written_into_the_tensor_equals_the_by_value_twin(kind, acc, form, D, out_dtype):
    """four steps with lr = 0.05, 0.0125, 0.2, 0.05: the tensor rewritten by a device copy before each step against a
    twin (a fresh object, same seed: same step counters) that takes the same floats by value -- weights, momentum and the
    stochastic rounding, bit for bit, after every step"""
    got = _schedule(kind, acc, form, D, True, out_dtype)
    want = _schedule(kind, acc, form, D, False, out_dtype)
    for k, ((gw, gm), (ww, wm)) in enumerate(zip(got, want)):
        assert torch.equal(gw, ww), (k, "weight rows", torch.nonzero((gw != ww).any(1)).flatten()[:8].tolist())
        if wm is not None:
            assert torch.equal(gm, wm), (k, "momentum")
    assert not torch.equal(got[0][0], got[1][0])              # the steps did move the table


@pytest.mark.parametrize("kind, acc, form", [("fp32-sgd", "cache", "src"), ("fp32-adagrad", "cache", "slots"),
                                             ("bf16-sgd", "step", "slots")])
def test_schedule_under_a_replayed_graph_equals_eager_by_value(kind, acc, form):
    """one captured forward + backward replayed four times, the tensor filled before each replay == four eager by-value
    steps, bit for bit.  (A host read of the tensor anywhere on the route would make the capture raise.)"""
    D = 128
    rng = np.random.default_rng(99)
    W0 = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(DT[kind.split("-")[0]])
    idx, offs, go, pre = _batch(rng, form, D, into_rows=kind == "fp32-sgd")

    we, fe = W0.clone().cuda(), _mk_fused(kind, acc, LRS[0])
    eager = []
    for k in range(4):
        fe.lr = LRS[k]
        _step(we, fe, idx, offs, go, pre)
        eager.append((_bits(we), _bits(getattr(fe, "momentum", None))))

    lr_t = torch.full((1,), LRS[0], dtype=torch.float32, device="cuda")
    wg, fg = W0.clone().cuda(), _mk_fused(kind, acc, lr_t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(wg, fg, idx, offs, go, pre)                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():                                      # back to the start: table, state, step counter
        wg.copy_(W0)
        if hasattr(fg, "momentum"):
            fg.momentum.zero_()
        if fg._ws_step is not None:
            fg._ws_step[:8].zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _step(wg, fg, idx, offs, go, pre)
    deltas = []
    for k in range(4):
        before = wg.detach().float().cpu()
        lr_t.fill_(LRS[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(wg), eager[k][0]), k
        if eager[k][1] is not None:
            assert torch.equal(_bits(fg.momentum), eager[k][1]), k
        deltas.append(wg.detach().float().cpu() - before)
    # the same gradient every replay: only the value in the tensor tells replay 0 from replay 2
    assert not torch.equal(deltas[0], deltas[2])
    assert float(deltas[2].abs().max()) > float(deltas[1].abs().max())


# ---- 4. modules ------------------------------------------------------------------------------------------------------

MODULE_LRS = [0.5, 0.25, 0.1, 0.05, 0.2, 0.4]


def _module_batches(N, D):
    g = torch.Generator().manual_seed(11)
    out = []
    for _ in MODULE_LRS:
        perm = torch.randperm(N, generator=g)
        order = torch.randperm(24, generator=g)
        ids = torch.cat([perm[:8], perm[:8], perm[8:16]])[order]                                # a row at most twice
        # (the two lookups of a row carry the same gradient row: fp32 SGD adds straight into the row, see _batch)
        go = torch.randn(16, D, generator=g) * 0.1
        out.append((ids, torch.cat([go[:8], go[:8], go[8:]])[order]))
    return out


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("table", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_module_follows_a_schedule_in_the_tensor(opt, table):
    """two CachedEmbeddingBags over a cache of 32 rows (every step evicts), six steps, the rate changing every step: one
    reads a tensor, the other is set by value before each step; the host tables (and momentum1) end bit-equal"""
    import cachedembedding_amd as ce
    N, D = 200, 16
    g = torch.Generator().manual_seed(3)
    w0 = torch.randn(N, D, generator=g)
    batches = _module_batches(N, D)
    offs = torch.arange(25, dtype=torch.int32, device="cuda")
    lr_t = torch.zeros(1, dtype=torch.float32, device="cuda")
    mods = []
    for from_device in (True, False):
        emb = ce.CachedEmbeddingBag(N, D, _weight=w0.clone(), mode="sum", include_last_offset=True, cuda_row_num=32,
                                    table_dtype=table)
        if table != torch.float32 and opt == "adagrad":
            emb.set_weight_rounding("nearest")
        setter = emb.set_fused_sgd if opt == "sgd" else emb.set_fused_rowwise_adagrad
        if from_device:
            setter(lr_t)
        for k, (ids, go) in enumerate(batches):
            if from_device:
                lr_t.fill_(MODULE_LRS[k])
            else:
                setter(MODULE_LRS[k])
            out = emb(ids.cuda(), offs)
            out.backward(go.cuda().to(out.dtype))
        if from_device:
            assert emb._fused().lr is lr_t
        assert sum(emb.num_write_back_history) > 0, "the cache never evicted"
        emb.flush()
        mods.append(emb)
    a, b = mods
    assert torch.equal(_bits(a.weight), _bits(b.weight))
    if opt == "adagrad":
        assert torch.equal(_bits(a.cache_weight_mgr.momentum1), _bits(b.cache_weight_mgr.momentum1))
        assert float(a.cache_weight_mgr.momentum1.abs().sum()) > 0
    assert not torch.equal(a.weight.float(), w0.to(table).float())
    if opt == "sgd" and table == torch.float32:
        # ... and to nn.EmbeddingBag + torch.optim.SGD on the CPU, param_groups changed per step, at the tolerance
        # test_prefetch_window_modes_train_identically_to_plain_embedding_bag holds the by-value path to
        ref = torch.nn.EmbeddingBag.from_pretrained(w0.clone(), freeze=False, mode="sum", include_last_offset=True)
        sgd = torch.optim.SGD(ref.parameters(), lr=MODULE_LRS[0])
        for k, (ids, go) in enumerate(batches):
            for grp in sgd.param_groups:
                grp["lr"] = MODULE_LRS[k]
            sgd.zero_grad()
            ref(ids, offs.cpu().long()).backward(go)
            sgd.step()
        torch.testing.assert_close(a.weight, ref.weight.detach(), rtol=1e-4, atol=1e-4)


# ---- 5. GraphedWindow ------------------------------------------------------------------------------------------------

def test_graphed_window_reads_the_rate_at_every_replay():
    """the `graph` mode with source-row keys of test_prefetch_window_modes_train_identically_to_plain_embedding_bag, at
    its shape, with set_fused_sgd(tensor) and the tensor refilled before every run"""
    import cachedembedding_amd as ce
    from cachedembedding_amd.pipeline import GraphedWindow
    torch.manual_seed(0)
    N, D, F_, B, P, nwin = 20000, 64, 4, 64, 4, 6
    warm_lr, lrs = 0.5, [0.5, 0.25, 0.5, 0.125, 0.0625, 0.25]
    w0 = torch.randn(N, D)
    emb = ce.CachedEmbeddingBag(N, D, sparse=True, _weight=w0.clone(), mode="sum", include_last_offset=True,
                                cuda_row_num=4 * F_ * B * P, warmup_ratio=0.5, strict=False)
    lr_t = torch.full((1,), warm_lr, dtype=torch.float32, device="cuda")
    emb.set_fused_sgd(lr_t)
    emb.set_cache_op(False)
    off = torch.arange(F_ * B + 1, dtype=torch.int32, device="cuda")
    grad = (torch.randn(B, F_, D) * 0.1).cuda()
    g = torch.Generator().manual_seed(5)
    windows = [[(torch.rand(F_ * B, generator=g) ** 3 * N).long().clamp_(0, N - 1) for _ in range(P)]
               for _ in range(nwin)]
    ref = w0.clone()
    rows = grad.cpu().transpose(0, 1).reshape(-1, D)

    def step(slots, i, keys=None):
        out = emb(slots, off, hook_features=F_, presorted=keys)
        out.backward(grad)

    gw = GraphedWindow(emb, P, F_ * B, step, overlap=True, warmup_values=[v.cuda() for v in windows[0]], presort=True,
                       transport="worker", bag_layout=(off, True, F_), arrangement="overlap")
    for v in windows[0]:                         # the capture warm-up's eager pass, with the value the tensor held then
        ref.index_add_(0, v, rows, alpha=-warm_lr)
    gw.submit([v.cuda() for v in windows[0]], 0)
    for w in range(nwin):
        if w + 1 < nwin:
            gw.submit([v.cuda() for v in windows[w + 1]], (w + 1) % 2)
        lr_t.fill_(lrs[w])
        gw.run(w % 2)
        for v in windows[w]:
            ref.index_add_(0, v, rows, alpha=-lrs[w])
    torch.cuda.synchronize()
    assert emb.cache_weight_mgr.sync_stats().status == 0 and emb.fused_sgd.lr is lr_t
    emb.flush()
    torch.testing.assert_close(emb.weight, ref, rtol=1e-4, atol=1e-4)


# ---- 6. refusals, each before any kernel has run ----------------------------------------------------------------------

def test_refusals_come_before_any_kernel():
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, FusedSGD, embedding_bag
    rng = np.random.default_rng(5)
    D = 8
    w = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).cuda().requires_grad_(True)
    start = w.detach().clone()
    idx, offs, go, _ = _batch(rng, "slots", D)
    on_gpu = torch.full((1,), 0.1, device="cuda")
    elsewhere = [torch.full((1,), 0.1)]
    if torch.cuda.device_count() > 1:
        elsewhere.append(torch.full((1,), 0.1, device="cuda:1"))

    def call(fused, mode="sum"):
        return embedding_bag(idx, w, offs, mode=mode, include_last_offset=True, fused_sgd=fused, masked_indices=True)

    for t in elsewhere:
        direct = FusedSGD(0.1)
        direct.lr = t                                               # assigned directly: checked in embedding_bag too
        for fused in (FusedSGD(t), FusedRowwiseAdagrad(t, momentum=torch.zeros(R, device="cuda")), direct):
            with pytest.raises(ValueError, match="learning-rate tensor"):
                call(fused)
    with pytest.raises(NotImplementedError, match="max"):
        call(FusedSGD(on_gpu), mode="max")
    for fused in (FusedSGD(on_gpu), FusedRowwiseAdagrad(on_gpu, momentum=torch.zeros(R, device="cuda"))):
        fused.deterministic = True                                  # (refused at construction; set afterwards here)
        with pytest.raises(NotImplementedError, match="deterministic"):
            call(fused)
    torch.cuda.synchronize()
    assert torch.equal(w.detach(), start) and w.grad is None
    # the same objects' by-value forms still run
    o = call(FusedSGD(0.1))
    o.backward(torch.ones_like(o))
    assert not torch.equal(w.detach(), start)


# ---- 7. the example trainer ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def toy():
    """the toy DLRM of tests/golden/make_dlrm_golden.py (its start and its batches: tests/golden/dlrm_toy.npz) trained
    by torch on the CPU with --change_lr at 0.5 to a quarter of the rate: (gold, losses, final table)"""
    sys.path.insert(0, str(HERE / "golden"))
    sys.path.insert(0, str(ROOT / "examples"))
    mk = importlib.import_module("make_dlrm_golden")
    dm = importlib.import_module("dlrm_main")
    gold = np.load(HERE / "golden" / "dlrm_toy.npz")
    assert [int(x) for x in gold["sizes"]] == mk.SIZES and gold["dense_x"].shape[:2] == (mk.STEPS, mk.B)
    Fn, lr = len(mk.SIZES), float(gold["lr"])
    dense = dm.DenseModules(mk.NUM_DENSE, Fn, mk.D, mk.DENSE_ARCH, mk.OVER_ARCH)
    dense.load_state_dict({k[len("dense."):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("dense.")})
    emb = torch.nn.EmbeddingBag.from_pretrained(torch.from_numpy(gold["table"]).clone(), freeze=False, mode="sum",
                                                include_last_offset=True, sparse=True)
    opt = torch.optim.SGD([{"params": emb.parameters(), "lr": lr}, {"params": dense.parameters(), "lr": lr}])
    crit = torch.nn.BCEWithLogitsLoss()
    offsets = torch.arange(Fn * mk.B + 1, dtype=torch.int64)
    losses, changed = [], False
    for it in range(mk.STEPS):
        e = emb(torch.from_numpy(gold["values"][it]), offsets).view(Fn, mk.B, mk.D).transpose(0, 1)
        loss = crit(dense(torch.from_numpy(gold["dense_x"][it]), e).squeeze(-1), torch.from_numpy(gold["labels"][it]))
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
        if not changed and (it * 1 / mk.STEPS) > 0.5:            # baselines/dlrm_main.py:453-462
            for grp in opt.param_groups:
                grp["lr"] = lr / 4
            changed = True
    assert changed and not np.allclose(losses, gold["losses"], atol=1e-4)    # the change is visible in the trajectory
    return gold, np.array(losses), emb.weight.detach().numpy()


@pytest.mark.parametrize("extra", [["--fused_sgd", "--fold_hook"], ["--overlap_cache_op", "--fused_sgd", "--fold_hook"],
                                   ["--overlap_cache_op", "--fused_sgd", "--fold_hook", "--graph_step", "--graph_after",
                                    "3"]], ids=["eager", "overlap", "graph_step"])
def test_trainer_changes_the_rate_like_torch_on_the_cpu(toy, extra):
    """20 steps of examples/dlrm_main.py's loop with --change_lr: losses within 1e-4 and the final table within 1e-5 of
    the CPU run (the bounds of test_toy_dlrm_matches_torch_cpu_trajectory); the graphed run captures once"""
    dm = importlib.import_module("dlrm_main")
    gold, want_losses, want_table = toy
    sizes = [int(x) for x in gold["sizes"]]
    steps, B = gold["dense_x"].shape[0], gold["dense_x"].shape[1]
    D, lr = gold["table"].shape[1], float(gold["lr"])
    args = dm.parse_args(["--use_cache", "--cache_ratio", "0.4", "--prefetch_num", "4", "--use_sparse_embed_grad",
                          "--embedding_dim", str(D), "--batch_size", str(B), "--learning_rate", str(lr),
                          "--dense_arch_layer_sizes", ",".join(str(int(x)) for x in gold["dense_arch"]),
                          "--over_arch_layer_sizes", ",".join(str(int(x)) for x in gold["over_arch"]),
                          "--change_lr", "--lr_change_point", "0.5", "--lr_after_change_point", str(lr / 4)] + extra)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = dm.HybridParallelDLRM(sizes, args, None, dev)
    embed = model.sparse_modules.embed
    embed.flush()                                            # empty cache, then the fixture's table
    embed.weight.copy_(torch.from_numpy(gold["table"]))
    model.dense_modules.load_state_dict({k[len("dense."):]: torch.from_numpy(gold[k]) for k in gold.files
                                         if k.startswith("dense.")})
    opt, lr_t = dm.make_optimizer(model, args, dev, 1)
    graphed = "--graph_step" in extra
    assert (lr_t is not None) == graphed and (embed.fused_sgd.lr is lr_t if graphed else embed.fused_sgd.lr == lr)
    offsets = torch.arange(len(sizes) * B + 1, dtype=torch.int32)
    loader = [dict(dense=torch.from_numpy(gold["dense_x"][i]), labels=torch.from_numpy(gold["labels"][i]),
                   sparse=[torch.from_numpy(gold["values"][i]), offsets, B]) for i in range(steps)]
    rec = []
    done, _, _ = dm.train(model, opt, loader, args, dev, 0, 1, record=rec,
                          lr_change=dm.LrChange(args, steps, opt, embed, lr_t))
    assert done == steps and dm.train.graph_captures == (1 if graphed else 0)
    losses = torch.stack(rec).double().cpu().numpy()
    np.testing.assert_allclose(losses, want_losses, rtol=0, atol=1e-4)
    embed.flush()
    np.testing.assert_allclose(embed.weight.numpy(), want_table, rtol=1e-5, atol=1e-5)
    if graphed:
        assert float(lr_t) == pytest.approx(lr / 4) and embed.fused_sgd.lr is lr_t
    else:
        assert embed.fused_sgd.lr == pytest.approx(lr / 4)
