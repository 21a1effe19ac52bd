"""CPU tests of the fused exact row-wise Adagrad: the reference against a hand-computed answer, the C ABI of the new
entry points, and the refusals that can be reached without a device."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

import rowwise_adagrad_ref as ref  # noqa: E402

ENTRY_POINTS = ["ce_bag_backward_rowwise_adagrad_workspace", "ce_bag_backward_rowwise_adagrad",
                "ce_bag_backward_rowwise_adagrad_src"]


def _three_steps(step_fn):
    """rows 0, 1, 2 of D = 4 (row 2 never looked up); one id per bag, lr = 0.1"""
    W = np.zeros((3, 4))
    W[2] = 5.0
    M = np.zeros(3)
    batches = [([0, 0, 1], [[1, 1, 1, 1], [1, 1, 1, 1], [2, 0, 0, 0]]),     # row 0 twice in one batch
               ([0], [[0, 0, 0, 4]]),
               ([1, 1], [[1, 0, 0, 0], [-1, 0, 0, 0]])]                        # row 1 twice, gradients cancel
    for ids, g in batches:
        rows, grads = ref.lookup_grads(ids, np.arange(len(ids) + 1), np.asarray(g, float), 3)
        step_fn(W, M, rows, grads, 0.1)
    return W, M


def test_reference_known_answer_one_update_per_unique_row():
    W, M = _three_steps(ref.step)
    # step 1: row 0 folds to g = 2 (all d): m = 16 / 4 = 4, W -= 0.1 * 2 / 2; row 1: g = (2,0,0,0), m = 1, W -= 0.2
    # step 2: row 0, g = (0,0,0,4): m = 4 + 4 = 8, W[3] -= 0.4 / sqrt(8)
    # step 3: row 1's two lookups fold to g = 0: no change at all
    np.testing.assert_allclose(W[0], [-0.1, -0.1, -0.1, -0.1 - 0.4 / np.sqrt(8)], rtol=1e-7)
    np.testing.assert_allclose(W[1], [-0.2, 0, 0, 0], rtol=1e-7)
    np.testing.assert_array_equal(W[2], [5, 5, 5, 5])
    np.testing.assert_allclose(M, [8, 1, 0], rtol=1e-7)
    Wl, Ml = _three_steps(ref.step_per_lookup)
    # per lookup: row 0 gets 0.1 / 1 + 0.1 / sqrt(2) in step 1 -- and row 1 moves in step 3
    assert abs(Wl[0, 0] - W[0, 0]) > 0.05 and not np.allclose(Wl[1], W[1]) and Ml[1] != M[1]


def test_reference_fp32_form_follows_fp64():
    rng = np.random.default_rng(3)
    R, D = 50, 16
    W64, M64 = rng.standard_normal((R, D)), np.zeros(R)
    W32, M32 = W64.astype(np.float32), M64.astype(np.float32)
    for _ in range(5):
        ids = rng.integers(0, R, 200)
        ids[:40] = 7                                              # one hot row
        off = np.arange(0, 201, 2)
        go = rng.standard_normal((100, D))
        r64, g64 = ref.lookup_grads(ids, off, go, R, mode="mean")
        r32, g32 = ref.lookup_grads(ids, off, go.astype(np.float32), R, mode="mean", dtype=np.float32)
        ref.step(W64, M64, r64, g64, 0.05)
        ref.step(W32, M32, r32, g32, 0.05, dtype=np.float32)
    np.testing.assert_allclose(W32, W64, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(M32, M64, rtol=1e-4)


def test_reference_hook_padding_and_row_map():
    go = np.arange(2 * 2 * 3, dtype=float).reshape(2, 2, 3)      # [B = 2, F = 2, D = 3]
    rows, g = ref.lookup_grads([4, 9, 4, -1], np.arange(5), go, 8, hook_features=2, padding_idx=None)
    # bag g = f * B + b: bags 0, 1 are feature 0 of samples 0, 1; 9 is out of range, -1 ignored
    assert rows.tolist() == [4, 4]
    np.testing.assert_array_equal(g, [go[0, 0], go[0, 1]])
    W, M = np.zeros((8, 3)), np.zeros(20)
    ref.step(W, M, rows, g, 1.0, row_of=np.arange(8) + 10)
    assert M[14] > 0 and M[:14].sum() == 0 and M[15:].sum() == 0


def test_header_declares_and_library_exports_the_adagrad_entry_points():
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    body = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ce_api.h").read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", body), name
        assert re.search(rf" T {name}\b", out), name
        assert name in _lib.SIGNATURES
    assert _lib.lib.ce_version() == 6
    # acc fp32 [rows, D] + one flag byte per row, each 256-byte aligned
    assert _lib.lib.ce_bag_backward_rowwise_adagrad_workspace(1000, 128) == 1000 * 128 * 4 + 1024
    assert _lib.lib.ce_bag_backward_rowwise_adagrad_workspace(-1, 128) == 0


def _dlrm():
    sys.path.insert(0, str(ROOT / "examples"))
    import importlib
    return importlib.import_module("dlrm_main")


def test_example_parses_adagrad_and_refuses_what_it_cannot_do(monkeypatch):
    dm = _dlrm()
    args = dm.parse_args(["--use_cache", "--adagrad", "--window_keys", "--fold_hook", "--graph_step", "--eval_acc"])
    assert args.adagrad and not args.fused_sgd
    assert not dm.parse_args(["--use_cache"]).adagrad
    with pytest.raises(ValueError, match="--adagrad takes the place of --fused_sgd"):
        dm.main(["--use_cache", "--adagrad", "--fused_sgd"])
    with pytest.raises(NotImplementedError, match="--adagrad"):
        dm.main(["--use_cache", "--adagrad", "--use_tablewise"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="--adagrad"):
        dm.main(["--use_cache", "--adagrad"])


def test_refusals_before_any_kernel():
    import torch
    from cachedembedding_amd.functional import FusedRowwiseAdagrad, embedding_bag
    from cachedembedding_amd.parallel import RowwiseShardedEmbeddingBag
    with pytest.raises(NotImplementedError, match="row-wise sharded"):
        RowwiseShardedEmbeddingBag.set_fused_rowwise_adagrad(None, 0.1)
    RowwiseShardedEmbeddingBag.set_fused_rowwise_adagrad(None, None)          # off: nothing to refuse
    w = torch.zeros(4, 2)
    with pytest.raises(NotImplementedError, match="mode='max'"):
        embedding_bag(torch.zeros(2, dtype=torch.long), w, torch.arange(2), mode="max",
                      fused_sgd=FusedRowwiseAdagrad(0.1, momentum=torch.zeros(4)))
    with pytest.raises(ValueError, match="momentum"):                         # state on the host: refused
        embedding_bag(torch.zeros(2, dtype=torch.long), w, torch.arange(2), mode="sum",
                      fused_sgd=FusedRowwiseAdagrad(0.1, momentum=torch.zeros(4)))


def test_adagrad_entries_refuse_an_unsupported_dim_before_their_first_launch():
    """dim = 2048 (a multiple of 4 past the 1024 of the vector form) is refused by both entries, fp32 and _act, with the
    code and message of every other bag entry -- before the mark kernel has set a flag in the workspace.  The pointers
    are made-up addresses, which is why this runs only where nothing could be launched."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("passes made-up addresses: only for machines without a GPU")
    import __graft_entry__ as g
    g.build()
    from cachedembedding_amd import _lib
    lib = _lib.lib
    R, D, n = 1000, 2048, 64
    p = [0x7f0000000000 + 0x100000 * i for i in range(8)]            # non-null, 256-byte aligned
    ws_bytes = lib.ce_bag_backward_rowwise_adagrad_workspace(R, D)
    bag = (p[1], n, p[2], 0, n, 1, None, _lib.CE_MODE_SUM, 0)         # indices ... hook_features
    tail = (None, p[5], R, 0.1, 1e-8, p[6], ws_bytes, None)           # row_of_slot ... stream
    calls = [lambda: lib.ce_bag_backward_rowwise_adagrad(p[0], R, D, *bag, p[3], None, *tail),
             lambda: lib.ce_bag_backward_rowwise_adagrad_act(p[0], R, D, *bag, p[3], _lib.CE_ACT_BF16, None, *tail),
             lambda: lib.ce_bag_backward_rowwise_adagrad_src(p[0], R, D, n, p[3], p[4], *tail),
             lambda: lib.ce_bag_backward_rowwise_adagrad_src_act(p[0], R, D, n, p[3], _lib.CE_ACT_F32, p[4], *tail)]
    for call in calls:
        assert call() == _lib.CE_ERR_UNSUPPORTED
        assert "too large for this build" in _lib.last_error()
