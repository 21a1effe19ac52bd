"""Inputs shared by the Adam tests (tests/test_adam_cpu.py, tests/test_gpu_adam.py) and torch's own answer to them:
torch.optim.SparseAdam over nn.EmbeddingBag(sparse=True) on the CPU.  Test infrastructure only."""
import numpy as np
import torch

N, D, STEPS = 64, 8, 12
LR, BETAS, EPS = 0.05, (0.9, 0.999), 1e-8
NEVER = N - 1                     # the row no step looks up


def zipf_steps(seed=11, steps=STEPS, nnz=48, max_unique=None):
    """[(ids [nnz], offsets [nb + 1], grad_out [nb, D] fp32, psw [nnz] fp32)]: Zipf ids with heavy duplicates over rows
    0 .. N - 2, ragged bags (some of them empty), per-sample weights with zeros among them.
    max_unique = u: every step names at most u distinct rows, from a window of rows that moves on by u - 2 per step and
    wraps around after 40 rows; every step names ALL u rows of its window -- a cache of u + 2 rows evicts at every step
    after the first and sees evicted rows again."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(steps):
        rank = np.minimum(rng.zipf(1.3, nnz) - 1, (max_unique or N - 1) - 1)
        if max_unique:
            rank[rng.permutation(nnz)[:max_unique]] = np.arange(max_unique)      # every row of the window is named
            ids = (k * (max_unique - 2) + rank) % 40
        else:
            ids = rng.permutation(N - 1)[rank]
        cuts = np.sort(rng.integers(0, nnz + 1, 15))
        off = np.concatenate([[0], cuts, [nnz]]).astype(np.int64)
        go = rng.standard_normal((len(off) - 1, D)).astype(np.float32)
        psw = rng.uniform(0.5, 1.5, nnz).astype(np.float32)
        psw[rng.random(nnz) < 0.15] = 0.0
        out.append((ids.astype(np.int64), off, go, psw))
    return out


def initial_weight(seed=5):
    return np.random.default_rng(seed).standard_normal((N, D)).astype(np.float32)


def sparse_adam_run(W0, steps, dtype=torch.float64, lr=LR, betas=BETAS, eps=EPS, use_psw=True):
    """(w, m, v) [N, D] numpy of torch.optim.SparseAdam after `steps`; loss = <out, grad_out>, so grad_out IS the
    gradient of the pooled output"""
    bag = torch.nn.EmbeddingBag(W0.shape[0], W0.shape[1], mode="sum", sparse=True, include_last_offset=True,
                                _weight=torch.tensor(W0, dtype=dtype))
    opt = torch.optim.SparseAdam(bag.parameters(), lr=lr, betas=betas, eps=eps)
    for ids, off, go, psw in steps:
        opt.zero_grad()
        out = bag(torch.from_numpy(ids), torch.from_numpy(off),
                  per_sample_weights=torch.tensor(psw, dtype=dtype) if use_psw else None)
        (out * torch.tensor(go, dtype=dtype)).sum().backward()
        opt.step()
    st = opt.state[bag.weight]
    z = np.zeros_like(W0, dtype=np.float64)
    return (bag.weight.detach().numpy().astype(np.float64),
            st["exp_avg"].numpy().astype(np.float64) if st else z, st["exp_avg_sq"].numpy().astype(np.float64) if st else z)
