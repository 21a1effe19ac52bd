"""Reference of the half-precision activations (bf16 / fp16 pooled output, bf16 / fp16 incoming gradient) in numpy and
torch-CPU: the specification the `ce_*_act` kernels are held to.  Test infrastructure only.

Forward.  The table and the sums are fp32; the output is rounded ONCE, to nearest even, on the store.
  * one id per bag, sum, no weights: the forward is a row copy, so out == W[slot].to(dtype) bit for bit (NaN stays
    NaN, whatever its payload) -- `assert_cast_equal`;
  * anything that sums: with ref64 the fp64 result, L the bag's length and E32 = L * 2^-24 * sum |terms| the fp32
    accumulation bound, |float(out) - ref64| <= u |ref64| + (1 + u) E32 (+ 2^-25 for fp16: half a subnormal step),
    u = 2^-8 (bf16) / 2^-11 (fp16) -- `forward_bound`.  Equality with the cast of ANOTHER fp32 summation order is not
    asserted: the order flips the rounding of some elements.
Backward.  The upcast of a 16-bit gradient is exact, so a kernel that reads g16 must give what the fp32 kernel gives
for g16.float(): no new tolerance."""
import numpy as np
import torch

UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U32 = 2.0 ** -24


def special_values() -> torch.Tensor:
    """fp32 values whose 16-bit cast has one right answer worth pinning: NaNs of both kinds and signs, infinities, a
    value above fp16's largest, fp16 subnormals and the ties around them, bf16 ties, signed zero."""
    bits = np.array([0x7fc00000, 0xffc00000,            # quiet NaN +-
                     0x7f800001, 0xff800001,            # signalling NaN +- (payload in the low bits only)
                     0x7f800000, 0xff800000], dtype=np.uint32)
    vals = np.array([70000.0, -70000.0, 65504.0, 65519.9, 65520.0,           # fp16: inf beyond 65504 + half a step
                     2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, -(2.0 ** -24), 2.0 ** -14 - 2.0 ** -25,
                     1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,
                     -0.0, 0.0, 1e-40, 3.0e38, -3.4e38], dtype=np.float32)
    return torch.from_numpy(np.concatenate([bits.view(np.float32), vals]))


def cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """the one correct rounding of fp32 values: torch's CPU cast (round to nearest even)"""
    assert x.dtype == torch.float32 and x.device.type == "cpu"
    return x.to(dtype)


def assert_cast_equal(got: torch.Tensor, want: torch.Tensor) -> None:
    """got == want as bits, except that any NaN matches any NaN"""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"NaN positions differ in {int((gn != wn).sum())} elements"
    gb, wb = got.view(torch.int16), want.view(torch.int16)
    bad = (gb != wb) & ~gn
    assert not bool(bad.any()), (f"{int(bad.sum())} elements differ as bits, first at "
                                 f"{bad.nonzero()[0].tolist()}: {got[bad][0].item()} vs {want[bad][0].item()}")


def bag_ref64(W, idx, offsets, psw=None, mode="sum", include_last_offset=True, hook_features=0):
    """(ref64 [nb, D], abs_sum [nb, D], L [nb]) of F.embedding_bag in fp64.  Lookups outside [0, rows) take no part in
    the sum; `mean` divides by the bag's length as the kernels do (tested without ignored lookups).  abs_sum = the sum
    of |terms| as they enter the fp32 sum (scaled by psw / 1 / L).  hook_features = F: the rows are returned in the
    order of the [B, F, D] output (row b * F + f for bag f * B + b)."""
    W = np.asarray(W, np.float64)
    idx = np.asarray(idx, np.int64).reshape(-1)
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    nb = len(offsets) - 1 if include_last_offset else len(offsets)
    ends = offsets[1:] if include_last_offset else np.append(offsets[1:], len(idx))
    D = W.shape[1]
    ref, asum, L = np.zeros((nb, D)), np.zeros((nb, D)), np.zeros(nb, np.int64)
    for b in range(nb):
        lo, hi = int(offsets[b]), int(ends[b])
        L[b] = hi - lo
        for j in range(lo, hi):
            r = idx[j]
            if r < 0 or r >= W.shape[0]:
                continue
            s = 1.0 if psw is None else float(psw[j])
            if mode == "mean" and hi - lo > 1:
                s = s / (hi - lo)
            ref[b] += W[r] * s
            asum[b] += np.abs(W[r] * s)
    if hook_features:
        F = hook_features
        B = nb // F
        perm = (np.arange(nb) % F) * B + np.arange(nb) // F         # output row b * F + f <- bag f * B + b
        ref, asum, L = ref[perm], asum[perm], L[perm]
    return ref, asum, L


def forward_bound(ref64, abs_sum, L, dtype: torch.dtype):
    """the per-element bound on |float(out) - ref64| stated at the top"""
    u = UNIT_ROUNDOFF[dtype]
    e32 = np.asarray(L, np.float64).reshape(-1, 1) * U32 * np.asarray(abs_sum, np.float64)
    b = u * np.abs(ref64) + (1 + u) * e32
    if dtype == torch.float16:
        b = b + 2.0 ** -25
    return b


def violations(out16: torch.Tensor, ref64, abs_sum, L) -> int:
    """elements of a 16-bit output outside forward_bound"""
    got = out16.detach().cpu().double().numpy().reshape(np.shape(ref64))
    return int((np.abs(got - ref64) > forward_bound(ref64, abs_sum, L, out16.dtype)).sum())
