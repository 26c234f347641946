"""Float64 references and error bounds for ops.changrad / tracking.monitor.compute_grad_metrics (a helper module, not a test).

Operands are NHWC (B, H, W, C), fp32 or bf16; the stored values widen exactly to float64, so every reference product is exact
and every reference sum carries float64 rounding only.

Bounds (nothing here is measured; they follow from the kernel's stated arithmetic, csrc/changrad.hip): a workgroup sums the
`per` pixels of its chunk in fp32 -- one rounding per product (the library is built without contraction) and fewer than `per`
fp32 additions on any chain however the pixel rows are dealt to lanes (an addition to an exact zero does not round) -- and
everything after the workgroup is float64.  With u = 2^-24 and S the sum of the absolute terms, a sum is therefore within
(per + 2) u S: per u S to first order and 2 u S for the higher orders and the float64 tail.  The saliency is a mean over images
of |P[b]|, and | |x| - |y| | <= |x - y|: its bound is the mean over images of the per-image bounds.  max |g| is bit-exact.
At the shapes of the tests one dropped or doubled element moves a sum by about S / N >= 1e-3 S, far outside (per + 2) u S."""
import numpy as np
import torch

U = 2.0 ** -24
ROWS = ("mean_abs_gradient_per_channel", "gain_gradient_per_channel", "taylor_saliency_per_channel")  # rows of `sums`
ABSMAX = "abs_max_gradient_per_channel"


def _f64(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu()
    return t.float().double().numpy().reshape(t.shape[0], -1, t.shape[-1])  # [B, HW, C]; bf16 -> fp32 -> float64 is exact


def ref(a: torch.Tensor, g: torch.Tensor):
    """-> dict(sums float64 [3, C], absmax fp32 [C] (NaN if the channel holds one), bound float64 [3, C] per unit of
    (per + 2) u: the absolute term sums behind each row, already divided like the row)"""
    a64, g64 = _f64(a), _f64(g)
    B, HW, Cc = g64.shape
    with np.errstate(invalid="ignore", over="ignore"):
        ag = a64 * g64
        P = ag.sum(axis=1)                                   # [B, C]
        Sb = np.abs(ag).sum(axis=1)                          # [B, C]: the absolute terms of each image
        sums = np.stack([np.abs(g64).sum(axis=(0, 1)) / (B * HW), P.sum(axis=0), np.abs(P).sum(axis=0) / B])
        scale = np.stack([np.abs(g64).sum(axis=(0, 1)) / (B * HW), Sb.sum(axis=0), Sb.sum(axis=0) / B])
    g32 = np.abs(g.detach().cpu().float().numpy().reshape(-1, Cc))
    absmax = g32.max(axis=0)                                 # np.max propagates a NaN
    return {"sums": sums, "absmax": absmax.astype(np.float32), "scale": scale}


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def check(sums, absmax, a: torch.Tensor, g: torch.Tensor, per: int, skip_channels=()):
    """the device results against ref(a, g) within (per + 2) u S; `per` = pixels of a chunk (ceil(HW / nchunk)).
    skip_channels: channels whose gradient holds an inf or a NaN: only their max |g| is held.  -> the worst error / bound"""
    r = ref(a, g)
    got = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    amax = absmax.detach().cpu().numpy() if isinstance(absmax, torch.Tensor) else np.asarray(absmax)
    assert got.dtype == np.float64 and got.shape == r["sums"].shape, (got.dtype, got.shape)
    assert amax.dtype == np.float32 and same_bits(amax, r["absmax"]), (amax, r["absmax"])
    keep = np.ones(got.shape[1], dtype=bool)
    keep[list(skip_channels)] = False
    bound = (per + 2) * U * r["scale"][:, keep]
    err = np.abs(got[:, keep] - r["sums"][:, keep])
    assert np.isfinite(got[:, keep]).all()
    assert (err <= bound).all(), (np.argwhere(err > bound)[:8], err.max(), bound.max())
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nan_to_num(err / bound, nan=0.0).max()) if err.size else 0.0


def draw(shape, seed: int):
    """(a, g) fp32 on the CPU: a = randn * 1.3 + 0.4, g = randn * 0.02 * 2^k (k in -3..3 per channel): a g has both signs
    and sum a g cancels to about sqrt(N) of the N absolute terms"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randn(shape, generator=gen) * 1.3 + 0.4
    g = torch.randn(shape, generator=gen) * 0.02 * torch.pow(2.0, torch.randint(-3, 4, (shape[-1],), generator=gen).float())
    return a, g
