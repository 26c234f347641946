"""References, input builders and bars of the reconstruction-loss tests (a helper module, not a test).

Definition (include/vaehip.h, vaehip/losses.py): with r = reconstruction, x = target, d = r - x over n elements,
    pixel = mean d^2 (mse) | mean |d| (l1) | mean(|d| <= delta ? d^2 / 2 : delta (|d| - delta / 2)) (huber)
    ssim  = mean over images, channels and window positions of the SSIM index of u(r) against u(x), u(v) = (v + 1) / 2 NOT
            clamped, 11 x 11 gaussian (sigma 1.5), c1 = 0.01^2, c2 = 0.03^2, positions whose window lies inside the image
    rec   = pixel + ssim_weight * (1 - ssim),   seed = grad_scale * d rec / d r
The authority is the float64 torch evaluation below: loss terms directly, gradients by autograd on float64 leaves built from
the fp32 inputs.  `ssim_grad_closed_form` is the formula the kernels implement, with switches for the single mistakes the
host test shows the bars to reject.

Bars (none of them comes from what the kernels give):
  * pixel part of the seed: BITWISE the fp32 CPU expression coef * g(d), coef = float32(grad_scale * k / n): one fp32
    subtraction and one fp32 multiplication on both sides, no contraction (the library is built with -ffp-contract=off).
  * loss scalar: 2^-23 relative to float64.  The partial sums are float64 (order effects ~ n * 2^-53), then one fp32 store
    (2^-24); the inputs of these tests have d exact in fp32.
  * SSIM index (float64 result): 1e-10 absolute: both sides are float64, only the summation order differs (the bar and the
    argument of tests/test_image_metrics_gpu.py).
  * combined seed, elementwise: |got - ref| <= 2^-22 (|pixel part| + |ssim part|) + 1e-10 max|ref|.  At most four fp32
    roundings of 2^-24 each (coefficient, product, the SSIM part's single rounding, the sum), each relative to a quantity no
    larger than |pixel part| + |ssim part|, plus float64 reordering.  It presumes everything before the last store is float64.
"""
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
K = 11
LOSS_REL = 2.0 ** -23
INDEX_ABS = 1e-10
SEED_REL, SEED_ABS_OF_MAX = 2.0 ** -22, 1e-10
KINDS = ("mse", "l1", "huber")


def window(dtype=torch.float64):
    ax = torch.arange(K, dtype=torch.float64) - (K - 1) / 2
    g = torch.exp(-(ax / 1.5) ** 2 / 2)
    return (g / g.sum()).to(dtype)


def to_unit(v):
    return (v + 1.0) / 2.0


# ---------------------------------------------------------------------------------------------------------- float64 reference
def _blur(v, w, same_pad=False):
    """separable window sums of a (B, C, H, W) tensor at the valid positions (same_pad: at every pixel, zero padded)"""
    B, C, H, W = v.shape
    pad = (K - 1) // 2 if same_pad else 0
    v = v.reshape(B * C, 1, H, W)
    v = F.conv2d(v, w.view(1, 1, 1, K), padding=(0, pad))
    v = F.conv2d(v, w.view(1, 1, K, 1), padding=(pad, 0))
    return v.reshape(B, C, v.shape[-2], v.shape[-1])


def ssim_map(p, t, same_pad=False):
    """the index at every window position from u(pred) = p and u(target) = t, in their dtype"""
    w = window(p.dtype)
    mp, mt = _blur(p, w, same_pad), _blur(t, w, same_pad)
    qp, qt, rr = _blur(p * p, w, same_pad), _blur(t * t, w, same_pad), _blur(p * t, w, same_pad)
    A1, A2 = 2 * mp * mt + C1, 2 * (rr - mp * mt) + C2
    B1, B2 = mp * mp + mt * mt + C1, (qp - mp * mp) + (qt - mt * mt) + C2
    return A1 * A2 / (B1 * B2)


def ssim_index(pred, target):
    """float64 [B]: per-image mean index of fp32 (B, C, H, W) tensors"""
    s = ssim_map(to_unit(pred.double()), to_unit(target.double()))
    return s.reshape(s.shape[0], -1).mean(1)


def pixel_term(d, kind, delta):
    if kind == "mse":
        return (d * d).mean()
    if kind == "l1":
        return d.abs().mean()
    return F.huber_loss(d, torch.zeros_like(d), delta=delta, reduction="mean")


def reference(recon, target, kind="mse", delta=1.0, ssim_weight=0.0, grad_scale=1.0):
    """float64 everything from fp32 (B, C, H, W) tensors (any shape when ssim_weight == 0): dict(pixel, ssim, rec, seed_pixel,
    seed_ssim, seed), the seeds by autograd on a float64 leaf"""
    r = recon.detach().double().requires_grad_(True)
    x = target.detach().double()
    pixel = pixel_term(r - x, kind, delta)
    (gp,) = torch.autograd.grad(pixel, r)
    pixel = pixel.detach()
    out = {"pixel": float(pixel), "ssim": float("nan"), "rec": float(pixel), "seed_pixel": grad_scale * gp,
           "seed_ssim": torch.zeros_like(gp)}
    if ssim_weight > 0:
        ssim = ssim_map(to_unit(r), to_unit(x)).mean()
        (gs,) = torch.autograd.grad(ssim, r)
        ssim = ssim.detach()
        out.update(ssim=float(ssim), rec=float(pixel) + ssim_weight * (1.0 - float(ssim)), seed_ssim=-grad_scale * ssim_weight * gs)
    out["seed"] = out["seed_pixel"] + out["seed_ssim"]
    return out


# ---------------------------------------------------------------------------------------------------------- the kernels' formulas
def _full(m, w):
    """the transposed gaussian of a valid-position map: (B, C, H - 10, W - 10) -> (B, C, H, W), zero outside the map"""
    B, C, Hp, Wp = m.shape
    m = m.reshape(B * C, 1, Hp, Wp)
    m = F.conv_transpose2d(m, w.view(1, 1, 1, K))
    m = F.conv_transpose2d(m, w.view(1, 1, K, 1))
    return m.reshape(B, C, Hp + K - 1, Wp + K - 1)


def ssim_grad_closed_form(recon, target, stats_dtype=torch.float64, clamp=False, half=0.5, same_pad=False):
    """d mean(S) / d recon, float64, by the closed form of csrc/recon_loss.hip.  The switches are single mistakes: window
    statistics in fp32, a clamped u, a missing 1/2, same-padded positions."""
    p, t = to_unit(recon.double()), to_unit(target.double())
    if clamp:
        p, t = p.clamp(0, 1), t.clamp(0, 1)
    w = window(stats_dtype)
    ps, ts = p.to(stats_dtype), t.to(stats_dtype)
    mp, mt, qp, qt, rr = (_blur(v, w, same_pad).double() for v in (ps, ts, ps * ps, ts * ts, ps * ts))
    A1, A2 = 2 * mp * mt + C1, 2 * (rr - mp * mt) + C2
    B1, B2 = mp * mp + mt * mt + C1, (qp - mp * mp) + (qt - mt * mt) + C2
    S = A1 * A2 / (B1 * B2)
    a = (2 * mt * A2 - 2 * mt * A1) / (B1 * B2) - S * (2 * mp / B1 - 2 * mp / B2)
    b = -S / B2
    c = 2 * A1 / (B1 * B2)
    w64 = window()
    if same_pad:
        crop = (K - 1) // 2
        Ga, Gb, Gc = (_full(m, w64)[..., crop:-crop, crop:-crop] for m in (a, b, c))
    else:
        Ga, Gb, Gc = (_full(m, w64) for m in (a, b, c))
    return half * (Ga + 2 * p * Gb + t * Gc) / S.numel()


def pixel_seed_fp32(recon, target, kind, delta, grad_scale, sign0=0.0, swap=False):
    """the fp32 CPU expression the pixel part is bitwise equal to: coef * g(d).  sign0 / swap: the mistakes sign(0) != 0 and
    Huber's branches exchanged."""
    d = recon - target
    assert d.dtype == torch.float32
    coef = torch.tensor(grad_scale * (2.0 if kind == "mse" else 1.0) / d.numel(), dtype=torch.float64).float()
    sgn = torch.where(d > 0, 1.0, torch.where(d < 0, -1.0, sign0)).float()
    if kind == "mse":
        g = d
    elif kind == "l1":
        g = sgn
    else:
        quad = d.double().abs() <= delta
        if swap:
            quad = ~quad
        g = torch.where(quad, d, torch.tensor(delta, dtype=torch.float64).float() * sgn)
    return coef * g


# ---------------------------------------------------------------------------------------------------------- bars
def loss_ok(got: float, ref: float) -> bool:
    return abs(got - ref) <= LOSS_REL * abs(ref)


def index_ok(got, ref) -> bool:
    return bool(((got.double().cpu() - ref).abs() <= INDEX_ABS).all())


def seed_excess(got, ref) -> float:
    """worst |got - ref| / bound over the elements (<= 1 passes); got: any float tensor shaped like ref['seed']"""
    bound = SEED_REL * (ref["seed_pixel"].abs() + ref["seed_ssim"].abs()) + SEED_ABS_OF_MAX * ref["seed"].abs().max()
    err = (got.detach().double().cpu() - ref["seed"]).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    ratio = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, float("inf")))  # 0 of a bound of 0 passes
    return float(torch.where(bound > 0, err / bound.clamp_min(1e-300), ratio).max())


def seed_ok(got, ref) -> bool:
    return seed_excess(got, ref) <= 1.0


# ---------------------------------------------------------------------------------------------------------- inputs
def pixel_inputs(n, seed=0, offset=0):
    """fp32 recon, target [n] whose difference is an exact multiple of 2^-4 in [-1.5, 1.5]; elements 0, 1, 2 (mod 4) have
    d = 0, +0.5, -0.5 exactly (r == x; |d| == delta for the tests' delta = 0.5), the rest are random"""
    g = torch.Generator().manual_seed(4000 + 13 * n + seed)
    x = torch.randint(-16, 17, (n,), generator=g).float() / 16
    d = torch.randint(-24, 25, (n,), generator=g).float() / 16
    i = torch.arange(n)
    d[i % 4 == 0] = 0.0
    d[i % 4 == 1] = 0.5
    d[i % 4 == 2] = -0.5
    r = x + d
    assert torch.equal(r - x, d)
    return r, x


def ssim_inputs(shape, variant):
    """target uniform in [-1, 1]; prediction `noisy` (target + 0.2 randn), `flat` (target with 1e-3 added on every third
    column: nearly identical, where the three terms of the gradient cancel) or `range` (the noisy one scaled to reach +-2)"""
    g = torch.Generator().manual_seed(2000 + sum(s * 7 ** i for i, s in enumerate(shape)))
    t = torch.rand(shape, generator=g) * 2 - 1
    if variant == "flat":
        p = t.clone()
        p[..., ::3] += 1e-3
        return p, t
    p = t + 0.2 * torch.randn(shape, generator=g)
    if variant == "range":
        p = p * (2.0 / float(p.abs().max()))
    else:
        assert variant == "noisy", variant
    return p, t
