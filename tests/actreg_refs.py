"""Float64 references and error bounds for ops.actreg_stats / ops.actreg_inject (csrc/actreg.hip) and the penalty definitions of
vaehip/actreg.py (a helper module, not a test).

Operands are NHWC (B, H, W, C), fp32 or bf16; the stored values widen exactly to float64.  The kernels compare and subtract the
threshold as an fp32 number, so the ceiling's reference terms use float64(fp32(t)); the floor's threshold enters only the
float64 final pass and is used as given.

Bounds (nothing here is measured; they follow from the kernel's association order).  u = 2^-24.
Statistics: a lane adds the pixels p0 + pr, p0 + pr + PR, ... of its chunk in order: a chain of at most L = ceil(per / PR)
fp32 additions, per = ceil(HW / nchunk) pixels of a chunk and PR = 256 // (channel units of the workgroup's tile) pixel rows;
the PR rows are then added in row order: PR more.  A term of sum |a| is exact; a term of the ceiling sum carries three
roundings (e = |a| - t once, e * e = e^2 (1 + d)^2 (1 + d') twice more).  With S the sum of the (non-negative) terms a sum is
within (L + PR + 2) u S, the ceiling sum within (L + PR + 5) u S: the chain to first order, the term roundings, and 2 u S for
the higher orders and the float64 final pass, which adds B * nchunk numbers.  The count is exact.  pen and coef are float64
functions of the sums: their bounds are those of the sums carried through (first order plus the square for the floor), plus one
fp32 rounding of coef.
Inject: out = fp32(g + fp32(k * psi)).  psi = sign(a) is exact; psi = a - clamp(a, -t, t) is rounded once.  So the product
carries one rounding for the floor and two for the ceiling, the sum one more, and a bf16 result is rounded once more (2^-8
relative: bf16 keeps 8 significant bits).  Where the product is zero the element of g is passed on exactly."""
import numpy as np
import torch

U = 2.0 ** -24
KINDS = ("ceiling", "floor")


def f64(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu()
    return t.float().double().numpy()  # bf16 -> fp32 -> float64 is exact


def t32(threshold: float) -> float:
    return float(np.float32(threshold))


def mask_of(C: int, channels):
    w = np.ones(C) if channels is None else np.zeros(C)
    if channels is not None:
        w[list(channels)] = 1.0
    return w


# ---------------------------------------------------------------------------------------------------- definitions (torch, float64)
def penalty(a: torch.Tensor, kind: str, threshold: float, weight: float, channels=None, channel_dim: int = -1) -> torch.Tensor:
    """the definition, differentiable: a float64 tensor with channels on `channel_dim` -> the scalar P"""
    a = a.movedim(channel_dim, -1)
    C = a.shape[-1]
    N = a.numel() // C
    w = torch.as_tensor(mask_of(C, channels), dtype=a.dtype, device=a.device)
    if kind == "ceiling":
        return weight * (w * torch.relu(a.abs() - threshold).pow(2).reshape(-1, C).sum(0)).sum() / (N * C)
    m = a.abs().reshape(-1, C).mean(0)
    return weight * (w * torch.relu(threshold - m).pow(2)).sum() / C


def grad_formula(a: np.ndarray, kind: str, threshold: float, weight: float, channels=None, grad_scale: float = 1.0):
    """the issue's closed forms on a float64 [..., C] array: (k [C], psi [..., C]) with grad_scale * dP/da = k * psi"""
    C = a.shape[-1]
    N = a.size // C
    w = mask_of(C, channels)
    if kind == "ceiling":
        k = 2.0 * weight * w * grad_scale / (N * C)
        psi = a - np.clip(a, -threshold, threshold)
    else:
        m = np.abs(a).reshape(-1, C).mean(0)
        k = -2.0 * weight * w * np.maximum(threshold - m, 0.0) * grad_scale / (N * C)
        psi = np.sign(a)
    return k, psi


# ---------------------------------------------------------------------------------------------------- the kernel's plan
def vector_path(*tensors: torch.Tensor) -> bool:
    """do the shapes, strides and base addresses allow 16-byte (8-byte bf16) accesses on every operand"""
    ok = tensors[0].shape[-1] % 4 == 0
    for t in tensors:
        ok = ok and t.stride(2) % 4 == 0 and t.data_ptr() % (8 if t.dtype == torch.bfloat16 else 16) == 0
    return bool(ok)


def chains(C: int, HW: int, nchunk: int, vec: bool) -> np.ndarray:
    """[C]: the longest chain of fp32 additions behind one (channel, image, chunk) partial sum: L + PR"""
    W = 4 if vec else 1
    nu, UT = C // W, 256 // W
    per = (HW + nchunk - 1) // nchunk
    out = np.zeros(C)
    for z in range((nu + UT - 1) // UT):
        nut = min(UT, nu - z * UT)
        PR = 256 // nut
        out[z * UT * W:(z * UT + nut) * W] = (per + PR - 1) // PR + PR
    return out


# ---------------------------------------------------------------------------------------------------- statistics
def stats_ref(a: torch.Tensor, kind: str, threshold: float, weight: float, channels=None, grad_scale: float = 1.0):
    """-> dict(sums [3, C], pen [C], coef [C]) in float64 from the operand as stored"""
    x = np.abs(f64(a)).reshape(-1, a.shape[-1])
    N, C = x.shape
    t = t32(threshold)
    with np.errstate(invalid="ignore", over="ignore"):
        over = ~(x <= t)
        e = np.where(over, x - t, 0.0)
        sums = np.stack([(e * e).sum(0), x.sum(0), over.sum(0).astype(np.float64)])
        k = weight * mask_of(C, channels)
        if kind == "ceiling":
            pen = k * sums[0] / (N * C)
            coef = 2.0 * k * grad_scale / (N * C) * np.ones(C)
        else:
            r = np.maximum(threshold - sums[1] / N, 0.0)
            pen = k * r * r / C
            coef = -2.0 * k * r * grad_scale / (N * C)
        pen, coef = np.where(k == 0, 0.0, pen), np.where(k == 0, 0.0, coef)
    return {"sums": sums, "pen": pen, "coef": coef, "N": N, "k": k}


def check_stats(got, a: torch.Tensor, kind: str, threshold: float, weight: float, nchunk: int, channels=None,
                grad_scale: float = 1.0, skip_channels=(), vec=None):
    """the device results (sums, pen, coef) against stats_ref within the derived bounds -> the worst error / bound"""
    r = stats_ref(a, kind, threshold, weight, channels, grad_scale)
    sums, pen, coef = (t.detach().cpu().numpy() for t in got)
    B, H, W_, C = a.shape
    N = r["N"]
    assert sums.dtype == np.float64 and sums.shape == (3, C) and pen.dtype == np.float64 and pen.shape == (C,)
    assert coef.dtype == np.float32 and coef.shape == (C,)
    keep = np.ones(C, dtype=bool)
    keep[list(skip_channels)] = False
    ch = chains(C, H * W_, nchunk, vector_path(a) if vec is None else vec)
    bS = (ch + 5) * U * r["sums"][0]
    bA = (ch + 2) * U * r["sums"][1]
    assert np.array_equal(sums[2][keep], r["sums"][2][keep]), "the count is exact"
    k = r["k"]
    if kind == "ceiling":
        bpen = k * bS / (N * C)
        bcoef = U * np.abs(r["coef"]) * (1 + 1e-6)  # one fp32 rounding of a float64 value
    else:
        with np.errstate(invalid="ignore"):
            rr = np.maximum(threshold - r["sums"][1] / N, 0.0)
            dm = bA / N
            bpen = k * (2.0 * rr * dm + dm * dm) / C
            bcoef = 2.0 * k * abs(grad_scale) * dm / (N * C) + U * (np.abs(r["coef"]) + 2.0 * k * abs(grad_scale) * dm / (N * C))
    worst = 0.0
    for name, g_, w_, b_ in (("sum e^2", sums[0], r["sums"][0], bS), ("sum |a|", sums[1], r["sums"][1], bA),
                             ("pen", pen, r["pen"], bpen * (1 + 1e-9) + 1e-300), ("coef", coef.astype(np.float64), r["coef"], bcoef + 1e-46)):
        assert np.isfinite(g_[keep]).all(), name
        with np.errstate(invalid="ignore"):  # (a skipped channel may hold inf - inf)
            err = np.abs(g_ - w_)[keep]
        assert (err <= b_[keep]).all(), (name, np.argwhere(err > b_[keep])[:8], err.max(), b_[keep].max())
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nan_to_num(err / b_[keep], nan=0.0, posinf=0.0).max()) if err.size else 0.0)
    return worst


# ---------------------------------------------------------------------------------------------------- inject
def inject_ref(a: torch.Tensor, g: torch.Tensor, kind: str, threshold: float, coef: torch.Tensor):
    """-> (value float64, bound float64) of out = g + coef[c] * psi(a) for a result stored like g"""
    x, y, k = f64(a), f64(g), f64(coef)
    t = t32(threshold)
    with np.errstate(invalid="ignore", over="ignore"):
        psi = x - np.clip(x, -t, t) if kind == "ceiling" else np.sign(x)
        p = k * psi
        v = y + p
        nr = 2.0 if kind == "ceiling" else 1.0
        b32 = U * (nr * np.abs(p) + np.abs(v)) * 1.001 + 2.0 ** -149
        bound = np.where(p == 0, 0.0, b32)
        if g.dtype == torch.bfloat16:
            bound = np.where(p == 0, 0.0, b32 + 2.0 ** -8 * (np.abs(v) + b32) + 2.0 ** -133)
    return v, bound


def check_inject(out: torch.Tensor, a, g, kind, threshold, coef, skip=None):
    """`out` against inject_ref within the bound; skip: boolean mask of elements not held (non-finite operands) -> worst error / bound"""
    v, bound = inject_ref(a, g, kind, threshold, coef)
    assert out.dtype == g.dtype and tuple(out.shape) == tuple(g.shape) and out.is_contiguous()
    got = f64(out)
    keep = np.ones(v.shape, dtype=bool) if skip is None else ~skip
    assert np.isfinite(got[keep]).all()
    with np.errstate(invalid="ignore"):  # (a skipped element may hold inf - inf)
        err = np.abs(got - v)
    assert (err[keep] <= bound[keep]).all(), (np.argwhere((err > bound) & keep)[:8], err[keep].max())
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nan_to_num(err[keep] / bound[keep], nan=0.0, posinf=0.0).max()) if keep.any() else 0.0


def same_bits(x: torch.Tensor, y: torch.Tensor) -> bool:
    iv = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}[x.dtype]
    return x.dtype == y.dtype and x.shape == y.shape and bool(torch.equal(x.reshape(-1).contiguous().view(iv), y.reshape(-1).contiguous().view(iv)))


def draw(shape, seed: int):
    """(a, g) fp32 on the CPU.  a = randn * s_c + 0.1 with s_c = 2^(c % 5 - 3): against a ceiling of 0.5 and a floor of 0.3
    channels 0 and 1 of every five lie (almost) wholly under the ceiling and have mean |a| under the floor, the others have
    elements over the one and a mean over the other; g = randn * 0.02"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    scale = torch.pow(2.0, (torch.arange(shape[-1]) % 5 - 3).float())
    a = torch.randn(shape, generator=gen) * scale + 0.1
    g = torch.randn(shape, generator=gen) * 0.02
    return a, g


# ---------------------------------------------------------------------------------------------------- engine against the oracle
CEILING_TARGETS = ["vae.decoder.up_blocks.1.resnets.0", "vae.decoder.up_blocks.1.resnets.0.conv2",
                   "vae.decoder.up_blocks.1.upsamplers.0", "vae.decoder"]
FLOOR_TARGETS = ["vae.quant_conv", "vae.encoder.down_blocks.0.resnets.0", "vae.decoder.mid_block"]
CEILING = dict(kind="ceiling", threshold=0.5, weight=1.0)
FLOOR = dict(kind="floor", threshold=0.3, weight=10.0)
ENGINE_TARGETS = [(n, CEILING) for n in CEILING_TARGETS] + [(n, FLOOR) for n in FLOOR_TARGETS]
R_, B_, SEED, KL = 32, 2, 7, 1e-6


def oracle_pass(targets, loss_scale: float = 1.0, step: int = 1):
    """one float64 pass of the oracle (synthetic weights of seed 7, synthetic_pixels / eps(2, 32, 5, step)) with the penalties
    of `targets` = [(module name, dict(kind, threshold, weight[, channels]))] added to the loss through forward hooks.
    -> dict(penalty, terms {name: value}, grads {parameter name: float64 tensor}, stats {name: (share of elements over the
    threshold, channels with mean |a| under it, channels)}, total); the gradients are those of loss_scale * total"""
    import torch.nn.functional as F
    import vae_oracle as vo
    o = vo.OracleWrapper(seed=SEED).double()
    terms, stats, hooks = {}, {}, []
    for name, spec in targets:
        def hook(m, i, out, name=name, spec=spec):
            terms[name] = penalty(out, spec["kind"], spec["threshold"], spec["weight"], spec.get("channels"), channel_dim=1)
            with torch.no_grad():
                ab = out.abs().movedim(1, -1).reshape(-1, out.shape[1])
                stats[name] = (float((ab > spec["threshold"]).double().mean()), int((ab.mean(0) < spec["threshold"]).sum()), out.shape[1])
        hooks.append(o.get_submodule(name).register_forward_hook(hook))
    x, eps = vo.synthetic_pixels(B_, R_, 5, step).double(), vo.synthetic_eps(B_, R_, 5, step).double()
    out = o(x, sample_posterior=True, eps=eps)
    for h in hooks:
        h.remove()
    pen = sum(terms.values()) if terms else torch.zeros((), dtype=torch.float64)
    total = F.mse_loss(out["reconstruction"], x) + KL * out["latent_dist"].kl().mean() + pen
    (loss_scale * total).backward()
    grads = {n: p.grad.detach().clone() for n, p in o.vae.named_parameters()}
    return {"penalty": float(pen.detach()), "terms": {n: float(v.detach()) for n, v in terms.items()}, "grads": grads, "stats": stats,
            "total": float(total.detach())}
