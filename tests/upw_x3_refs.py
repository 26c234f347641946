"""The arithmetic of the fp32 upsampler convolution under split-bf16 products (csrc/conv3_upwino.hip, VAE_UPW_X3 = 1), emulated in
torch on the CPU; shared by tests/test_upw_x3_host.py and tests/test_upw_x3_gpu.py.  Nothing here launches a kernel.

conv3x3(nearest_upsample_2x(x)), forward and dgrad, on the 9 positions p = 3 a + b of the transform domain:
    forward  M[p][t][co] = sum_ci V[t][p][ci] U[p][co][ci],   V = L d3 L^T  (d3: 3x3 patch of the zero-padded low-resolution x, origin
             (i - 1, j - 1)),   U = G' g G'^T (g = w[co, :, :, ci]),   Y[2i + a, 2j + b] = (A'^T M A')[a][b]
    dgrad    M[p][t][ci] = sum_co V[t][p][co] U[p][ci][co],   V = Bt3 d4 Bt3^T (d4: 4x4 patch of the zero-padded dY, origin
             (2i - 1, 2j - 1)),   U = G' rot180(w[co, :, :, ci]) G'^T,   dx[i, j] = s^T M s
    L = [1 -1 0; 0 1 0; 0 1 -1]   Bt3 = [1 0 -1 0; 0 1 1 0; 0 1 0 -1]   G' = [1 0 0; 1 1 1; 0 0 1]   A'^T = [1 1 0; 0 1 -1]   s = [1 1 -1]
Tiles t run (image, row, column) over the low-resolution pixels.  U and V are formed in fp32 (sums in the kernel's association),
split into three bf16 planes, and the contraction runs in steps of 16 channels: per step the six plane products, smallest first,
into the fp32 accumulator.  K is padded to a multiple of 16 with zeros in BOTH operands.

Crafted operands (crafted): x (forward) is non-zero on one low-resolution pixel per 3x3 lattice cell, dY (dgrad) on one pixel per
4x4 cell, so every V value is plus or minus one operand or zero; the weights have ONE non-zero tap per channel pair, tap
(co + ci) % 9, so every U value is one operand or zero and all nine positions receive products.  The operands are c 2^e with
c = 1 + 0.75 2^-8 + 0.375 2^-16, whose planes are exactly (1, 0.75 2^-8, 0.375 2^-16) 2^e: every one of the six terms then has a
known share of a product (tests/test_flat_x3_host.py)."""
import torch

C_CRAFTED = 1 + 0.75 * 2.0 ** -8 + 0.375 * 2.0 ** -16
TERMS = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))  # (plane of V, plane of U), in the order the kernel adds them


def split(a):
    """fp32 tensor -> (hi, mid, lo) as fp32 tensors holding bf16 values; round to nearest even, both subtractions in fp32"""
    hi = a.bfloat16().float()
    r1 = a - hi
    mid = r1.bfloat16().float()
    return hi, mid, (r1 - mid).bfloat16().float()


def crafted(B, H, W, Ci, Co, seed, dgrad):
    """-> (source, w): source = x [B, H, W, Ci] (forward) or dY [B, 2H, 2W, Co] (dgrad), w OHWI [Co, 3, 3, Ci]"""
    g = torch.Generator().manual_seed(seed)
    src = torch.zeros(B, 2 * H, 2 * W, Co) if dgrad else torch.zeros(B, H, W, Ci)
    st = 4 if dgrad else 3
    e = torch.randint(-2, 3, src[:, 1::st, 1::st].shape, generator=g)
    src[:, 1::st, 1::st] = (C_CRAFTED * 2.0 ** e.double()).float()
    w = torch.zeros(Co, 9, Ci)
    co, ci = torch.meshgrid(torch.arange(Co), torch.arange(Ci), indexing="ij")
    ew = torch.randint(-2, 3, (Co, Ci), generator=g)
    w[co, (co + ci) % 9, ci] = (C_CRAFTED * 2.0 ** ew.double()).float()
    return src, w.reshape(Co, 3, 3, Ci)


def transform_v(src, dgrad, dtype=torch.float32):
    """source [B, ., ., K] -> V [T, 9, K] in `dtype` (each value one sum or difference per transform side, as the kernel forms it)"""
    p = torch.nn.functional.pad(src.to(dtype), (0, 0, 1, 1, 1, 1))
    if dgrad:
        d = p.unfold(1, 4, 2).unfold(2, 4, 2)                                   # [B, H, W, K, 4 rows, 4 columns]
        r = torch.stack([d[..., 0, :] - d[..., 2, :], d[..., 1, :] + d[..., 2, :], d[..., 1, :] - d[..., 3, :]], dim=-2)
        v = torch.stack([r[..., 0] - r[..., 2], r[..., 1] + r[..., 2], r[..., 1] - r[..., 3]], dim=-1)
    else:
        d = p.unfold(1, 3, 1).unfold(2, 3, 1)                                   # [B, H, W, K, 3, 3]
        r = torch.stack([d[..., 0, :] - d[..., 1, :], d[..., 1, :], d[..., 1, :] - d[..., 2, :]], dim=-2)
        v = torch.stack([r[..., 0] - r[..., 1], r[..., 1], r[..., 1] - r[..., 2]], dim=-1)
    K = src.shape[3]
    return v.reshape(-1, K, 9).permute(0, 2, 1).contiguous()                    # [T, 9, K]


def transform_u(w, dgrad, dtype=torch.float32):
    """w OHWI [Co, 3, 3, Ci] -> U [9, N, K] in `dtype`, sums in the kernel's association: (g0 + g2) + g1"""
    g = w.to(dtype)
    if dgrad:
        g = g.flip(1, 2).permute(3, 1, 2, 0)                                    # [N = Ci, 3, 3, K = Co], rotated
    t = torch.stack([g[:, 0], (g[:, 0] + g[:, 2]) + g[:, 1], g[:, 2]], dim=1)   # rows:    [N, 3, 3 (b), K]
    u = torch.stack([t[:, :, 0], (t[:, :, 0] + t[:, :, 2]) + t[:, :, 1], t[:, :, 2]], dim=2)  # columns
    N, K = u.shape[0], u.shape[3]
    return u.reshape(N, 9, K).permute(1, 0, 2).contiguous()


def pad16(t):
    K = t.shape[-1]
    return torch.nn.functional.pad(t, (0, -K % 16))


def reference(V, U):
    """float64: M [9, T, N] and S = sum over channels |V| |U| (the scale every error here is measured on)"""
    v, u = V.double().permute(1, 0, 2), U.double().permute(0, 2, 1)            # [9, T, K], [9, K, N]
    return v @ u, v.abs() @ u.abs()


def emulate(V, U, terms=TERMS, planes_v=(0, 1, 2), stale=False, unmasked_tail=False):
    """The kernel's sums: steps of 16 channels, per step the plane products of `terms` in order into an fp32 accumulator.
    planes_v: which plane of V stands where (a swap exchanges two).  stale: the last step reads the V buffer of its parity before
    it was rewritten (the step two before it).  unmasked_tail (K % 16 == 8): the octet behind channel K of both operands holds
    the octet in front of it instead of zeros."""
    K = V.shape[2]
    Vp, Up = pad16(V), pad16(U)
    if unmasked_tail:
        assert K % 16 == 8
        Vp[..., K:], Up[..., K:] = Vp[..., K - 8:K].clone(), Up[..., K - 8:K].clone()
    pv, pu = split(Vp), split(Up)
    pv = [pv[i] for i in planes_v]
    ns = Vp.shape[2] // 16
    acc = torch.zeros(9, V.shape[0], U.shape[1])
    for s in range(ns):
        sv = s - 2 if (stale and s == ns - 1) else s
        assert sv >= 0
        for i, j in terms:
            acc = acc + pv[i][:, :, sv * 16:sv * 16 + 16].permute(1, 0, 2) @ pu[j][:, :, s * 16:s * 16 + 16].permute(0, 2, 1)
    return acc


def output(M, dgrad, magnitude=False):
    """M [9, T, N] -> forward [T, 2, 2, N] = A'^T M A', dgrad [T, N] = s^T M s, in M's dtype and the kernel's association;
    magnitude: every sign plus (|A'|, |s|: how far an error of M can reach)"""
    m = M.reshape(3, 3, *M.shape[1:])
    sub = (lambda a, b: a + b) if magnitude else (lambda a, b: a - b)
    if dgrad:
        h = [sub(m[0][j] + m[1][j], m[2][j]) for j in range(3)]
        return sub(h[0] + h[1], h[2])
    h = [[m[0][j] + m[1][j] for j in range(3)], [sub(m[1][j], m[2][j]) for j in range(3)]]
    return torch.stack([torch.stack([h[a][0] + h[a][1], sub(h[a][1], h[a][2])], dim=1) for a in range(2)], dim=1)


def image(out, B, H, W, dgrad):
    """output() -> NHWC: forward [B, 2H, 2W, N], dgrad [B, H, W, N]"""
    N = out.shape[-1]
    if dgrad:
        return out.reshape(B, H, W, N)
    return out.reshape(B, H, W, 2, 2, N).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, N)


def rel_err(out, ref, scale):
    """max |out - ref| / scale over the elements with scale > 0; elements without any product must be exactly zero"""
    live = scale > 0
    assert bool(live.any()) and not bool(out[~live].any())
    return float(((out.double() - ref).abs()[live] / scale[live]).max())


def mistakes(V, U):
    """name -> the sums with one single mistake: a dropped term, a doubled term, two planes of V swapped, a stale double-buffer
    side, a missing K-tail mask"""
    out = {}
    for t in range(6):
        out[f"term {TERMS[t]} dropped"] = emulate(V, U, terms=TERMS[:t] + TERMS[t + 1:])
        out[f"term {TERMS[t]} doubled"] = emulate(V, U, terms=TERMS[:t + 1] + TERMS[t:])
    for a, b in ((0, 1), (0, 2), (1, 2)):
        p = [0, 1, 2]
        p[a], p[b] = p[b], p[a]
        out[f"planes {a} and {b} of V swapped"] = emulate(V, U, planes_v=tuple(p))
    if V.shape[2] > 32:
        out["last step on a stale V buffer"] = emulate(V, U, stale=True)
    if V.shape[2] % 16 == 8:
        out["K tail not masked"] = emulate(V, U, unmasked_tail=True)
    return out


def crafted_sides(B, H, W, Ci, Co, seed, dgrad):
    """the crafted case -> (source, w, float64 output, its scale, the emulated correct form's error, the smallest single
    mistake's error, name -> error of every mistake), outputs as output() returns them"""
    src, w = crafted(B, H, W, Ci, Co, seed, dgrad)
    V, U = transform_v(src, dgrad), transform_u(w, dgrad)
    M, S = reference(V, U)
    ref, scale = output(M, dgrad), output(S, dgrad, magnitude=True)
    e_ok = rel_err(output(emulate(V, U), dgrad), ref, scale)
    errs = {k: rel_err(output(m, dgrad), ref, scale) for k, m in mistakes(V, U).items()}
    return src, w, ref, scale, e_ok, min(errs.values()), errs


def bar_between(e_ok, e_bad):
    """The bar of a crafted case, from its two measured sides: the geometric mean of the correct form's error and the smallest
    single mistake's.  It is a bar only if the sides are apart: the smallest mistake at least 4 x the correct form's error."""
    assert e_bad >= 4 * e_ok, f"the smallest single mistake ({e_bad:.3e}) is not clear of the correct form ({e_ok:.3e})"
    return (max(e_ok, 1e-12) * e_bad) ** 0.5
