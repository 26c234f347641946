"""The arithmetic of the fp32 upsampler weight gradient under split-bf16 products (csrc/wgrad3_upwino.hip, VAE_UPWGRAD_X3 = 1),
emulated in torch on the CPU; shared by tests/test_upwgrad_x3_host.py and tests/test_upwgrad_x3_gpu.py.  Nothing here launches a
kernel.

The weight gradient of conv3x3(nearest_upsample_2x(x)) on the 9 positions p = 3 a + b of the transform domain (what the kernel's
slab holds, summed over the splits):
    M[p][ci][co] = sum over low-resolution pixels t of V[t][p][ci] * D[t][p][co]
    V = L d3 L^T   (d3: the 3x3 patch of the zero-padded low-resolution x with origin (i - 1, j - 1): tests/upw_x3_refs.py)
    D = G'' dy G''^T   (dy: the 2x2 block of dY that belongs to pixel (i, j))
    dW = A''^T M A''     L = [1 -1 0; 0 1 0; 0 1 -1]   G'' = [1 0; 1 1; 0 1]   A''^T = [1 1 0; 0 1 0; 0 1 -1]
Pixels run (image, row, column) row-major; 8 consecutive pixels of a row are a unit.  A split walks its unit range in PAIRS, 16
pixels: the K of one MFMA per plane pair; a range with an odd count pairs its last unit with a unit of zeros.  V and D are formed
in fp32 (rows first, then columns), split into three bf16 planes, and a pair adds the six plane products, smallest first, to the
fp32 accumulator.

Crafted operands (crafted_xy): x is non-zero on one pixel per 3x3 lattice cell and dY on one pixel per 2x2 block (the corner
(i % 2, j % 2): all nine positions receive products), so every V and D value is plus or minus one operand or zero; the operands are
c 2^e with c = 1 + 0.75 2^-8 + 0.375 2^-16, whose planes are exactly (1, 0.75 2^-8, 0.375 2^-16) 2^e: every one of the six terms
then has a known share of a product (tests/test_flat_x3_host.py)."""
import torch
import torch.nn.functional as F

from upw_x3_refs import C_CRAFTED, TERMS, bar_between, split, transform_v  # noqa: F401  (re-exported)


def crafted_xy(B, H, W, Ci, Co, seed):
    """x [B, H, W, Ci] non-zero where y % 3 == 1 and x % 3 == 1; dY [B, 2H, 2W, Co] non-zero on corner (i % 2, j % 2) of the block
    of pixel (i, j)"""
    g = torch.Generator().manual_seed(seed)
    x, dy = torch.zeros(B, H, W, Ci), torch.zeros(B, 2 * H, 2 * W, Co)
    ex = torch.randint(-2, 3, x[:, 1::3, 1::3].shape, generator=g)
    x[:, 1::3, 1::3] = (C_CRAFTED * 2.0 ** ex.double()).float()
    ey = torch.randint(-2, 3, (B, H, W, Co), generator=g)
    val = (C_CRAFTED * 2.0 ** ey.double()).float()
    blocks = dy.reshape(B, H, 2, W, 2, Co)
    i, j = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    blocks[:, i, i % 2, j, j % 2] = val
    return x, dy


def transforms(x, dy, dtype=torch.float32):
    """x [B, H, W, Ci], dy [B, 2H, 2W, Co] -> V [T, 9, Ci], D [T, 9, Co] in `dtype`, pixels in the kernel's order; each value one
    sum or difference per transform side, rows first, as the kernel forms it"""
    B, H, W, _ = x.shape
    Co = dy.shape[3]
    V = transform_v(x, False, dtype)
    e = dy.to(dtype).reshape(B, H, 2, W, 2, Co)
    r = [e[:, :, 0], e[:, :, 0] + e[:, :, 1], e[:, :, 1]]                       # rows: [B, H, W, 2 (columns), Co]
    D = torch.stack([c for ra in r for c in (ra[:, :, :, 0], ra[:, :, :, 0] + ra[:, :, :, 1], ra[:, :, :, 1])], dim=3)  # [B, H, W, 9, Co]
    return V, D.reshape(-1, 9, Co).contiguous()


def reference(V, D):
    """float64: M [9, Ci, Co] and S = sum over pixels |V| |D| (the scale every error here is measured on)"""
    v, d = V.double().permute(1, 2, 0), D.double().permute(1, 0, 2)             # [9, Ci, T], [9, T, Co]
    return v @ d, v.abs() @ d.abs()


def unit_ranges(units, nsplit):
    """the kernel's split of `units` units: [(first, count)] per split (a split beyond the range has none)"""
    per = -(-units // nsplit)
    return [(s * per, max(0, min(units, (s + 1) * per) - s * per)) for s in range(nsplit)]


def emulate(V, D, nsplit=1, terms=TERMS, planes_v=(0, 1, 2), stale=False):
    """The kernel's slab [nsplit, 9, Ci, Co]: per split its units in pairs, per pair the plane products of `terms` in order into an
    fp32 accumulator.  planes_v: which plane of V stands where (a swap exchanges two).  stale: an odd last unit is paired with the
    unit before it in memory (what a stage would still hold) instead of zeros."""
    T = V.shape[0]
    assert T % 8 == 0
    out = torch.zeros(nsplit, 9, V.shape[2], D.shape[2])
    for s, (u0, nu) in enumerate(unit_ranges(T // 8, nsplit)):
        v, d = V[8 * u0:8 * (u0 + nu)], D[8 * u0:8 * (u0 + nu)]
        if nu % 2:
            fill = slice(8 * (u0 + nu - 2), 8 * (u0 + nu - 1)) if (stale and u0 + nu >= 2) else None
            v = torch.cat([v, V[fill] if fill else torch.zeros_like(V[:8])])
            d = torch.cat([d, D[fill] if fill else torch.zeros_like(D[:8])])
        pv, pd = split(v), split(d)
        pv = [pv[i] for i in planes_v]
        for k in range(0, v.shape[0], 16):
            for i, j in terms:
                out[s] = out[s] + pv[i][k:k + 16].permute(1, 2, 0) @ pd[j][k:k + 16].permute(1, 0, 2)
    return out


def rel_err(M, ref, S):
    """max |M - ref| / S over the elements with S > 0; elements without any product must be exactly zero"""
    live = S > 0
    assert bool(live.any()) and not bool(M[~live].any())
    return float(((M.double() - ref).abs()[live] / S[live]).max())


def mistakes(V, D, nsplit=1):
    """name -> the slab sums with one single mistake: a dropped term, a doubled term, two planes of V swapped, a stale partner unit"""
    out = {}
    for t in range(6):
        out[f"term {TERMS[t]} dropped"] = emulate(V, D, nsplit, terms=TERMS[:t] + TERMS[t + 1:])
        out[f"term {TERMS[t]} doubled"] = emulate(V, D, nsplit, terms=TERMS[:t + 1] + TERMS[t:])
    for a, b in ((0, 1), (0, 2), (1, 2)):
        p = [0, 1, 2]
        p[a], p[b] = p[b], p[a]
        out[f"planes {a} and {b} of V swapped"] = emulate(V, D, nsplit, planes_v=tuple(p))
    if any(nu % 2 and u0 + nu >= 2 for u0, nu in unit_ranges(V.shape[0] // 8, nsplit)):
        out["odd unit paired with stale data"] = emulate(V, D, nsplit, stale=True)
    return {k: m.sum(dim=0) for k, m in out.items()}


def output(M):
    """M [9, Ci, Co] -> dW OHWI [Co, 3, 3, Ci] = A''^T M A'' in M's dtype (rows [1 1 0], [0 1 0], [0 1 -1])"""
    m = M.reshape(3, 3, *M.shape[1:])
    rows = [m[0] + m[1], m[1], m[1] - m[2]]                                     # [3 (b), Ci, Co] each
    taps = [[r[0] + r[1], r[1], r[1] - r[2]] for r in rows]
    return torch.stack([torch.stack(t, dim=0) for t in taps], dim=0).permute(3, 0, 1, 2).contiguous()


def dw_f64(x, dy):
    """float64 weight gradient of conv3x3(nearest_upsample_2x(x)), OHWI [Co, 3, 3, Ci], and the bias gradient [Co]"""
    up = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    w0 = torch.zeros(dy.shape[3], x.shape[3], 3, 3, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad(F.conv2d(up, w0, None, 1, 1), w0, dy.double().permute(0, 3, 1, 2))
    return gw.permute(0, 2, 3, 1).contiguous(), dy.double().sum(dim=(0, 1, 2))


def bias_partials_f32(dy, W, nsplit):
    """The kernel's bias partials [nsplit, Co] replayed in float32: per split, dY column xx (0..15) of the units' 2 x 16 strips is
    summed unit by unit, row 0 before row 1, then the 16 columns in a tree of neighbouring pairs (the lane shuffles of bias_tail)"""
    B, H2, W2, Co = dy.shape
    strips = W // 8
    d = dy.reshape(B, H2 // 2, 2, strips, 16, Co).permute(0, 1, 3, 2, 4, 5).reshape(-1, 2, 16, Co)  # [unit][row][column][co]
    out = torch.zeros(nsplit, Co)
    for s, (u0, nu) in enumerate(unit_ranges(d.shape[0], nsplit)):
        acc = torch.zeros(16, Co)
        for u in range(u0, u0 + nu):
            acc = (acc + d[u, 0]) + d[u, 1]
        while acc.shape[0] > 1:
            acc = acc[0::2] + acc[1::2]
        out[s] = acc[0]
    return out
