"""The arithmetic of the fp32 Winograd weight gradient under split-bf16 products (csrc/wgrad3_wino.hip, VAE_WGRAD_X3 = 1), emulated
in torch on the CPU; shared by tests/test_wgrad_x3_host.py and tests/test_wgrad_x3_gpu.py.  Nothing here launches a kernel.

The kernel's transform-domain sums (what its slab holds, summed over the splits):
    M[p][ci][co] = sum over tiles t of V[t][p][ci] * D'[t][p][co],      p = 4 i + j,
    V = B^T d B (d: the 4x4 patch of the zero-padded input with origin 2t - 1),   D' = G' dy G'^T (dy: the 2x2 block of dY),
    B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1],   G' = [1 0; 1 1; 1 -1; 0 1]   (the halves of G are the reduction's).
Tiles run (image, tile row, tile column) row-major; 8 consecutive tiles are a unit, 16 a step: the K of one MFMA per plane pair.
V and D' are formed in fp32, split into three bf16 planes, and a step adds the six plane products, smallest first, to the fp32
accumulator.  An odd last unit is paired with a unit of zeros.

Crafted operands (crafted_xy): x is non-zero on one pixel per 4x4 lattice cell and dy on one pixel per 2x2 block, so every V and
D' value is plus or minus one operand; the operands are c 2^e with c = 1 + 0.75 2^-8 + 0.375 2^-16, whose planes are exactly
(1, 0.75 2^-8, 0.375 2^-16) 2^e: every one of the six terms then has a known share of a product (tests/test_flat_x3_host.py)."""
import torch

C_CRAFTED = 1 + 0.75 * 2.0 ** -8 + 0.375 * 2.0 ** -16
TERMS = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))  # (plane of V, plane of D'), in the order the kernel adds them
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float32)
GP = torch.tensor([[1, 0], [1, 1], [1, -1], [0, 1]], dtype=torch.float32)


def split(a):
    """fp32 tensor -> (hi, mid, lo) as fp32 tensors holding bf16 values; round to nearest even, both subtractions in fp32"""
    hi = a.bfloat16().float()
    r1 = a - hi
    mid = r1.bfloat16().float()
    return hi, mid, (r1 - mid).bfloat16().float()


def crafted_xy(B, H, W, Ci, Co, seed):
    """x [B, H, W, Ci] non-zero where y % 4 == 1 and x % 4 == 1, dy [B, H, W, Co] non-zero where y % 2 == 0 and x % 2 == 0:
    the 9 positions i, j <= 2 of the transform domain receive products, the other 7 stay exactly zero"""
    g = torch.Generator().manual_seed(seed)
    x, dy = torch.zeros(B, H, W, Ci), torch.zeros(B, H, W, Co)
    ex = torch.randint(-2, 3, x[:, 1::4, 1::4].shape, generator=g)
    ey = torch.randint(-2, 3, dy[:, 0::2, 0::2].shape, generator=g)
    x[:, 1::4, 1::4] = (C_CRAFTED * 2.0 ** ex.double()).float()
    dy[:, 0::2, 0::2] = (C_CRAFTED * 2.0 ** ey.double()).float()
    return x, dy


def transforms(x, dy, dtype=torch.float32):
    """x [B, H, W, Ci], dy [B, H, W, Co] (H even, W % 16 == 0) -> V [T, 16, Ci], D' [T, 16, Co] in `dtype`, tiles in the kernel's order"""
    B, H, W, Ci = x.shape
    xp = torch.nn.functional.pad(x.to(dtype), (0, 0, 1, 1, 1, 1))                     # [B, H + 2, W + 2, Ci]
    d = xp.unfold(1, 4, 2).unfold(2, 4, 2)                                            # [B, H/2, W/2, Ci, 4 (rows), 4 (columns)]
    V = torch.einsum("ir,byxcrs,js->byxijc", BT.to(dtype), d, BT.to(dtype))
    e = dy.to(dtype).unfold(1, 2, 2).unfold(2, 2, 2)                                  # [B, H/2, W/2, Co, 2, 2]
    D = torch.einsum("ir,byxcrs,js->byxijc", GP.to(dtype), e, GP.to(dtype))
    return V.reshape(-1, 16, Ci).contiguous(), D.reshape(-1, 16, dy.shape[3]).contiguous()


def reference(V, D):
    """float64: M [16, Ci, Co] and S = sum over tiles |V| |D'| (the scale every error here is measured on)"""
    v, d = V.double().permute(1, 2, 0), D.double().permute(1, 0, 2)                   # [16, Ci, T], [16, T, Co]
    return v @ d, v.abs() @ d.abs()


def emulate(V, D, terms=TERMS, planes_v=(0, 1, 2), stale=False):
    """The kernel's sums: steps of 16 tiles, per step the plane products of `terms` in order into an fp32 accumulator.
    planes_v: which plane of V stands where (a swap exchanges two).  stale: an odd last unit is paired with the unit before it
    (the data a stage would still hold) instead of zeros."""
    T = V.shape[0]
    assert T % 8 == 0
    if (T // 8) % 2:
        fill = slice(T - 8, T) if stale else None
        V = torch.cat([V, V[fill] if stale else torch.zeros_like(V[:8])])
        D = torch.cat([D, D[fill] if stale else torch.zeros_like(D[:8])])
    pv, pd = split(V), split(D)
    pv = [pv[i] for i in planes_v]
    acc = torch.zeros(16, V.shape[2], D.shape[2])
    for s in range(0, V.shape[0], 16):
        for i, j in terms:
            acc = acc + pv[i][s:s + 16].permute(1, 2, 0) @ pd[j][s:s + 16].permute(1, 0, 2)
    return acc


def rel_err(M, ref, S):
    """max |M - ref| / S over the elements with S > 0; elements without any product must be exactly zero"""
    live = S > 0
    assert bool(live.any()) and not bool(M[~live].any())
    return float(((M.double() - ref).abs()[live] / S[live]).max())


def mistakes(V, D):
    """name -> the sums with one single mistake: a dropped term, a doubled term, two planes of V swapped, a stale partner unit"""
    out = {}
    for t in range(6):
        out[f"term {TERMS[t]} dropped"] = emulate(V, D, terms=TERMS[:t] + TERMS[t + 1:])
        out[f"term {TERMS[t]} doubled"] = emulate(V, D, terms=TERMS[:t + 1] + TERMS[t:])
    for a, b in ((0, 1), (0, 2), (1, 2)):
        p = [0, 1, 2]
        p[a], p[b] = p[b], p[a]
        out[f"planes {a} and {b} of V swapped"] = emulate(V, D, planes_v=tuple(p))
    if (V.shape[0] // 8) % 2:
        out["odd unit paired with stale data"] = emulate(V, D, stale=True)
    return out


def bar_between(e_ok, e_bad):
    """The bar of a crafted case, from its two measured sides: the geometric mean of the correct form's error and the smallest
    single mistake's.  It is a bar only if the sides are apart: the smallest mistake at least 4 x the correct form's error."""
    assert e_bad >= 4 * e_ok, f"the smallest single mistake ({e_bad:.3e}) is not clear of the correct form ({e_ok:.3e})"
    return (max(e_ok, 1e-12) * e_bad) ** 0.5
