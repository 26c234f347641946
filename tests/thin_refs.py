"""float64 references, operand builders, case tables and criteria for the six kernels that serve the <= 4-channel convolutions
(a helper module, not a test):

  csrc/skinny.hip            conv_smallk_kernel, wgrad_smallk_kernel<SMALL_X,XF>, conv_smalln_kernel<XF>      fp32 on the VALU
  csrc/conv_thin_bf16.hip    conv_thin_bf16_kernel, conv_thinn_bf16_kernel<XF>                                 matrix pipe
  csrc/wgrad_thin_bf16.hip   wgrad_thin_bf16_kernel<SMALL_X,XF>                                                matrix pipe

A case is a launch described by integers: the kernel instantiation it is for, the layer, the map, the channel counts, the storage
flags, the library option and (weight gradient) the split count.  rows_block / wg_block turn it into the argument block the C
ABI takes, with placeholder pointers; tests/test_thin_edges_host.py holds every block to the kernel name its case states (no GPU
needed), tests/test_thin_edges_gpu.py puts the pointers in and launches.

References are float64 on the host: F.conv2d, autograd for the gradients.  For a matrix-pipe kernel the reference rounds where
the kernel rounds (r16: the narrow operand, the weights, an fp32 tensor the kernel rounds when it stages it, the
GroupNorm(+SiLU)-transformed wide operand); products are of rounded operands, sums float64.  The same functions with
acc = float32 are a correct implementation with another summation order, and with one `mut` switched on a wrong one: the host
test shows that the criteria accept the first and reject each of the second.

Criteria (bars of tests/bf16_refs.py / tests/conv_routes.py): forward / dgrad 2e-5, weight gradient 3e-5, with a fused
GroupNorm 5e-5, of max |v|; a bf16 result gets ulp_bf16(v) / 2 per element on top.  A matrix-pipe kernel with a transform rounds
fp32 transforms to bf16, and a float64 transform rounds a few elements to the other neighbour: its bar is
streaming_refs.bar(4, fp32_cpu, floor) with fp32_cpu the error of the same case with the transform in torch float32 on the CPU.
"""
from __future__ import annotations

import ctypes as C
import zlib
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

import bf16_refs as br
import streaming_refs as sr

TP = 128                 # pixels per tile of the five kernels that walk linear pixels
SN_TH, SN_TW = 4, 32     # conv_smalln / conv_thinn: 4 x 32-pixel tiles
U = 2.0 ** -24
XF_NONE, XF_AFFINE, XF_AFFINE_SILU = 0, 1, 2
FAR = 1e4                # what an unused channel of a wider storage holds
MAX_WGRAD_PIXELS = 3072

# every instantiation of the six kernels (dispatch.cpp: rows_kernel_name / wgrad_kernel_name)
INSTANTIATIONS = (
    "conv_smallk_kernel",
    "wgrad_smallk_kernel<true,0>", "wgrad_smallk_kernel<false,0>", "wgrad_smallk_kernel<false,1>", "wgrad_smallk_kernel<false,2>",
    "conv_smalln_kernel<0>", "conv_smalln_kernel<1>", "conv_smalln_kernel<2>",
    "conv_thin_bf16_kernel",
    "conv_thinn_bf16_kernel<0>", "conv_thinn_bf16_kernel<1>", "conv_thinn_bf16_kernel<2>",
    "wgrad_thin_bf16_kernel<true,0>", "wgrad_thin_bf16_kernel<false,0>", "wgrad_thin_bf16_kernel<false,1>", "wgrad_thin_bf16_kernel<false,2>",
)


def family(kernel: str) -> str:
    return kernel.split("<")[0]


def matrix_pipe(kernel: str) -> bool:
    return family(kernel) in ("conv_thin_bf16_kernel", "conv_thinn_bf16_kernel", "wgrad_thin_bf16_kernel")


# ---------------------------------------------------------------------------------------------------- geometry
def out_hw(kind, H, W):
    if kind == "c3s2":   # padding (0, 1, 0, 1)
        return (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1
    if kind == "c3up":
        return 2 * H, 2 * W
    return H, W


def taps_of(kind):
    return 1 if kind == "c1" else 9


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def gather_index(kind, H, W):
    """the kernels' own pixel mapping (csrc/common.h: src_pixel), restated by hand: [Ho*Wo, taps] -> source pixel sy * W + sx of
    output pixel (y, x) and tap (kh, kw), or -1 where the tap meets padding"""
    Ho, Wo = out_hw(kind, H, W)
    k = 1 if kind == "c1" else 3
    y, x = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
    idx = torch.full((Ho, Wo, k * k), -1, dtype=torch.int64)
    for kh in range(k):
        for kw in range(k):
            if kind == "c3up":   # tap of the 3x3 kernel on the virtual 2H x 2W map, read at half the coordinates
                uy, ux = y + kh - 1, x + kw - 1
                ok = (uy >= 0) & (uy < 2 * H) & (ux >= 0) & (ux < 2 * W)
                sy, sx = uy >> 1, ux >> 1
            else:
                stride, pad = (2, 0) if kind == "c3s2" else (1, 0 if kind == "c1" else 1)
                sy, sx = y * stride + kh - pad, x * stride + kw - pad
                ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
            idx[:, :, kh * k + kw] = torch.where(ok, sy * W + sx, torch.full_like(sy, -1))
    return idx.reshape(Ho * Wo, k * k)


def patches(x, kind):
    """im2col by the hand-written mapping: x [B,H,W,C] -> [B, Ho*Wo, taps, C], zeros at padding"""
    B, H, W, Cc = x.shape
    idx = gather_index(kind, H, W)
    flat = torch.cat([x.reshape(B, H * W, Cc), torch.zeros(B, 1, Cc, dtype=x.dtype)], dim=1)   # (index -1 reads the zero row)
    return flat[:, idx]


def fwd_by_hand(x, w, kind):
    """x [B,H,W,Ci], w [Co,taps,Ci] -> [B,Ho,Wo,Co]"""
    B, H, W, _ = x.shape
    Ho, Wo = out_hw(kind, H, W)
    return torch.einsum("bptc,otc->bpo", patches(x, kind), w).reshape(B, Ho, Wo, -1)


def wgrad_by_hand(dy, x, kind):
    """-> [Co,taps,Ci]"""
    B = x.shape[0]
    return torch.einsum("bpo,bptc->otc", dy.reshape(B, -1, dy.shape[-1]), patches(x, kind))


def dgrad_by_hand(dy, w, kind, H, W):
    """dy [B,Ho,Wo,Co], w [Co,taps,Ci] -> [B,H,W,Ci]: every (output pixel, tap) adds dy . w[:, tap] to its source pixel"""
    B = dy.shape[0]
    idx = gather_index(kind, H, W)
    contrib = torch.einsum("bpo,otc->bptc", dy.reshape(B, -1, dy.shape[-1]), w)             # [B, P, taps, Ci]
    dx = torch.zeros(B, H * W + 1, w.shape[-1], dtype=dy.dtype)
    dx.index_add_(1, torch.where(idx < 0, torch.full_like(idx, H * W), idx).reshape(-1), contrib.reshape(B, -1, w.shape[-1]))
    return dx[:, :H * W].reshape(B, H, W, -1)


def _oihw(w, kind):
    k = 1 if kind == "c1" else 3
    return w.reshape(w.shape[0], k, k, w.shape[-1]).permute(0, 3, 1, 2)


def _seed(cid: str) -> int:
    return zlib.crc32(cid.encode()) & 0x7FFFFFFF


def _silu(a):
    return a * torch.sigmoid(a)


def _transform(x, scale, shift, xf, bidx=None):
    """x [B,H,W,C] in its arithmetic dtype; bidx [B,H,W]: the image whose scale / shift row a pixel is given (None: its own)"""
    if xf == XF_NONE:
        return x
    if bidx is None:
        a = x * scale.to(x.dtype)[:, None, None, :] + shift.to(x.dtype)[:, None, None, :]
    else:
        a = x * scale.to(x.dtype)[bidx] + shift.to(x.dtype)[bidx]
    return _silu(a) if xf == XF_AFFINE_SILU else a


# ---------------------------------------------------------------------------------------------------- rows form: cases
class Rows(NamedTuple):
    id: str
    kernel: str
    form: str              # fwd | dgrad
    kind: str              # c3 | c3s2 | c3up | c1: the LAYER
    shape: tuple           # B, H, W of the layer's forward input map
    Cs: int                # fwd: channels of the input's storage (>= Ci); dgrad: unused (the gradient has exactly Co)
    Co: int
    Ci: int
    xf: int = XF_NONE
    bias: bool = True
    track: bool = False
    bf16: bool = False     # arithmetic mode (prec)
    out16: bool = False    # storage flags
    a16: bool = False
    no_thin: bool = False  # library option no_thin_mfma


MAP_B = (3, 10, 10)        # 300 pixels: 3 tiles, the last with 44 rows, image boundaries inside tiles
MAP_S = (2, 9, 11)         # 198 pixels: 2 tiles, the last with 70 rows
MAP_T = (4, 8, 12)         # 384 pixels = 3 whole tiles over images of 96 pixels: tiles 0, 1, 2 straddle images
MAP_N = (2, 8, 64)         # 2 x 2 tiles of 4 x 32 per image, two images
LARGE = (1, 411, 640)      # 263040 pixels = 2055 tiles: 2 tiles per workgroup, the last of 1028 workgroups gets one

_SK, _TK = "conv_smallk_kernel", "conv_thin_bf16_kernel"
SMALLK_CASES = (
    Rows("smallk-c3-ragged", _SK, "fwd", "c3", MAP_B, 4, 128, 3, track=True),
    Rows("smallk-k1", _SK, "fwd", "c3", MAP_S, 1, 128, 1),
    Rows("smallk-k2", _SK, "fwd", "c3", MAP_S, 2, 128, 2, bias=False),
    Rows("smallk-k4", _SK, "fwd", "c3", MAP_S, 4, 128, 4, track=True),
    Rows("smallk-n96", _SK, "fwd", "c3", MAP_S, 4, 96, 3, track=True),
    Rows("smallk-n160", _SK, "fwd", "c3", MAP_S, 4, 160, 3, track=True),
    Rows("smallk-dgrad", _SK, "dgrad", "c3", MAP_S, 3, 3, 128, bias=False),
    Rows("smallk-c3s2", _SK, "fwd", "c3s2", (1, 10, 14), 4, 128, 3),
    Rows("smallk-c3s2-dgrad", _SK, "dgrad", "c3s2", (1, 10, 14), 3, 3, 128, bias=False),
    Rows("smallk-c3up", _SK, "fwd", "c3up", (1, 5, 6), 4, 128, 4, track=True),
    Rows("smallk-c1", _SK, "fwd", "c1", (2, 5, 7), 4, 128, 4),
    Rows("smallk-out16", _SK, "fwd", "c3", MAP_B, 4, 128, 3, track=True, bf16=True, out16=True),   # M % 128 != 0: no thin kernel
)
THIN_CASES = (
    Rows("thin-straddle", _TK, "fwd", "c3", MAP_T, 4, 128, 3, track=True, bf16=True, out16=True),
    Rows("thin-k1", _TK, "fwd", "c3", MAP_T, 1, 128, 1, track=True, bf16=True, out16=True),
    Rows("thin-k2", _TK, "fwd", "c3", MAP_T, 2, 128, 2, bf16=True, out16=True),                      # tracker off
    Rows("thin-k4", _TK, "fwd", "c3", MAP_T, 4, 128, 4, bias=False, track=True, bf16=True, out16=True),
    Rows("thin-n256", _TK, "fwd", "c3", MAP_T, 4, 256, 3, track=True, bf16=True, out16=True),
    Rows("thin-dgrad", _TK, "dgrad", "c3", (2, 16, 16), 3, 3, 128, bias=False, bf16=True, out16=True),
)
THIN_LARGE = Rows("thin-large", _TK, "fwd", "c3", LARGE, 4, 128, 3, track=True, bf16=True, out16=True)


def _sn(i, K, Cs, N, xf, bias=True, bf16=False, a16=False, no_thin=False):
    return Rows(f"smalln-{i}-k{K}of{Cs}-n{N}-xf{xf}", f"conv_smalln_kernel<{xf}>", "fwd", "c3", MAP_N, Cs, N, K, xf=xf, bias=bias,
                bf16=bf16, a16=a16, no_thin=no_thin)


def _tn(i, K, Cs, N, xf, bias=True):
    return Rows(f"thinn-{i}-k{K}of{Cs}-n{N}-xf{xf}", f"conv_thinn_bf16_kernel<{xf}>", "fwd", "c3", MAP_N, Cs, N, K, xf=xf, bias=bias,
                bf16=True, a16=True)


# K = 32: one chunk, no prefetch; 96: three; 128: four.  N = 1..4; XF 0, 1, 2; bias on and off; K of a wider storage
SMALLN_CASES = (
    _sn(0, 32, 32, 1, 0, bias=False), _sn(1, 32, 32, 3, 2), _sn(2, 96, 96, 2, 1), _sn(3, 96, 96, 4, 0), _sn(4, 128, 128, 3, 2),
    _sn(5, 128, 128, 4, 1, bias=False), _sn(6, 32, 64, 3, 2),
    # bf16 input in bf16 mode: K = 96 gets to the VALU kernel by itself (256 % 12 != 0), K = 128 with the option
    _sn(7, 96, 96, 3, 2, bf16=True, a16=True), _sn(8, 96, 96, 1, 0, bf16=True, a16=True), _sn(9, 128, 128, 3, 1, bf16=True, a16=True, no_thin=True),
)
# K = 32, 64, 128: 1, 2 and 4 passes of the halo loop
THINN_CASES = (
    _tn(0, 32, 32, 1, 0), _tn(1, 32, 32, 3, 2), _tn(2, 64, 64, 4, 1), _tn(3, 64, 64, 3, 0), _tn(4, 128, 128, 3, 2), _tn(5, 128, 128, 1, 1),
    _tn(6, 128, 128, 4, 0, bias=False), _tn(7, 32, 64, 3, 2),
)
ROWS_CASES = SMALLK_CASES + THIN_CASES + SMALLN_CASES + THINN_CASES   # (THIN_LARGE has tests of its own)


def rows_case(cid: str) -> Rows:
    return {c.id: c for c in ROWS_CASES + (THIN_LARGE,)}[cid]


def rows_dims(c: Rows):
    """-> rows M of the output, N, K, (Hr, Wr) of the row grid"""
    B, H, W = c.shape
    Hr, Wr = (H, W) if c.form == "dgrad" else out_hw(c.kind, H, W)
    return B * Hr * Wr, (c.Ci if c.form == "dgrad" else c.Co), (c.Co if c.form == "dgrad" else c.Ci), (Hr, Wr)


def _placeholder():
    return C.c_void_p(256)   # (what ops._UNALLOCATED is: a non-null pointer with the alignment of a device allocation)


def rows_block(c: Rows, ops):
    """the launch's argument block with placeholder pointers; the GPU test replaces each by a tensor's"""
    B, H, W = c.shape
    prec = ops.PREC_BF16 if c.bf16 else ops.PREC_F32
    if c.form == "fwd":
        a = ops.fwd_args(c.kind, B, H, W, c.Cs, c.Co, c.Ci, xf=c.xf, prec=prec)
    else:
        a = ops.dgrad_args(c.kind, B, H, W, c.Co, c.Ci, s2=False, prec=prec)
    a.A, a.W, a.C = _placeholder(), _placeholder(), _placeholder()
    if c.bias:
        a.bias = _placeholder()
    if c.track:
        a.track = _placeholder()
    if c.xf != XF_NONE:
        a.scale, a.shift = _placeholder(), _placeholder()
    a.out_bf16, a.a_bf16 = int(c.out16), int(c.a16)
    return a


def kernel_name(lib, fn: str, a) -> str:
    buf = C.create_string_buffer(128)
    lib.call(fn, C.byref(a), buf, 128)
    return buf.value.decode()


# ---------------------------------------------------------------------------------------------------- rows form: operands, values
class RowsOps(NamedTuple):
    src: torch.Tensor                 # fwd: x [B,H,W,Cs]; dgrad: dy [B,Ho,Wo,Co]; as stored (fp32 or bf16)
    w: torch.Tensor                   # [Co,taps,Ci] fp32 (OHWI memory)
    bias: Optional[torch.Tensor]      # [N]
    scale: Optional[torch.Tensor]     # [B,Cs]
    shift: Optional[torch.Tensor]


def _rows_operands(c: Rows) -> RowsOps:
    g = torch.Generator().manual_seed(_seed(c.id))
    B, H, W = c.shape
    taps = taps_of(c.kind)
    if c.form == "fwd":
        src = torch.randn((B, H, W, c.Cs), generator=g)
        src[..., c.Ci:] = FAR    # the kernels must read only s < K
    else:
        src = torch.randn((B, *out_hw(c.kind, H, W), c.Co), generator=g)
    if c.a16:
        src = src.bfloat16()
    w = torch.randn((c.Co, taps, c.Ci), generator=g) * 0.2
    N = rows_dims(c)[1]
    bias = torch.randn((N,), generator=g) * 0.5 if c.bias else None
    scale = shift = None
    if c.xf != XF_NONE:
        scale, shift = torch.rand((B, c.Cs), generator=g) + 0.5, torch.randn((B, c.Cs), generator=g) * 0.5
    return RowsOps(src, w, bias, scale, shift)


_CACHE = {}


def _cached(key, make, small=True):
    if not small:
        return make()
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def rows_operands(c: Rows) -> RowsOps:
    """seeded, computed once per case and shared (never modified)"""
    return _cached(("rows-ops", c.id), lambda: _rows_operands(c))


ROWS_MUTANTS = ("tap", "unused", "lastblock", "pad")


def rows_value(c: Rows, acc=torch.float64, xfdt=torch.float64, mut: Optional[str] = None) -> torch.Tensor:
    """the launch's result [M, N] before storage rounding, as float64.  acc: dtype of products and sums; xfdt: of the transform.
    mut: ONE mistake -- tap (a tap shifted by one pixel), unused (the channel after the contraction's last is read),
    lastblock (the last 128-channel block left zero), pad (padding transformed instead of kept zero)"""
    o = rows_operands(c)
    mp = matrix_pipe(c.kernel)
    rnd = (lambda t: br.r16(t)) if mp else (lambda t: t)
    w = o.w
    if c.form == "fwd":
        a = o.src.to(xfdt)
        K = c.Ci
        if mut == "unused":
            assert c.Cs > c.Ci
            K, w = c.Ci + 1, torch.cat([w, w[..., :1]], dim=-1)
        if mut == "pad":   # zero padding first, then the transform over it (the border takes the image's shift)
            assert c.xf != XF_NONE and c.kind == "c3"
            a = _transform(F.pad(a, (0, 0, 1, 1, 1, 1)), o.scale, o.shift, c.xf)
        else:
            a = _transform(a, o.scale, o.shift, c.xf)
        a = rnd(a[..., :K]).to(acc)
        if mut == "tap":
            a = torch.roll(a, 1, dims=2)
        wk = _oihw(rnd(w).to(acc), c.kind)
        y = F.conv2d(_nchw(a), wk) if mut == "pad" else br.conv_nchw(_nchw(a), wk, c.kind)
        y = _nhwc(y)
    else:
        assert mut in (None, "tap", "lastblock")
        B, H, W = c.shape
        d = rnd(o.src.to(xfdt)).to(acc)
        if mut == "tap":
            d = torch.roll(d, 1, dims=2)
        x0 = torch.zeros(B, c.Ci, H, W, dtype=acc, requires_grad=True)
        (gx,) = torch.autograd.grad(br.conv_nchw(x0, _oihw(rnd(w).to(acc), c.kind), c.kind), x0, _nchw(d))
        y = _nhwc(gx)
    if o.bias is not None:
        y = y + o.bias.to(acc)
    y = y.double().reshape(-1, y.shape[-1]).contiguous()
    if mut == "lastblock":
        y[:, 128 * ((y.shape[1] - 1) // 128):] = 0.0
    return y


def rows_ref(c: Rows) -> torch.Tensor:
    return _cached(("rows-ref", c.id), lambda: rows_value(c), small=c.id != THIN_LARGE.id)


def rows_store(c: Rows, v: torch.Tensor) -> torch.Tensor:
    """v as the kernel stores it"""
    return br.r16(v) if c.out16 else v.to(torch.float32)


def rows_bias_early(c: Rows, acc=torch.float64) -> torch.Tensor:
    """the wrong bf16 store: the sum rounded, the bias added, rounded again"""
    o = rows_operands(c)
    assert c.out16 and o.bias is not None
    v = rows_value(c, acc) - o.bias.double()
    return br.r16(br.r16(v).double() + o.bias.double())


def rows_bar(c: Rows):
    """-> (bar, fp32_cpu or None)"""
    if matrix_pipe(c.kernel) and c.xf != XF_NONE:
        fp32_cpu = _cached(("rows-fp32", c.id), lambda: sr.rel(rows_value(c, xfdt=torch.float32), rows_ref(c)))
        return sr.bar(4, fp32_cpu, br.BAR_DIRECT), fp32_cpu
    return br.BAR_DIRECT, None


def stage(name, v, got, bf16: bool, bar: float) -> br.Stage:
    return br.Stage(name, "thin_edges", v.double(), got, "bf16" if bf16 else "f32", bar, None)


def figure(s: br.Stage) -> float:
    """the figure recorded next to s.bar, on its scale (of max |v|), such that figure <= bar is exactly bf16_refs.ratio(s) <= 1:
    max |got - v| / max |v| for an fp32 result, the same after each element's ulp / 2 is taken off for a bf16 one"""
    r = br.ratio(s)
    return r * s.bar if s.kind == "f32" else (br.bar_used(s) * s.bar if r != float("inf") else r)


def _allowed(v: torch.Tensor, bf16: bool, bar: float) -> torch.Tensor:
    al = torch.full_like(v, bar * float(v.abs().max()))
    return al + 0.5 * br.ulp_bf16(v) if bf16 else al


def track_ref(c: Rows, v: torch.Tensor, bar: float, ragged_included: bool = False):
    """the tracker partials [tile][n]: sums over the tile's valid rows of |v as stored|, and what they may be off by: the
    output criterion's allowance of every such element plus 128 * 2^-24 * sum |v| for the fp32 sum.
    ragged_included: the wrong sums that count the rows past M (the kernel computes bias + 0 there)"""
    M, N = v.shape
    nt = (M + TP - 1) // TP
    stored = rows_store(c, v).double().abs()
    al = _allowed(v, c.out16, bar)
    if ragged_included:
        b = rows_operands(c).bias
        fill = rows_store(c, b.double()[None, :]).double().abs().expand(nt * TP - M, N)
    else:
        fill = torch.zeros(nt * TP - M, N, dtype=torch.float64)
    tiles = lambda t, f: torch.cat([t, f]).reshape(nt, TP, N).sum(dim=1)   # noqa: E731
    ref = tiles(stored, fill)
    allow = tiles(al, torch.zeros_like(fill)) + TP * U * tiles(v.abs(), torch.zeros_like(fill))
    return ref, allow


def track_ratio(got: torch.Tensor, ref: torch.Tensor, allow: torch.Tensor) -> float:
    e = (got.double().reshape(ref.shape) - ref).abs() / allow
    return float("inf") if not bool(torch.isfinite(e).all()) else float(e.max())


# ---------------------------------------------------------------------------------------------------- weight gradient: cases
class Wg(NamedTuple):
    id: str
    kernel: str
    side: int              # 1: the narrow side is X (Ci <= 4), 2: it is dY (Co <= 4)
    kind: str
    shape: tuple           # B, H, W of the forward input map
    Cs: int
    Co: int
    Ci: int
    ns: int                # nsplit, set by hand
    xf: int = XF_NONE
    bias: bool = True
    bf16: bool = False
    wide16: bool = False   # the wide side stored as bf16 (side 1: y_bf16, side 2: x_bf16)
    no_thin: bool = False


MAP_A = (3, 16, 32)        # 12 tiles, 4 per image


def _wg(tag, side, narrow, cs_or_none, wide, ns, xf=0, bias=True, thin=False, shape=MAP_A, kind="c3", wide16=None, no_thin=False, bf16=None):
    tf = "true" if side == 1 else "false"
    kernel = f"wgrad_thin_bf16_kernel<{tf},{xf}>" if thin else f"wgrad_smallk_kernel<{tf},{xf}>"
    if side == 1:
        Cs, Co, Ci = cs_or_none, wide, narrow
    else:
        Cs, Co, Ci = wide, narrow, wide
    w16 = thin if wide16 is None else wide16
    return Wg(f"{'thin' if thin else 'smallk'}-{tag}-ns{ns}", kernel, side, kind, shape, Cs, Co, Ci, ns, xf, bias,
              thin if bf16 is None else bf16, w16, no_thin)


def _both(*a, **k):
    return (_wg(*a, **k), _wg(*a, thin=True, **k))


WG_CASES = (
    # map A, kind 1 (narrow X): nsplit 1 (per = 12, across two image boundaries), 5 (per = 3, the last split empty), 12 (planned)
    *_both("k1-3of4-m128", 1, 3, 4, 128, 1), *_both("k1-3of4-m128", 1, 3, 4, 128, 5), *_both("k1-3of4-m128", 1, 3, 4, 128, 12),
    *_both("k1-3of4-m128-nobias", 1, 3, 4, 128, 5, bias=False),
    *_both("k1-4of4-m256", 1, 4, 4, 256, 5), *_both("k1-1of1-m128", 1, 1, 1, 128, 1, bias=False),
    # map A, kind 2 (narrow dY): XF 0, 1, 2; XF 1 and 2 with nsplit 1 reload the scale row across images
    *(c for xf in (0, 1, 2) for ns in (1, 5, 12) for c in _both(f"k2-m3-n128-xf{xf}", 2, 3, None, 128, ns, xf=xf)),
    *_both("k2-m1-n128-xf0", 2, 1, None, 128, 12), *_both("k2-m4-n256-xf2", 2, 4, None, 256, 5, xf=2), *_both("k2-m4-n256-xf1", 2, 4, None, 256, 1, xf=1),
    # VALU kernel only, map B: a ragged last tile, image boundaries inside tiles, a channel-block tail, xb changing mid-tile
    *(_wg("mapB-k1-3of4-m160", 1, 3, 4, 160, ns, shape=MAP_B) for ns in (1, 2, 3)),
    *(_wg("mapB-k2-m3-n128-xf2", 2, 3, None, 128, ns, xf=2, shape=MAP_B) for ns in (1, 2, 3)),
    # kind 1 on the other geometries wgrad_smallk_kind admits
    _wg("c3s2-k1-3of4-m128", 1, 3, 4, 128, 1, shape=(1, 10, 14), kind="c3s2"),
    _wg("c3up-k1-4of4-m128", 1, 4, 4, 128, 2, shape=(1, 5, 6), kind="c3up"),      # 1 tile in 2 splits: the second empty
    _wg("c1-k1-4of4-m128", 1, 4, 4, 128, 1, shape=(2, 5, 7), kind="c1"),
    # the wide side stored as bf16 on the VALU kernel
    _wg("wide16-k1-3of4-m128", 1, 3, 4, 128, 5, wide16=True, no_thin=True, bf16=True),
    _wg("wide16-k2-m3-n128-xf2", 2, 3, None, 128, 5, xf=2, wide16=True, no_thin=True, bf16=True),
)


def wg_case(cid: str) -> Wg:
    return {c.id: c for c in WG_CASES}[cid]


def wg_pixels(c: Wg) -> int:
    """pixels of the grid the kernel walks (side 1: dY's, side 2: X's): the contraction length"""
    B, H, W = c.shape
    Hy, Wy = out_hw(c.kind, H, W)
    return B * Hy * Wy if c.side == 1 else B * H * W


def wg_tiles(c: Wg) -> int:
    return (wg_pixels(c) + TP - 1) // TP


def wg_ranges(c: Wg):
    """[(first tile, end tile)] of every split, as the kernels deal them: per = ceil(tiles / nsplit)"""
    nt = wg_tiles(c)
    per = (nt + c.ns - 1) // c.ns
    return [(min(nt, s * per), min(nt, s * per + per)) for s in range(c.ns)]


def wg_block(c: Wg, ops):
    B, H, W = c.shape
    a = ops.wgrad_args(c.kind, B, H, W, c.Cs, c.Co, c.Ci, xf=c.xf, prec=ops.PREC_BF16 if c.bf16 else ops.PREC_F32)
    a.dY, a.X = _placeholder(), _placeholder()
    a.nsplit = c.ns
    if c.ns == 1:
        a.out = _placeholder()
    else:
        a.partial = _placeholder()
    if c.bias:
        a.bias_partial = _placeholder()
    if c.xf != XF_NONE:
        a.scale, a.shift = _placeholder(), _placeholder()
    if c.wide16:
        if c.side == 1:
            a.y_bf16 = 1
        else:
            a.x_bf16 = 1
    return a


# ---------------------------------------------------------------------------------------------------- weight gradient: values
class WgOps(NamedTuple):
    x: torch.Tensor        # [B,H,W,Cs] as stored
    dy: torch.Tensor       # [B,Ho,Wo,Co] as stored
    scale: torch.Tensor    # [B,Cs]
    shift: torch.Tensor


def _wg_operands(c: Wg) -> WgOps:
    g = torch.Generator().manual_seed(_seed(c.id.rsplit("-ns", 1)[0]))   # (the same operands under every split count)
    B, H, W = c.shape
    x = torch.randn((B, H, W, c.Cs), generator=g)
    x[..., c.Ci:] = FAR
    dy = torch.randn((B, *out_hw(c.kind, H, W), c.Co), generator=g)
    scale, shift = torch.rand((B, c.Cs), generator=g) + 0.5, torch.randn((B, c.Cs), generator=g) * 0.5
    if c.wide16:
        if c.side == 1:
            dy = dy.bfloat16()
        else:
            x = x.bfloat16()
    return WgOps(x, dy, scale, shift)


def wg_operands(c: Wg) -> WgOps:
    return _cached(("wg-ops", c.id), lambda: _wg_operands(c))


class WgVal(NamedTuple):
    gw: torch.Tensor       # [Co,taps,Ci] float64
    gb: torch.Tensor       # [Co]
    gb_abs: torch.Tensor   # sum |dy| per channel over what gb sums


def wg_value(c: Wg, acc=torch.float64, xfdt=torch.float64, pw: Optional[torch.Tensor] = None, bidx: Optional[torch.Tensor] = None) -> WgVal:
    """dW and db.  pw [pixels of the walked grid]: how often each pixel is counted (None: once; 0: dropped; 2: twice) -- a
    dropped or doubled tile is 128 consecutive entries.  bidx [B,H,W]: the image whose scale / shift row each pixel is given"""
    o = wg_operands(c)
    mp = matrix_pipe(c.kernel)
    rnd = (lambda t: br.r16(t)) if mp else (lambda t: t)
    a = rnd(_transform(o.x.to(xfdt), o.scale, o.shift, c.xf, bidx)[..., :c.Ci]).to(acc)
    d = rnd(o.dy.to(xfdt)).to(acc)
    # the bias gradient: kind 1 sums dY as the kernel is given it (the thin kernel: the bf16 tensor), kind 2 the fp32 dY before
    # any rounding (the centre tap of the gather)
    dsum = o.dy.double()
    if pw is not None:
        p = pw.to(torch.float64)
        if c.side == 1:
            d, dsum = d * p.to(acc).reshape(*d.shape[:3], 1), dsum * p.reshape(*d.shape[:3], 1)
        else:
            a, dsum = a * p.to(acc).reshape(*a.shape[:3], 1), dsum * p.reshape(*d.shape[:3], 1)
    k = 1 if c.kind == "c1" else 3
    w0 = torch.zeros(c.Co, c.Ci, k, k, dtype=acc, requires_grad=True)
    (gw,) = torch.autograd.grad(br.conv_nchw(_nchw(a), w0, c.kind), w0, _nchw(d))
    gw = gw.permute(0, 2, 3, 1).reshape(c.Co, k * k, c.Ci).double()
    return WgVal(gw, dsum.sum(dim=(0, 1, 2)), dsum.abs().sum(dim=(0, 1, 2)))


def wg_ref(c: Wg) -> WgVal:
    return _cached(("wg-ref", c.id.rsplit("-ns", 1)[0]), lambda: wg_value(c))


def wg_bar(c: Wg):
    """-> (bar, fp32_cpu or None)"""
    floor = br.BAR_WGRAD_GN if c.xf != XF_NONE else br.BAR_WGRAD
    if matrix_pipe(c.kernel) and c.xf != XF_NONE:
        fp32_cpu = _cached(("wg-fp32", c.id.rsplit("-ns", 1)[0]), lambda: sr.rel(wg_value(c, xfdt=torch.float32).gw, wg_ref(c).gw))
        return sr.bar(4, fp32_cpu, floor), fp32_cpu
    return floor, None


def db_ratio(c: Wg, db: torch.Tensor, ref: WgVal) -> float:
    """worst |db - ref| / (n * 2^-24 * sum |dy|), n = B*H*W of the walked grid"""
    e = (db.double().reshape(-1) - ref.gb).abs() / (wg_pixels(c) * U * ref.gb_abs)
    return float("inf") if not bool(torch.isfinite(e).all()) else float(e.max())


def own_image(c: Wg) -> torch.Tensor:
    """[B,H,W] int64: every pixel's own image"""
    B, H, W = c.shape
    return torch.arange(B)[:, None, None].expand(B, H, W).contiguous()


# ---------------------------------------------------------------------------------------------------- figures
# {what: (figure, its bar, fp32_cpu or None)} of one launch's results; a launch passes when every figure is within its bar
def passes(figs) -> bool:
    return all(m <= lim for m, lim, _ in figs.values())


def rows_figures(c, out, track=None, v=None):
    v = rows_ref(c) if v is None else v
    bar, fp = rows_bar(c)
    figs = {"out": (figure(stage(c.id, v, out, c.out16, bar)), bar, fp)}
    if track is not None:
        ref, allow = track_ref(c, v, bar)
        figs["track"] = (track_ratio(track, ref, allow), 1.0, None)
    return figs


def wg_figures(c, gw, db=None):
    ref = wg_ref(c)
    bar, fp = wg_bar(c)
    figs = {"dW": (figure(stage(c.id, ref.gw, gw, False, bar)), bar, fp)}
    if db is not None:
        figs["db"] = (db_ratio(c, db, ref), 1.0, None)
    return figs
