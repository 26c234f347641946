"""Tensor-level wrappers over the C ABI.  Activations are NHWC fp32 CUDA tensors.

Every function enqueues on torch's current HIP stream and never synchronises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional, Tuple

import torch

from .lib import ConvGeom, IgemmArgs, WgradArgs, lib

XF_NONE, XF_AFFINE, XF_AFFINE_SILU = 0, 1, 2
PREC_F32, PREC_BF16 = 0, 1
# arithmetic of the conv contractions (set by the engine from training.mixed_precision); tensors stay fp32
PRECISION = PREC_F32

# bf16 image of a parameter arena (base address of the fp32 arena, its size in bytes, base address of the image):
# weights that live inside the arena are handed to the bf16 kernels as `Wh` (set by the engine per forward)
WEIGHTS16: Optional[Tuple[int, int, int]] = None


def pack_bf16(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst (bf16 storage, same numel) = round-to-nearest-even image of the fp32 tensor `src`."""
    assert src.is_contiguous() and dst.is_contiguous() and dst.numel() == src.numel() and dst.element_size() == 2
    lib.call("vae_pack_bf16", _p(src), src.numel(), _p(dst), _stream())
    return dst


def _wh(w: torch.Tensor):
    if PRECISION != PREC_BF16 or WEIGHTS16 is None:
        return None
    base, nbytes, base16 = WEIGHTS16
    off = w.data_ptr() - base
    return C.c_void_p(base16 + off // 2) if 0 <= off < nbytes else None


class precision:
    """context manager: arithmetic of the conv contractions inside the block (PREC_F32 | PREC_BF16)"""

    def __init__(self, prec: int):
        self.prec = prec

    def __enter__(self):
        global PRECISION
        self.prev, PRECISION = PRECISION, self.prec

    def __exit__(self, *exc):
        global PRECISION
        PRECISION = self.prev
        return False


class option:
    """context manager over the library's process-wide kernel-selection switches (vae_set_option: "flat_conv", "no_wino",
    "no_wino4", "no_wide", "no_thin_mfma", "no_wgrad_dma", and the count "wide_reserved_cus"); the environment (VAEHIP_FLAT_CONV / VAEHIP_NO_WINO / ...) only
    gives their initial values"""

    def __init__(self, name: str, value: int = 1):
        self.name, self.value = name.encode(), int(value)

    def __enter__(self):
        self.prev = lib.query("vae_get_option", self.name)
        lib.call("vae_set_option", self.name, self.value)

    def __exit__(self, *exc):
        lib.call("vae_set_option", self.name, self.prev)
        return False


def get_option(name: str) -> int:
    return int(lib.query("vae_get_option", name.encode()))


MODE_FWD, MODE_UP2X, MODE_DGRAD, MODE_DGRAD_S2, MODE_UP2X_DGRAD = 0, 1, 2, 3, 4
GN_GROUPS = 32
GN_EPS = 1e-6


class LaunchProfiler:
    """optional HIP-event timing per kernel instantiation (bench.py's live roofline figures; events go on the launch
    stream).  A record carries two FLOP counts: `flops` = the ALGORITHMIC work of the reference formulation (direct
    convolution: 9 taps, also for an upsampler's phase launches) and `executed` = the multiply-adds the kernel really
    issues on the matrix pipe (16/36 of that for the Winograd kernels, the taps of its mask for a phase convolution).
    HBM-bound helpers (reductions) are recorded with zero FLOPs."""

    def __init__(self):
        self.records = []  # (key, flops, executed, start_event, end_event)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for key, flops, executed, e0, e1 in self.records:
            d = out.setdefault(key, {"launches": 0, "flops": 0.0, "executed": 0.0, "ms": 0.0})
            d["launches"] += 1
            d["flops"] += flops
            d["executed"] += executed
            d["ms"] += e0.elapsed_time(e1)
        return out


PROFILER: Optional[LaunchProfiler] = None
WINO_EXECUTED = 16.0 / 36.0  # F(2x2,3x3) / F(3x3,2x2): 16 multiplications per 36 direct multiply-adds
WINO4_EXECUTED = 36.0 / 144.0  # F(4x4,3x3): 36 per 144


def _kernel_name(fn: str, a) -> str:
    buf = C.create_string_buffer(128)
    lib.call(fn, C.byref(a), buf, 128)
    return buf.value.decode()


def _timed(key, flops: float, executed: float, fn: str, *args):
    """lib.call(fn, *args), bracketed by two events on the launch stream when a profiler is installed; `key` may be a
    callable (evaluated only when profiling)"""
    if PROFILER is None:
        lib.call(fn, *args)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    lib.call(fn, *args)
    e1.record()
    PROFILER.records.append((key() if callable(key) else key, flops, executed, e0, e1))


def _launch_igemm(a: IgemmArgs):
    if PROFILER is None:
        lib.call("vae_igemm_rows", C.byref(a), _stream())
        return
    # executed taps per row: the parity-class stride-2 dgrad meets 9/4 taps per row on average (that IS the direct
    # convolution's count), a phase convolution of an upsampler only those of its tap mask (algorithmic: all 9 at high resolution)
    taps = 2.25 if a.g.mode == MODE_DGRAD_S2 else a.g.taps
    ex_taps = bin(a.tapmask).count("1") if a.tapmask else taps
    name = _kernel_name("vae_igemm_kernel_name", a)
    base = 2.0 * a.M * a.N * a.K * a.batch
    if "upwino" in name:  # conv3x3 over the virtual 2x upsample: 36 multiply-adds per low-resolution pixel and channel pair, 9 executed
        lowres = a.M / 4.0 if a.g.mode == MODE_UP2X else float(a.M)
        _timed(name, 2.0 * lowres * a.N * a.K * 36, 2.0 * lowres * a.N * a.K * 9, "vae_igemm_rows", C.byref(a), _stream())
        return
    frac = WINO4_EXECUTED if "wino4" in name else (WINO_EXECUTED if "wino" in name else 1.0)
    _timed(name, base * taps, base * ex_taps * frac, "vae_igemm_rows", C.byref(a), _stream())


def _launch_wgrad(a: WgradArgs):
    if PROFILER is None:
        lib.call("vae_wgrad", C.byref(a), _stream())
        return
    ex_taps = bin(a.tapmask).count("1") if a.tapmask else a.g.taps
    base = 2.0 * a.M * a.N * a.npix * a.batch
    _timed(_kernel_name("vae_wgrad_kernel_name", a), base * a.g.taps, base * ex_taps, "vae_wgrad", C.byref(a), _stream())


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _b16(t: Optional[torch.Tensor]) -> int:
    """1 when the tensor is stored as bf16 (the *_bf16 flags of the C ABI)"""
    return 1 if (t is not None and t.dtype == torch.bfloat16) else 0


def _chk(t: torch.Tensor, name: str):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise ValueError(f"{name}: expected a float32 CUDA tensor, got {t.dtype} on {t.device}")


def _chk_c(t: torch.Tensor, name: str):
    _chk(t, name)
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous NHWC tensor, strides {t.stride()}")


def ohwi(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d weight (logical OIHW, channels_last memory) -> [O,KH,KW,I] contiguous view; nn.Linear -> [O,1,1,I]."""
    if w.ndim == 2:
        v = w.view(w.shape[0], 1, 1, w.shape[1])
    else:
        v = w.permute(0, 2, 3, 1)
    if not v.is_contiguous():
        raise ValueError("weight memory is not OHWI (channels_last); parameters must live in the VAE arena")
    return v


class Stats(NamedTuple):
    mean: torch.Tensor   # [B, G]
    rstd: torch.Tensor   # [B, G]
    scale: torch.Tensor  # [B, C]
    shift: torch.Tensor  # [B, C]


# ------------------------------------------------------------------ launch descriptions
# Every launch's argument block from integers alone (no tensor, no allocation, no library call); the entry points add the
# pointers, views, storage flags and epilogue fields.  tests/golden/make_dispatch_table.py and the tests build their blocks
# here too.  H, W: the layer's forward INPUT map; Cs: channels of its storage (>= Ci); prec: None = PRECISION.
def out_hw(kind: str, H: int, W: int) -> Tuple[int, int]:
    if kind in ("c3", "c1"):
        return H, W
    if kind == "c3s2":  # padding (0, 1, 0, 1)
        return (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1
    if kind == "c3up":
        return 2 * H, 2 * W
    raise ValueError(kind)


_KIND = {"c3": (9, 1, 1, MODE_FWD), "c1": (1, 1, 0, MODE_FWD), "c3s2": (9, 2, 0, MODE_FWD), "c3up": (9, 1, 1, MODE_UP2X)}  # taps, stride, pad, forward mode


def _fwd_geom(kind: str, B: int, H: int, W: int, Cs: int) -> ConvGeom:
    taps, stride, pad, mode = _KIND[kind]
    return ConvGeom(B, H, W, Cs, *out_hw(kind, H, W), taps, stride, pad, pad, mode)


def _rows_args(g: ConvGeom, Co: int, Ci: int, dgrad: bool, prec: Optional[int], xf: int = XF_NONE) -> IgemmArgs:
    """rows form over the row grid of `g`: forward (N = Co, contraction over Ci, OHWI weights read k-contiguous) or dgrad
    (N = Ci, contraction over Co, the same weights read n-contiguous)"""
    a = IgemmArgs(g=g)
    a.M = g.B * g.Ho * g.Wo
    if dgrad:
        a.N, a.K, a.ldc = Ci, Co, Ci
        a.sn, a.sk = 1, g.taps * Ci
    else:
        a.N, a.K, a.ldc = Co, Ci, Co
        a.sn, a.sk = g.taps * Ci, 1
    a.st, a.batch = Ci, 1
    a.xf, a.alpha, a.prec = xf, 1.0, PRECISION if prec is None else prec
    return a


def _wgrad_form(g: ConvGeom, Co: int, Ci: int, prec: Optional[int], xf: int = XF_NONE) -> WgradArgs:
    """wgrad form: [Co, taps, Ci] = dY^T @ patches(X) over the pixels of `g`, one split until a plan says otherwise"""
    a = WgradArgs(g=g)
    a.M, a.N, a.ldy, a.npix, a.nsplit, a.batch = Co, Ci, Co, g.B * g.Ho * g.Wo, 1, 1
    a.xf, a.alpha, a.prec = xf, 1.0, PRECISION if prec is None else prec
    return a


def fwd_args(kind: str, B: int, H: int, W: int, Cs: int, Co: int, Ci: int, *, xf: int = XF_NONE, prec: Optional[int] = None) -> IgemmArgs:
    """forward of a layer (c3up: MODE_UP2X, the virtual-upsample kernel and the upsampler-Winograd forward alike)"""
    return _rows_args(_fwd_geom(kind, B, H, W, Cs), Co, Ci, False, prec, xf)


def dgrad_args(kind: str, B: int, H: int, W: int, Co: int, Ci: int, *, s2: bool = True, prec: Optional[int] = None) -> IgemmArgs:
    """dgrad of a layer: dy [B,Ho,Wo,Co] -> rows over the input map (c3up: the virtual-upsample form over 2H x 2W, which the
    caller sums 2x2).  A stride-2 layer gets the parity-class form where its map allows (s2 = False: the plain form)."""
    Hy, Wy = out_hw(kind, H, W)
    Hr, Wr = (Hy, Wy) if kind == "c3up" else (H, W)
    taps, stride, pad, _ = _KIND[kind]
    mode = MODE_DGRAD
    if s2 and kind == "c3s2" and H % 2 == 0 and W % 2 == 0 and (B * H * W // 4) % 128 == 0:
        mode = MODE_DGRAD_S2  # parity-class-major rows: only the taps a class meets are computed (9/4 instead of 9)
    return _rows_args(ConvGeom(B, Hy, Wy, Co, Hr, Wr, taps, stride, pad, pad, mode), Co, Ci, True, prec)


def up2x_dgrad_args(B: int, H: int, W: int, Co: int, Ci: int, *, prec: Optional[int] = None) -> IgemmArgs:
    """dgrad of an upsampler in one pass (MODE_UP2X_DGRAD): dy [B,2H,2W,Co] -> rows over the low-resolution map"""
    return _rows_args(ConvGeom(B, 2 * H, 2 * W, Co, H, W, 9, 1, 1, 1, MODE_UP2X_DGRAD), Co, Ci, True, prec)


def phase_args(B: int, H: int, W: int, Co: int, Ci: int, dgrad: bool, *, prec: Optional[int] = None) -> IgemmArgs:
    """one phase convolution of an upsampler on its low-resolution map, forward or dgrad: the high-resolution side is read
    (dgrad) or written (forward) at every second pixel; tap mask of phase (0, 0), which the caller replaces per phase"""
    a = _rows_args(ConvGeom(B, H, W, Co if dgrad else Ci, H, W, 9, 1, 1, 1, MODE_DGRAD if dgrad else MODE_FWD), Co, Ci, dgrad, prec)
    a.a_step, a.c_step = (2, 0) if dgrad else (0, 2)  # (0 = a plain view)
    a.tapmask = _phase_tapmask(0, 0)
    return a


def wgrad_args(kind: str, B: int, H: int, W: int, Cs: int, Co: int, Ci: int, *, xf: int = XF_NONE, prec: Optional[int] = None) -> WgradArgs:
    """weight gradient of a layer, over its forward geometry"""
    return _wgrad_form(_fwd_geom(kind, B, H, W, Cs), Co, Ci, prec, xf)


def wgrad_phase_args(B: int, H: int, W: int, Co: int, Ci: int, *, prec: Optional[int] = None) -> WgradArgs:
    """weight gradient of one phase of an upsampler (dy read at every second pixel; tap mask of phase (0, 0))"""
    a = _wgrad_form(ConvGeom(B, H, W, Ci, H, W, 9, 1, 1, 1, MODE_FWD), Co, Ci, prec)
    a.y_step, a.tapmask = 2, _phase_tapmask(0, 0)
    return a


def gemm_rows_args(M: int, N: int, K: int, bkm: bool, alpha: float, z: int, *, prec: Optional[int] = None) -> IgemmArgs:
    """z dense GEMMs out = alpha * A @ Bm^T (A [M,K], Bm [N,K]), or A @ Bm (bkm: Bm [K,N]): a one-tap convolution over M pixels
    in a row, forward or dgrad form.  (In bf16 mode scores / context / their gradients run on the bf16 MFMA too)"""
    a = _rows_args(ConvGeom(1, 1, M, K, 1, M, 1, 1, 0, 0, MODE_FWD), K if bkm else N, N if bkm else K, bkm, prec)
    a.st, a.alpha, a.batch, a.sAb, a.sWb, a.sCb = 0, alpha, z, M * K, N * K, M * N
    return a


def gemm_tn_args(M: int, N: int, K: int, alpha: float, z: int, *, prec: Optional[int] = None) -> WgradArgs:
    """z dense GEMMs out = alpha * A^T @ Bm (A [K,M], Bm [K,N]): a one-tap weight gradient over K pixels in a row"""
    a = _wgrad_form(ConvGeom(1, 1, K, N, 1, K, 1, 1, 0, 0, MODE_FWD), M, N, prec)
    a.alpha, a.batch, a.sYb, a.sXb, a.sOb = alpha, z, K * M, K * N, M * N
    return a


# The conv entry points decide (every library query), then allocate, then launch, so a query may concern an output, or a bf16
# image, that does not exist yet.  This placeholder stands for such a tensor: one this module will allocate itself.  The
# library's answers depend on a pointer only through null / non-null and its 16-byte alignment, and the module's own
# allocations are at least 256-byte aligned (torch's device allocator; tests/guarded.py ALIGN).  It is never dereferenced,
# and every site replaces it by the real pointer before it launches.
_UNALLOCATED = C.c_void_p(256)


def _reduce_splits(partial, bpart, ns: int, n: int, Co: int, wout, bout):
    """fixed-order sums over the ns splits of a weight gradient: the slab partial [ns, n] into wout (None: one split, the kernel
    wrote wout itself) and the bias slab bpart [ns, Co] (None: no bias gradient) into bout"""
    if partial is not None and bpart is not None:  # one launch for both reductions
        lib.call("vae_reduce_splits2", _p(partial), ns, n, _p(wout), _p(bpart), Co, _p(bout), _stream())
    elif partial is not None:
        lib.call("vae_reduce_splits", _p(partial), ns, n, _p(wout), _stream())
    elif bpart is not None:
        lib.call("vae_reduce_splits", _p(bpart), ns, Co, _p(bout), _stream())


# bf16 mode stores activations as bf16 (round 3): every conv output with at least ACT16_MIN_C channels, the residual stream
# and the gradients of both -- what autocast keeps for the reference (src/train.py:147-154).  GroupNorm statistics, tracker
# sums, the loss, the narrow tensors (image, latents, moments) and the parameters stay fp32.  False = fp32 storage with bf16
# images next to it (round 2's layout; kept for the kernel tests and as the A/B switch).
ACT_BF16 = True
ACT16_MIN_C = 32


def act16() -> bool:
    return PRECISION == PREC_BF16 and ACT_BF16 and WEIGHTS16 is not None


def to_f32(t: torch.Tensor) -> torch.Tensor:
    """fp32 copy of a bf16-stored tensor (the tensor itself when it is fp32)"""
    if t.dtype == torch.float32:
        return t
    out = torch.empty(t.shape, device=t.device, dtype=torch.float32)
    lib.call("vae_unpack_bf16", _p(t.contiguous()), t.numel(), _p(out), _stream())
    return out


def to_bf16(t: torch.Tensor) -> torch.Tensor:
    if t.dtype == torch.bfloat16:
        return t
    return pack_bf16(t.contiguous(), torch.empty(t.shape, device=t.device, dtype=torch.bfloat16))


def _like(t: torch.Tensor, want16: bool) -> torch.Tensor:
    return to_bf16(t) if want16 else to_f32(t)


def act_image_ok(kind: str, x_shape, Co: int, Ci: int) -> bool:
    """bf16 mode: may this layer's forward and wgrad read a bf16 image of the transformed input (gn_apply_bf16)?"""
    if PRECISION != PREC_BF16 or WEIGHTS16 is None or kind != "c3":
        return False
    return bool(lib.query("vae_bf16_act_image_ok", C.byref(_fwd_geom(kind, *x_shape)), Co, Ci))


# fp32 mode: a Winograd workgroup covers 64 output channels, so GroupNorm+SiLU fused into its halo staging is recomputed
# Cout/64 times per element (and once more per 128 channels in the wgrad).  Writing the transformed tensor once
# (vae_gn_apply: 8 B/element) and running forward + wgrad without a transform is cheaper (tools/microbench_wino.py, 512
# channels @64^2: fused forward 1.38 vs 1.20 ms, fused wgrad 1.43 vs 1.27, the extra pass 0.07 ms).  Measured on the whole step
# (bench.py, 256^2, batch 16): never 214.8 ms / 15.5 GiB peak, Cin >= 512: 209.6 / 17.7, >= 256: 207.2 / 20.7, >= 128 (all
# of them): 205.2 ms / 25.4 GiB.  VAEHIP_ACT32_MIN_CIN overrides (a large value = always fuse: the lowest peak memory).
ACT_IMAGE32_MIN_CIN = int(os.environ.get("VAEHIP_ACT32_MIN_CIN", "128"))


def act_image32_ok(kind: str, x_shape, Co: int, Ci: int) -> bool:
    if PRECISION != PREC_F32 or not WINOGRAD or kind != "c3" or Ci < ACT_IMAGE32_MIN_CIN or get_option("no_wino") or get_option("flat_conv"):
        return False
    B, H, W, Cs = x_shape
    return H % 8 == 0 and W % 16 == 0 and Ci % 32 == 0 and Co % 64 == 0 and Cs == Ci


def grad_image_ok(kind: str, x_shape, Co: int, Ci: int) -> bool:
    """bf16 mode: may the OUTPUT gradient of this layer (forward input x_shape) be handed to its dgrad and wgrad as a bf16 image?
    (bf16 mode with fp32 storage, ACT_BF16 = False, keeps gradients that only feed bf16 kernels as bf16 images: the dgrad
    outputs of the halo-tile kernels and the GroupNorm-backward outputs)"""
    if PRECISION != PREC_BF16 or WEIGHTS16 is None or kind != "c3":
        return False
    return bool(lib.query("vae_bf16_grad_image_ok", C.byref(_fwd_geom(kind, *x_shape)), int(Co), int(Ci)))


def _grad16(dy: torch.Tensor) -> Optional[torch.Tensor]:
    """the bf16 form of a gradient tensor: the tensor itself when it is stored as bf16, or the image its producer attached"""
    if dy.dtype == torch.bfloat16:
        return dy
    return getattr(dy, "_b16", None)


def gn_apply_bf16(x: torch.Tensor, st: "Stats", xf: int) -> torch.Tensor:
    """bf16(XF(x)) as a [B,H,W,C] bfloat16 tensor: the activation image conv_fwd(a16=) / conv_wgrad(x16=) read."""
    B, H, W, Cc = x.shape
    y = torch.empty((B, H, W, Cc), device=x.device, dtype=torch.bfloat16)
    lib.call("vae_gn_apply_bf16", _p(x), _b16(x), _p(st.scale), _p(st.shift), B, H * W, Cc, xf, _p(y), _stream())
    return y


# fp32 mode: forward and dgrad of the plain 3x3 stride-1 layers as Winograd F(2x2,3x3) (16 instead of 36 multiplications per
# 2x2 outputs; csrc/conv3_wino.hip).  False = the direct halo-tile kernels (also what the library option "no_wino" selects)
WINOGRAD = True


def _wino_ok(a: IgemmArgs) -> bool:
    """does a Winograd kernel serve the launch `a` describes?"""
    return WINOGRAD and PRECISION == PREC_F32 and bool(lib.query("vae_wino_ok", C.byref(a)))


def _wino_weights(a: IgemmArgs, dev):
    """transformed weights for a launch _wino_ok accepted (a.Wu is set)"""
    nbytes = int(lib.query("vae_wino_weight_bytes", C.byref(a)))  # fp32 values or bf16 planes: the serving kernel's image
    wu = torch.empty(((nbytes + 3) // 4,), device=dev, dtype=torch.float32)
    lib.call("vae_wino_weights", C.byref(a), _p(wu), _stream())
    a.Wu = _p(wu)
    return wu


# conv3x3(nearest_upsample_2x(x)) as four phase convolutions on the low-resolution x (2x2 effective kernels: 16 instead
# of 36 tap-MACs per low-resolution pixel, forward and dgrad); False = the virtual-upsample kernel
PHASE_UPCONV = True
_PHASE_MASK = {0: (0, 1), 1: (1, 2)}  # parity -> rows (columns) of the 3x3 window on the low-resolution grid


def _phase_tapmask(pa: int, pb: int) -> int:
    return sum(1 << (kh * 3 + kw) for kh in _PHASE_MASK[pa] for kw in _PHASE_MASK[pb])


def upconv_phase_weights(wv: torch.Tensor) -> torch.Tensor:
    """wv: OHWI memory [Co,3,3,Ci] -> [4,Co,3,3,Ci] effective kernels per output parity (vae_upconv_phase_weights)."""
    Co, kh, kw, Ci = wv.shape
    we = torch.empty((4, Co, 3, 3, Ci), device=wv.device, dtype=torch.float32)
    lib.call("vae_upconv_phase_weights", _p(wv), Co, Ci, _p(we), _stream())
    return we


def _phase_weights(wv):
    """effective kernels of the four phases, and their bf16 image in bf16 mode"""
    we = upconv_phase_weights(wv)
    we16 = pack_bf16(we, torch.empty(we.shape, device=we.device, dtype=torch.bfloat16)) if PRECISION == PREC_BF16 else None
    return we, we16


def _phases(wv: Optional[torch.Tensor] = None):
    """the four phases of an upsampler in launch order -> (index, tap mask, row offset, column offset, W, Wh): W / Wh are the
    phase's effective kernel and its bf16 image, made here from the layer's OHWI weights `wv` (None: the weight gradient)"""
    we, we16 = _phase_weights(wv) if wv is not None else (None, None)
    for ph, (pa, pb) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yield ph, _phase_tapmask(pa, pb), pa, pb, None if we is None else _p(we[ph]), None if we16 is None else _p(we16[ph])


def _upconv_wino(a: IgemmArgs, src, wv, bias):
    """fp32: the upsampler launch `a` over `src` on csrc/conv3_upwino.hip (9 multiplications per low-resolution pixel and
    channel pair) -> the tensor of its row grid, or None when the kernel does not serve the layer"""
    a.A, a.W, a.C, a.bias = _p(src), _p(wv), _UNALLOCATED, _p(bias)
    if not _wino_ok(a):
        return None
    out = torch.empty((a.g.B, a.g.Ho, a.g.Wo, a.N), device=src.device, dtype=torch.float32)
    a.C = _p(out)
    wu = _wino_weights(a, src.device)  # (kept alive until the launch is enqueued; the allocator orders its reuse on the stream)
    _launch_igemm(a)
    return out


def _upconv_wino_fwd(x, wv, bias):
    """fp32: conv3x3(nearest_upsample_2x(x)) -> [B,2H,2W,Co], or None"""
    if not WINOGRAD or PRECISION != PREC_F32 or x.dtype != torch.float32:
        return None
    Co, _, _, Ci = wv.shape
    return _upconv_wino(fwd_args("c3up", *x.shape, Co, Ci), x, wv, bias)


def _upconv_wino_dgrad(dy, wv, in_hw):
    """fp32: dy [B,2H,2W,Co] -> gradient wrt the low-resolution input [B,H,W,Ci] (3x3 dgrad + 2x2 sum-pool in one pass), or None"""
    if not WINOGRAD or PRECISION != PREC_F32 or dy is None or dy.dtype != torch.float32:
        return None
    Co, _, _, Ci = wv.shape
    return _upconv_wino(up2x_dgrad_args(dy.shape[0], *in_hw, Co, Ci), dy, wv, None)


def _upconv_phase_fwd(x, wv, bias, want16: bool):
    """-> [B,2H,2W,Co] (bf16 when want16 and the kernel can write it) or None when the halo-tile kernels do not serve the
    low-resolution geometry.  x: fp32, or bf16 (then it IS the operand image)."""
    B, H, W, Cs = x.shape
    Co, _, _, Ci = wv.shape
    if Cs != Ci:
        return None
    a = phase_args(B, H, W, Co, Ci, False)
    a.A, a.W, a.Wh, a.bias = _p(x), _p(wv), _wh(wv), _p(bias)  # (W / Wh: the layer's own stand for the phase kernels in the queries)
    xb = x.dtype == torch.bfloat16
    use16 = False
    if PRECISION == PREC_BF16 and a.Wh is not None and Cs % 8 == 0:
        # bf16 image of the low-resolution input (a resnet output, no GroupNorm in front): the wide-tile kernel takes the four
        # phase convolutions as 2x2 tap blocks.  The image is a bf16 x itself, else a copy made below (a misaligned fp32 x is
        # refused through A: the bf16 halo-tile kernels take 16-byte aligned operands only)
        a.A16, a.out_bf16 = (_p(x) if xb else _UNALLOCATED), int(want16)
        # (only the wide-tile kernel serves a phase with an image, and it writes either storage: vae_conv_io16_ok is not asked)
        use16 = bool(lib.query("vae_conv_phase_ok", C.byref(a)))
        if not use16:
            a.A16, a.out_bf16 = None, 0
    if not use16:
        if xb or not lib.query("vae_conv_phase_ok", C.byref(a)):
            return None
        want16 = False
    elif not xb:
        x._b16 = pack_bf16(x, torch.empty(x.shape, device=x.device, dtype=torch.bfloat16))  # the layer's weight gradient reads the same image
        a.A16 = _p(x._b16)
    out = torch.empty((B, 2 * H, 2 * W, Co), device=x.device, dtype=torch.bfloat16 if want16 else torch.float32)
    a.C = _p(out)
    for _, a.tapmask, a.c_oy, a.c_ox, a.W, a.Wh in _phases(wv):
        _launch_igemm(a)
    return out


def _upconv_phase_dgrad(dy, wv, in_hw, dy16=None):
    """dy [B,2H,2W,Co] (fp32, or None when only the bf16 form dy16 exists) -> gradient wrt the LOW-resolution input
    [B,H,W,Ci], fp32 (the four phases add up through the residual input), or None when not served"""
    src = dy if dy is not None else dy16
    B, Hy, Wy, Co = src.shape
    H, W = in_hw
    _, _, _, Ci = wv.shape
    a = phase_args(B, H, W, Co, Ci, True)
    a.A, a.W, a.Wh = _p(src), _p(wv), _wh(wv)
    use16 = False
    if PRECISION == PREC_BF16 and a.Wh is not None and Co % 8 == 0:
        # the image: dy16, else a copy of dy made below (a misaligned fp32 dy is refused through A, as in _upconv_phase_fwd)
        a.A16 = _p(dy16) if dy16 is not None else _UNALLOCATED
        use16 = bool(lib.query("vae_conv_phase_ok", C.byref(a)))
        if not use16:
            a.A16 = None
    if not use16 and (dy is None or not lib.query("vae_conv_phase_ok", C.byref(a))):
        return None
    if use16 and dy16 is None:
        dy16 = pack_bf16(dy, torch.empty(dy.shape, device=dy.device, dtype=torch.bfloat16))
        a.A16 = _p(dy16)
    out = torch.empty((B, H, W, Ci), device=src.device, dtype=torch.float32)
    a.C = _p(out)
    for ph, a.tapmask, a.a_oy, a.a_ox, a.W, a.Wh in _phases(wv):
        a.res = _p(out) if ph else None  # the four phases add up
        _launch_igemm(a)
    return out


def _chk_act(t: torch.Tensor, name: str):
    if not (t.is_cuda and t.dtype in (torch.float32, torch.bfloat16)):
        raise ValueError(f"{name}: expected a float32 or bfloat16 CUDA tensor, got {t.dtype} on {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous NHWC tensor, strides {t.stride()}")


def conv_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], kind: str, *,
             xf: int = XF_NONE, stats: Optional[Stats] = None, res: Optional[torch.Tensor] = None,
             track: Optional[torch.Tensor] = None, a16: Optional[torch.Tensor] = None,
             gstat_groups: Optional[int] = None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """x [B,H,W,Cs] (Cs >= Cin, extra channels must be zero-weighted i.e. Cin is taken from w), stored as fp32 or bf16.
    a16: bf16 image of XF(x) (then xf / stats are not applied again; x only gives the geometry).
    gstat_groups: the output feeds a GroupNorm with that many groups: where the kernel has a statistics epilogue the
    partial sums are attached to the returned tensor (`_gstat`) and gn_stats() on it skips its pass over the tensor.
    out_dtype: storage of the result; None = bf16 when bf16 mode stores activations as bf16 (act16()) and the layer has at
    least ACT16_MIN_C output channels, else fp32.  A kernel that cannot honour the storage of an operand gets fp32 copies."""
    _chk_act(x, "conv_fwd.x")
    wv = ohwi(w)
    Co, kh, kw, Ci = wv.shape
    want16 = (out_dtype == torch.bfloat16) if out_dtype is not None else (act16() and Co >= ACT16_MIN_C)
    if a16 is not None:
        assert a16.shape == x.shape and a16.dtype == torch.bfloat16 and a16.is_contiguous()
        xf = XF_NONE
    if kind == "c3up" and xf == XF_NONE and res is None and track is None and a16 is None and not want16:
        out = _upconv_wino_fwd(x, wv, bias)
        if out is not None:
            return out
    if kind == "c3up" and PHASE_UPCONV and xf == XF_NONE and res is None and track is None and a16 is None:
        out = _upconv_phase_fwd(x, wv, bias, want16)
        if out is not None:
            return out if (out.dtype == torch.bfloat16) == want16 else _like(out, want16)
    B, H, W, Cs = x.shape
    assert kh * kw == (1 if kind == "c1" else 9) and Ci <= Cs, (kind, wv.shape, x.shape)
    a = fwd_args(kind, B, H, W, Cs, Co, Ci, xf=xf)
    if xf != XF_NONE and not lib.query("vae_xf_fusable_rows", C.byref(a.g), a.M, Ci):
        x, xf, a.xf = gn_apply(x, stats, xf), XF_NONE, XF_NONE  # tiny spatial size: several batch items per tile
    a.A, a.W, a.Wh, a.C, a.bias, a.track = _p(x), _p(wv), _wh(wv), _UNALLOCATED, _p(bias), _p(track)
    xb = x.dtype == torch.bfloat16
    if a16 is not None:
        a.A16 = _p(a16)
    elif xb and xf == XF_NONE:
        a.A16 = _p(x)   # a bf16 tensor IS its own image; the dispatcher turns it into a_bf16 for the flat kernels
    elif xb:
        a.a_bf16 = 1    # bf16 storage with a transform on load: the flat / <= 4-channel kernels
    a.out_bf16 = int(want16)
    if res is not None:  # the residual is stored like the output: res itself, or a copy made once the storage is settled
        _chk_act(res, "conv_fwd.res")
        assert res.shape == (B, a.g.Ho, a.g.Wo, Co)
        a.res, a.res_bf16 = (_p(res) if _b16(res) == a.out_bf16 else _UNALLOCATED), a.out_bf16
    if xf != XF_NONE:
        assert stats is not None and stats.scale.shape == (B, Cs)
        a.scale, a.shift = _p(stats.scale), _p(stats.shift)
    if track is not None:
        assert track.numel() >= ((a.M + 127) // 128) * Co
    if (a.A16 or a.a_bf16 or a.out_bf16 or a.res_bf16) and not lib.query("vae_conv_io16_ok", C.byref(a)):
        # the kernel serving this launch takes fp32 storage only (unvectorised shapes, a tracked halo-tile output, ...): fp32
        # copies.  (The residual still goes through the output's storage first, so an fp32 one is rounded to bf16 as on the
        # bf16 kernels.)
        x32 = to_f32(a16) if a16 is not None else to_f32(x)
        y = conv_fwd(x32, w, bias, kind, xf=xf, stats=stats, res=None if res is None else to_f32(_like(res, want16)), track=track,
                     gstat_groups=None if want16 else gstat_groups, out_dtype=torch.float32)
        # (epilogue statistics would describe the UNROUNDED result: a re-stored one goes without them, and gn_stats makes its own
        # pass over the tensor as stored)
        return to_bf16(y) if want16 else y
    wino = _wino_ok(a)
    if res is not None:
        res = _like(res, want16)
        a.res = _p(res)
    out = torch.empty((B, a.g.Ho, a.g.Wo, Co), device=x.device, dtype=torch.bfloat16 if want16 else torch.float32)
    a.C = _p(out)
    wu = _wino_weights(a, x.device) if wino else None
    if gstat_groups:  # GroupNorm statistics of the output from this launch's epilogue where the serving kernel has one
        a.gstat_groups = int(gstat_groups)
        nch = lib.query("vae_conv_gstat_chunks", C.byref(a))
        if nch > 0:
            ws = torch.empty((B, nch, int(gstat_groups), 2), device=x.device, dtype=torch.float32)
            a.gstat = _p(ws)
            out._gstat = (ws, int(gstat_groups), nch)
    _launch_igemm(a)
    return out


def _gnb_key(x, st, gamma, beta, silu) -> tuple:
    """identity of the GroupNorm(+SiLU) a dgrad epilogue's backward sums were computed for: input, statistics, affine
    parameters, activation flag and shape"""
    return (x.data_ptr(), st.mean.data_ptr(), st.rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), bool(silu), tuple(x.shape))


class GnCtx(NamedTuple):
    """the GroupNorm (+SiLU) whose output the convolution read: what its backward needs besides dL/d(output)"""
    x: torch.Tensor       # the GroupNorm input, NHWC, as stored
    st: "Stats"
    gamma: torch.Tensor
    beta: torch.Tensor
    silu: bool
    groups: int


def conv_dgrad(dy: torch.Tensor, w: torch.Tensor, kind: str, in_hw: Tuple[int, int], out_bf16: bool = False,
               out_dtype: Optional[torch.dtype] = None, gnb: Optional[GnCtx] = None) -> torch.Tensor:
    """gradient wrt the conv input (the XF'ed tensor); dy [B,Ho,Wo,Co] -> [B,H,W,Ci].
    gnb: the result is dL/d silu(gn(x)) of this GroupNorm and goes to gn_bwd: where the kernel serving the launch can, its
    epilogue also leaves gn_bwd's first pass (the per-chunk sums over x and the result), attached as `_gnb = (ws, nchunk)`.
    dy: fp32 (optionally with a bf16 image attached, `_b16`) or a bf16 tensor.  Storage of the result: out_dtype, or bf16 when
    act16() and Ci >= ACT16_MIN_C, or when out_bf16 is asked for and the halo-tile kernel serving the layer can write it (fp32
    storage mode: the caller feeds it to gn_bwd only), else fp32."""
    dy16 = _grad16(dy)
    dy32 = dy if dy.dtype == torch.float32 else None
    _chk_act(dy, "conv_dgrad.dy")
    wv = ohwi(w)
    Co, kh, kw, Ci = wv.shape
    B, (H, W) = dy.shape[0], in_hw
    assert kh * kw == (1 if kind == "c1" else 9) and dy.shape == (B, *out_hw(kind, H, W), Co), (kind, wv.shape, dy.shape, in_hw)
    forced = out_dtype is not None
    want16 = (out_dtype == torch.bfloat16) if forced else (act16() and Ci >= ACT16_MIN_C)
    use16 = dy16 is not None and (dy32 is None or grad_image_ok(kind, (B, H, W, Ci), Co, Ci))
    if kind == "c3up" and not want16:
        out = _upconv_wino_dgrad(dy32, wv, in_hw)
        if out is not None:
            return out
    if kind == "c3up" and PHASE_UPCONV:
        out = _upconv_phase_dgrad(dy32, wv, in_hw, dy16)
        if out is not None:
            return _like(out, want16)
    a = dgrad_args(kind, B, H, W, Co, Ci)
    dev = dy.device
    a.A, a.W, a.Wh = _p(dy32 if dy32 is not None else dy16), _p(wv), _wh(wv)  # with A16 the kernel reads the image; A only gives the alignment
    a.A16 = _p(dy16) if use16 else None
    a.C = _UNALLOCATED
    pool = kind == "c3up"  # (the virtual-upsample fallback: the high-resolution gradient is summed 2x2 in fp32)
    if not pool and (want16 or (out_bf16 and not forced and PRECISION == PREC_BF16 and kind == "c3")):
        a.out_bf16 = 1  # (as asked; kept when the kernel serving the launch can write it)
        a.out_bf16 = int(lib.query("vae_conv_io16_ok", C.byref(a)))
    if a.A16 and not lib.query("vae_conv_io16_ok", C.byref(a)):  # an fp32-only kernel: hand it an fp32 copy of the gradient
        return _like(conv_dgrad(to_f32(dy16), w, kind, in_hw, out_dtype=torch.float32), want16)
    wino = _wino_ok(a)
    out = torch.empty((B, a.g.Ho, a.g.Wo, Ci), device=dev, dtype=torch.bfloat16 if a.out_bf16 else torch.float32)
    a.C = _p(out)
    wu = _wino_weights(a, dev) if wino else None
    # GroupNorm-backward partial sums from this launch's epilogue where the serving kernel has one (a result that is re-stored as
    # bf16 below drops its attributes: no sums are computed for it)
    if gnb is not None and not pool and gnb.x.shape == out.shape and not (want16 and out.dtype != torch.bfloat16):
        a.gnb_x, a.gnb_x_bf16 = _p(gnb.x), _b16(gnb.x)
        a.gnb_mean, a.gnb_rstd, a.gnb_gamma, a.gnb_beta = _p(gnb.st.mean), _p(gnb.st.rstd), _p(gnb.gamma), _p(gnb.beta)
        a.gnb_groups, a.gnb_silu = int(gnb.groups), int(gnb.silu)
        nch = lib.query("vae_conv_gnb_chunks", C.byref(a))
        if nch > 0:
            ws = torch.empty((B, nch, Ci, 2), device=dev, dtype=torch.float32)
            a.gnb_ws = _p(ws)
            # (what the sums belong to: gn_bwd takes them only for exactly this GroupNorm, see _gnb_key)
            out._gnb = (ws, nch, _gnb_key(gnb.x, gnb.st, gnb.gamma, gnb.beta, gnb.silu))
        else:
            a.gnb_x = None
    _launch_igemm(a)
    if pool:
        pooled = torch.empty((B, H, W, Ci), device=dev, dtype=torch.float32)
        lib.call("vae_sumpool2x2", _p(out), B, H, W, Ci, _p(pooled), _stream())
        out = pooled
    if want16 and out.dtype != torch.bfloat16:
        return to_bf16(out)
    return out


def _upconv_phase_wgrad(dy, x, gv, bgrad_out, dy16=None) -> bool:
    """weight (and bias) gradient of conv3x3(nearest_upsample_2x(x)) from four phase weight gradients on the low-resolution
    grid (each computes the 4 taps of its 2x2 effective kernel), folded back into the 3x3 gradient; False = not served.
    bf16 mode: both operands as bf16 images (x at low resolution, dy at high resolution through the strided view); either
    may be a bf16-stored tensor (dy None: only dy16 exists)."""
    Co, _, _, Ci = gv.shape
    B, H, W, Cs = x.shape
    if Cs != Ci:
        return False
    xb = x.dtype == torch.bfloat16
    a = wgrad_phase_args(B, H, W, Co, Ci)
    a.dY, a.X = _p(dy if dy is not None else dy16), _p(x)
    if not lib.query("vae_wgrad_phase_ok", C.byref(a)):
        return False
    images = PRECISION == PREC_BF16 and Cs % 8 == 0 and Co % 8 == 0
    x16 = None
    if images:  # the images that exist already; the plan is asked about the others as copies made below
        x16 = x if xb else getattr(x, "_b16", None)
        a.X16 = _p(x16) if x16 is not None else _UNALLOCATED
        a.dY16 = _p(dy16) if dy16 is not None else _UNALLOCATED
    elif xb or dy is None:
        return False  # the fp32 halo-tile kernel needs fp32 operands
    ns, fus = C.c_int32(0), C.c_int32(0)
    lib.call("vae_wgrad_plan", C.byref(a), C.byref(ns), C.byref(fus))
    ns = ns.value
    a.nsplit = ns
    if images:
        if x16 is None:
            x16 = pack_bf16(x, torch.empty(x.shape, device=x.device, dtype=torch.bfloat16))
        if dy16 is None:
            dy16 = pack_bf16(dy, torch.empty(dy.shape, device=dy.device, dtype=torch.bfloat16))
            dy._b16 = dy16  # the dgrad that follows reads the same image
        a.X16, a.dY16 = _p(x16), _p(dy16)
    n = Co * 9 * Ci
    dwe = torch.empty((4, n), device=x.device, dtype=torch.float32)
    dbe = torch.empty((4, Co), device=x.device, dtype=torch.float32) if bgrad_out is not None else None
    partial = torch.empty((ns, n), device=x.device, dtype=torch.float32) if ns > 1 else None
    bpart = torch.empty((ns, Co), device=x.device, dtype=torch.float32) if bgrad_out is not None else None
    a.partial, a.bias_partial = _p(partial), _p(bpart)
    for ph, a.tapmask, a.y_oy, a.y_ox, _, _ in _phases():
        a.out = _p(dwe[ph]) if ns == 1 else None  # (one split: the kernel writes the phase's gradient itself)
        _launch_wgrad(a)
        _reduce_splits(partial, bpart, ns, n, Co, dwe[ph], None if dbe is None else dbe[ph])
    lib.call("vae_upconv_fold_wgrad", _p(dwe), _p(dbe), Co, Ci, _p(gv), _p(bgrad_out), _stream())
    return True


def _wgrad_wino(a: WgradArgs, gv: torch.Tensor, bgrad_out: Optional[torch.Tensor], dev) -> bool:
    """fp32 plain 3x3 stride-1 layers: Winograd F(3x3,2x2) weight gradient (csrc/wgrad3_wino.hip) into a transform-domain slab,
    then the fixed-order reduction + output transform.  False when the layer is not served."""
    if not WINOGRAD or PRECISION != PREC_F32:
        return False
    ns = C.c_int32(0)
    lib.call("vae_wgrad_wino_plan", C.byref(a), C.byref(ns))
    ns = ns.value
    if ns <= 0:
        return False
    npos = int(lib.query("vae_wgrad_wino_positions", C.byref(a)))  # 16, or 9 for an upsampler convolution
    slab = torch.empty((ns, npos * a.N * a.M), device=dev, dtype=torch.float32)
    bpart = torch.empty((ns, a.M), device=dev, dtype=torch.float32) if bgrad_out is not None else None
    a.nsplit, a.partial, a.bias_partial = ns, _p(slab), _p(bpart)
    fl = 2.0 * a.M * a.N * a.npix * 9  # (npix = output pixels: the direct convolution's count in both cases)
    if npos == 9:
        _timed("wgrad3_upwino_kernel", fl, fl * 0.25, "vae_wgrad_wino", C.byref(a), _stream())
    else:
        _timed(f"wgrad3_wino_kernel<{a.xf}>", fl, fl * WINO_EXECUTED, "vae_wgrad_wino", C.byref(a), _stream())
    _timed("wgrad_wino_reduce (split sum + output transform)", 0.0, 0.0, "vae_wgrad_wino_reduce", _p(slab), ns, npos, a.N, a.M,
           None, _p(gv), _p(bpart), _p(bgrad_out), _stream())  # (no scratch buffer: the reduction reads the slab once)
    return True


def conv_wgrad(dy: torch.Tensor, x: torch.Tensor, kind: str, wgrad_out: torch.Tensor,
               bgrad_out: Optional[torch.Tensor], *, xf: int = XF_NONE, stats: Optional[Stats] = None,
               x16: Optional[torch.Tensor] = None):
    """writes dW into `wgrad_out` (a view with the weight's OHWI memory) and db into `bgrad_out`.
    dy and x: fp32 or bf16 tensors; x16: bf16 image of XF(x) (as conv_fwd's a16)."""
    dy16 = _grad16(dy)
    dy32 = dy if dy.dtype == torch.float32 else None
    _chk_act(dy, "conv_wgrad.dy")
    _chk_act(x, "conv_wgrad.x")
    if x16 is not None:
        assert x16.shape == x.shape and x16.dtype == torch.bfloat16 and x16.is_contiguous()
        xf = XF_NONE
    gv = ohwi(wgrad_out)
    Co, _, _, Ci = gv.shape
    B, H, W, Cs = x.shape
    assert dy.shape == (B, *out_hw(kind, H, W), Co), (dy.shape, kind, x.shape, Co)
    if (kind == "c3up" and PRECISION == PREC_F32 and WINOGRAD and xf == XF_NONE and x16 is None and dy32 is not None
            and x.dtype == torch.float32):
        a = wgrad_args(kind, B, H, W, Cs, Co, Ci)  # the 9-position scheme of csrc/wgrad3_upwino.hip (fp32)
        a.dY, a.X = _p(dy32), _p(x)
        if _wgrad_wino(a, gv, bgrad_out, x.device):
            return
    if kind == "c3up" and PHASE_UPCONV and xf == XF_NONE and x16 is None and _upconv_phase_wgrad(dy32, x, gv, bgrad_out, dy16):
        return
    xb = x.dtype == torch.bfloat16
    use16 = dy16 is not None and (dy32 is None or grad_image_ok(kind, x.shape, Co, Ci))
    a = wgrad_args(kind, B, H, W, Cs, Co, Ci, xf=xf)
    a.dY, a.X = _p(dy32 if dy32 is not None else dy16), _p(x)
    a.dY16 = _p(dy16) if use16 else None
    if x16 is not None:
        a.X16 = _p(x16)
    elif xb and xf == XF_NONE:
        a.X16 = _p(x)  # a bf16 tensor is its own image (the dispatcher turns it into x_bf16 for the flat kernels)
    elif xb:
        a.x_bf16 = 1
    if xf != XF_NONE:
        assert stats is not None
        a.scale, a.shift = _p(stats.scale), _p(stats.shift)
    if _wgrad_wino(a, gv, bgrad_out, x.device):
        return
    ns, fus = C.c_int32(0), C.c_int32(0)
    lib.call("vae_wgrad_plan", C.byref(a), C.byref(ns), C.byref(fus))
    if xf != XF_NONE and not fus.value:  # tiny spatial size: several batch items per split
        x, xf = gn_apply(x, stats, xf), XF_NONE
        a.X, a.xf, a.scale, a.shift, a.x_bf16 = _p(x), XF_NONE, None, None, 0
        lib.call("vae_wgrad_plan", C.byref(a), C.byref(ns), C.byref(fus))
    if (a.X16 or a.dY16 or a.x_bf16) and not lib.query("vae_wgrad_io16_ok", C.byref(a)):
        # an fp32-only kernel: fp32 copies of the operands (x16 already holds XF(x))
        x32 = to_f32(x16) if x16 is not None else to_f32(x)
        return conv_wgrad(dy32 if dy32 is not None else to_f32(dy16), x32, kind, wgrad_out, bgrad_out, xf=xf, stats=stats)
    ns = ns.value
    a.nsplit = ns
    partial = None
    if ns == 1:
        a.out = _p(gv)
    else:
        partial = torch.empty((ns, gv.numel()), device=x.device, dtype=torch.float32)
        a.partial = _p(partial)
    bpart = None
    if bgrad_out is not None:  # bias gradient = column sums of dY, folded into the wgrad kernel
        bpart = torch.empty((ns, Co), device=x.device, dtype=torch.float32)
        a.bias_partial = _p(bpart)
    _launch_wgrad(a)
    _reduce_splits(partial, bpart, ns, gv.numel(), Co, gv, bgrad_out)


# ------------------------------------------------------------------ GroupNorm
_GN_TARGET = 1024  # workgroups per GroupNorm streaming pass (B * nchunk); tools/gn_bench.py: best of 256..4096 on MI355X


def _gn_nchunk(B: int, HW: int, Cc: int) -> int:
    pr = max(1, 256 // (Cc // 4))
    return max(1, min(_GN_TARGET // max(B, 1), HW // (16 * pr) if HW >= 16 * pr else 1))


def gn_stats(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, G: int = GN_GROUPS, eps: float = GN_EPS) -> Stats:
    _chk_act(x, "gn_stats.x")
    B, H, W, Cc = x.shape
    HW = H * W
    dev = x.device
    fused = getattr(x, "_gstat", None)  # partial sums left by the conv epilogue that produced x (conv_fwd(gstat_groups=G))
    if fused is not None and fused[1] == G:
        ws, nch = fused[0], fused[2]
    else:
        nch = _gn_nchunk(B, HW, Cc)
        ws = torch.empty((B, nch, G, 2), device=dev, dtype=torch.float32)
        lib.call("vae_gn_stats_partial", _p(x), _b16(x), B, HW, Cc, G, nch, _p(ws), _stream())
    mean = torch.empty((B, G), device=dev, dtype=torch.float32)
    rstd = torch.empty((B, G), device=dev, dtype=torch.float32)
    scale = torch.empty((B, Cc), device=dev, dtype=torch.float32)
    shift = torch.empty((B, Cc), device=dev, dtype=torch.float32)
    lib.call("vae_gn_stats_final", _p(ws), B, HW, Cc, G, nch, _p(gamma), _p(beta), eps, _p(mean), _p(rstd),
             _p(scale), _p(shift), _stream())
    return Stats(mean, rstd, scale, shift)


def gn_apply(x: torch.Tensor, st: Stats, xf: int) -> torch.Tensor:
    B, H, W, Cc = x.shape
    y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    lib.call("vae_gn_apply", _p(x), _b16(x), _p(st.scale), _p(st.shift), B, H * W, Cc, xf, _p(y), _stream())
    return y


def gn_track(x: torch.Tensor, st: Stats) -> torch.Tensor:
    """mean over (b,h,w) of |gn(x)| per channel (monitor.py:66), no tensor materialised."""
    B, H, W, Cc = x.shape
    HW = H * W
    nch = _gn_nchunk(B, HW, Cc)
    ws = torch.empty((B * nch, Cc), device=x.device, dtype=torch.float32)
    out = torch.empty((Cc,), device=x.device, dtype=torch.float32)
    lib.call("vae_gn_track_partial", _p(x), _b16(x), _p(st.scale), _p(st.shift), B, HW, Cc, nch, _p(ws), _stream())
    lib.call("vae_track_final", _p(ws), B * nch, Cc, 1.0 / float(B * HW), _p(out), _stream())
    return out


def _nhwc_ld(who: str, x: torch.Tensor) -> int:
    B, H, W, Cc = x.shape
    ld = x.stride(2)
    if x.stride(3) != 1 or ld < Cc or x.stride(1) != W * ld or x.stride(0) != H * W * ld:
        raise ValueError(f"{who}: expected NHWC rows with contiguous channels, strides {x.stride()}")
    return ld


def _stat_operand(who: str, x: torch.Tensor, stats: Optional[Stats], xf: int):
    """the NHWC operand of a statistics pass and the GroupNorm transform applied to it on the fly
    -> (B, H * W, C, pixel stride, scale, shift); scale and shift are None without a transform"""
    if x.dim() != 4 or not x.is_cuda or x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{who}: expected a 4-D NHWC fp32 / bf16 CUDA tensor, got {tuple(x.shape)} {x.dtype} on {x.device}")
    ld = _nhwc_ld(who, x)
    B, H, W, Cc = x.shape
    if (stats is None) != (xf == XF_NONE):
        raise ValueError(f"{who}: a GroupNorm transform (xf) needs its stats and stats need an xf")
    if stats is None:
        return B, H * W, Cc, ld, None, None
    if tuple(stats.scale.shape) != (B, ld) or not stats.scale.is_contiguous() or x.storage_offset() % ld:
        raise ValueError(f"{who}: stats rows {tuple(stats.scale.shape)} do not describe this tensor's channels")
    return B, H * W, Cc, ld, stats.scale, stats.shift


# a workgroup's channel tile in units of (four channels, one channel): _stat_chunks' vec_tile and scalar_tile
_MOMENTS_TILE = (256, 256)   # moments(): 256 units, whatever the unit
_CHANHIST_TILE = (32, 128)   # chanhist(): 128 channels
_CHANGRAD_TILE = (64, 256)   # changrad(), changroup(), actreg_stats(): 256 channels


def _stat_chunks(B: int, HW: int, Cc: int, vec_tile: int, scalar_tile: int) -> int:
    """pixel chunks per image of a statistics partial pass whose workgroup takes a tile of vec_tile units of four channels (C a
    multiple of 4) or of scalar_tile single channels: B * nchunk * tiles workgroups near _GN_TARGET, a chunk no shorter than 16
    pixels per pixel row of a workgroup, and every chunk non-empty"""
    units, tile = (Cc // 4, vec_tile) if Cc % 4 == 0 else (Cc, scalar_tile)
    pr = max(1, 256 // min(tile, units))
    tiles = (units + tile - 1) // tile
    nch = max(1, min(_GN_TARGET // max(B * tiles, 1), HW // (16 * pr)))
    per = (HW + nch - 1) // nch
    return (HW + per - 1) // per


def moments(x: torch.Tensor, stats: Optional[Stats] = None, xf: int = XF_NONE) -> torch.Tensor:
    """the other ActivityMonitor metrics of y = XF(x) in one read of x, no tensor materialised: a device vector of C + 2 fp32
    values, [per-channel mean |y| (as gn_track), mean of y, unbiased std of y (torch.Tensor.std)].  x: NHWC, fp32 or bf16
    storage, channels contiguous; a channel-prefix view of a wider buffer (x4[..., :3]) is read in place.  stats: the
    GroupNorm whose per-(b, c) scale / shift XF applies (rows as wide as the buffer's pixel stride)."""
    B, HW, Cc, ld, scale, shift = _stat_operand("moments", x, stats, xf)
    nch = _stat_chunks(B, HW, Cc, *_MOMENTS_TILE)
    dev = x.device
    ws = torch.empty((Cc, B * nch, 4), device=dev, dtype=torch.float32)
    chan = torch.empty((Cc, 2), device=dev, dtype=torch.float64)
    out = torch.empty((Cc + 2,), device=dev, dtype=torch.float32)
    lib.call("vae_moments_partial", _p(x), _b16(x), _p(scale), _p(shift), xf, B, HW, Cc, ld, nch, _p(ws), _stream())
    lib.call("vae_moments_final", _p(ws), B, HW, Cc, nch, _p(chan), _p(out), _stream())
    return out


CHANHIST_BINS = 48  # vae_chanhist_bins(): bin = clamp(floor(log2 |y|) + 31, 0, 47)


def chanhist(x: torch.Tensor, stats: Optional[Stats] = None, xf: int = XF_NONE, tau: float = 1e-3):
    """per-channel magnitude statistics of y = XF(x) in one read of x, no tensor materialised: (hist int64 [C, 48], nzero int64
    [C], absmax fp32 [C]) on the device.  hist[c, k] counts the values of channel c whose fp32 exponent puts them in bin
    k = clamp(floor(log2 |y|) + 31, 0, 47) (bin 0: |y| < 2^-30 with zeros and denormals, bin 47: |y| >= 2^16, inf, NaN); every
    row sums to B * H * W.  nzero[c] counts |y| < tau (compared in fp32; NaN is not below), absmax[c] is max |y| (NaN if the
    channel holds one).  x, stats and xf as in moments(); nothing synchronises the host."""
    B, HW, Cc, ld, scale, shift = _stat_operand("chanhist", x, stats, xf)
    nch = _stat_chunks(B, HW, Cc, *_CHANHIST_TILE)
    dev = x.device
    n = C.c_int64(0)
    lib.call("vae_chanhist_workspace", B, HW, Cc, nch, C.byref(n))
    ws = torch.empty((n.value,), device=dev, dtype=torch.int32)
    hist = torch.empty((Cc, CHANHIST_BINS), device=dev, dtype=torch.int64)
    nzero = torch.empty((Cc,), device=dev, dtype=torch.int64)
    absmax = torch.empty((Cc,), device=dev, dtype=torch.float32)
    lib.call("vae_chanhist_partial", _p(x), _b16(x), _p(scale), _p(shift), xf, B, HW, Cc, ld, nch, float(tau), _p(ws), _stream())
    lib.call("vae_chanhist_final", _p(ws), B, HW, Cc, nch, _p(hist), _p(nzero), _p(absmax), _stream())
    return hist, nzero, absmax


def changroup_chunks(B: int, HW: int, Cc: int) -> int:
    """pixel chunks per image of changroup(): B * nchunk * (tiles of 256 channels) workgroups near _GN_TARGET, a chunk no shorter
    than 16 pixels per pixel row of a workgroup, and every chunk non-empty (the rule of changrad_chunks: the two kernels share
    their layout).  The workspace, 3 doubles per (image, chunk, channel), stays below chanhist()'s 50 words at every shape: a
    tile twice as wide gives at most twice the chunks."""
    return changrad_chunks(B, HW, Cc)


def changroup(x: torch.Tensor, stats: Optional[Stats] = None, xf: int = XF_NONE) -> torch.Tensor:
    """per-(sample, channel) sums of y = XF(x) in one read of x, no tensor materialised: a float64 [B, C, 3] device tensor of
    S1 = sum y, S2 = sum y^2 and A = sum |y| over the H * W pixels of every (b, c).  y is evaluated in fp32, every sum is float64
    from the first addition on (csrc/changroup.hip), in a fixed order: two calls agree bitwise.  A NaN or an infinity reaches the
    sums of its own (b, c) only.  x, stats and xf as in moments(); nothing synchronises the host.  changroup_metrics() turns the
    sums into the GroupNorm group dynamics and per-sample activity figures of the ActivityMonitor."""
    B, HW, Cc, ld, scale, shift = _stat_operand("changroup", x, stats, xf)
    nch = changroup_chunks(B, HW, Cc)
    dev = x.device
    n = C.c_int64(0)
    lib.call("vae_changroup_workspace", B, HW, Cc, nch, C.byref(n))
    ws = torch.empty((n.value,), device=dev, dtype=torch.float64)
    sums = torch.empty((B, Cc, 3), device=dev, dtype=torch.float64)
    lib.call("vae_changroup_partial", _p(x), _b16(x), _p(scale), _p(shift), xf, B, HW, Cc, ld, nch, _p(ws), _stream())
    lib.call("vae_changroup_final", _p(ws), B, HW, Cc, nch, _p(sums), _stream())
    return sums


def changroup_metrics(sums: torch.Tensor, HW: int, groups: Optional[int], eps: float, tau: float):
    """the per-sample arithmetic behind the ActivityMonitor's group and sample metrics, in float64 on the device of `sums`
    ([B, C, 3] = sum y, sum y^2, sum |y| over the n = HW pixels of every (b, c): changroup(), or the same sums from torch).
    With cg = C / groups and g(c) = c // cg:
        mu_bg = sum_{c in g} S1_bc / (n cg)                   v_bc = max(0, S2_bc - 2 mu_bg S1_bc + n mu_bg^2)
        V_bg = sum_{c in g} v_bc                              share_bc = v_bc / V_bg (0 where V_bg == 0)
        nrms_bc = sqrt((v_bc / n) / (V_bg / (n cg) + eps))    dom_bg = max_{c in g} share_bc          m_bc = A_bc / n
    Returns (chan float64 [5, C], grp float64 [G], B): the rows of chan are the sums over the B samples of share, nrms, m, m^2
    and [m >= tau]; grp is the sum over the samples of dom.  groups None (no group metric asked for): the first two rows of chan
    are zero and grp is empty.  Every monitor metric is a mean over samples of a per-sample quantity or a function of two such
    means, so forwards and data-parallel ranks combine by adding these sums and the sample counts, whatever their batch sizes.
    A NaN or an infinity in a (b, c) stays in the group figures of its (b, group) and in the sample figures of its channel."""
    if sums.dim() != 3 or sums.shape[2] != 3 or sums.dtype != torch.float64:
        raise ValueError(f"changroup_metrics: expected float64 [B, C, 3] sums, got {tuple(sums.shape)} {sums.dtype}")
    B, Cc, _ = sums.shape
    if not HW >= 1:
        raise ValueError(f"changroup_metrics: HW = {HW}")
    # n as a tensor: torch divides a device tensor by a Python number as a product with its rounded reciprocal, and a constant
    # channel's v is exactly 0 only if mu is the correctly rounded quotient
    n = torch.full((), float(HW), device=sums.device, dtype=torch.float64)
    chan = torch.zeros((5, Cc), device=sums.device, dtype=torch.float64)
    if groups is None:
        grp = torch.zeros((0,), device=sums.device, dtype=torch.float64)
    else:
        G = int(groups)
        if G < 1 or Cc % G:
            raise ValueError(f"changroup_metrics: {Cc} channels do not divide into {groups} groups")
        cg = Cc // G
        S1 = sums[:, :, 0].reshape(B, G, cg)
        S2 = sums[:, :, 1].reshape(B, G, cg)
        ncg = n * float(cg)
        mu = S1.sum(dim=2, keepdim=True) / ncg
        v = S2 - 2.0 * mu * S1 + n * mu * mu
        v = torch.where(v < 0.0, torch.zeros_like(v), v)  # (not clamp: a NaN stays)
        V = v.sum(dim=2, keepdim=True)
        share = torch.where(V == 0.0, torch.zeros_like(v), v / V)
        nrms = torch.sqrt((v / n) / (V / ncg + float(eps)))
        chan[0] = share.reshape(B, Cc).sum(dim=0)
        chan[1] = nrms.reshape(B, Cc).sum(dim=0)
        # the largest share of a group; a NaN in the group makes it NaN (amax propagates)
        grp = share.amax(dim=2).sum(dim=0)
    m = sums[:, :, 2] / n
    chan[2] = m.sum(dim=0)
    chan[3] = (m * m).sum(dim=0)
    chan[4] = (m >= float(tau)).to(torch.float64).sum(dim=0)
    return chan, grp, B


def changrad_chunks(B: int, HW: int, Cc: int) -> int:
    """pixel chunks per image of changrad(): B * nchunk * (tiles of 256 channels) workgroups near _GN_TARGET, a chunk no shorter
    than 16 pixels per pixel row of a workgroup, and every chunk non-empty"""
    return _stat_chunks(B, HW, Cc, *_CHANGRAD_TILE)


def changrad(a: torch.Tensor, g: torch.Tensor):
    """per-channel gradient metrics of one backward pass in one read of a module's output `a` and the gradient `g` of the loss
    with respect to it: (sums float64 [3, C], absmax fp32 [C]) on the device.  sums[0] = mean |g| over the N = B * H * W pixel
    rows, sums[1] = sum_b sum_p a g (the gradient of a per-channel gain at 1), sums[2] = (1 / B) sum_b |sum_p a g| (the Taylor
    saliency); absmax = max |g| (NaN if the channel holds one).  a and g: 4-D NHWC of one shape, each fp32 or bf16, channels
    contiguous, each with its own pixel stride (a channel-prefix view is read in place).  Products are rounded once and summed in
    fp32 inside a workgroup (csrc/changrad.hip), everything after is float64 in a fixed order: two calls agree bitwise.  Nothing
    synchronises the host."""
    for t in (a, g):
        if t.dim() != 4 or not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"changrad: expected 4-D NHWC fp32 / bf16 CUDA tensors, got {tuple(t.shape)} {t.dtype} on {t.device}")
    if tuple(a.shape) != tuple(g.shape) or a.device != g.device:
        raise ValueError(f"changrad: output {tuple(a.shape)} on {a.device} and gradient {tuple(g.shape)} on {g.device} differ")
    lda, ldg = _nhwc_ld("changrad", a), _nhwc_ld("changrad", g)
    B, H, W, Cc = a.shape
    HW = H * W
    nch = changrad_chunks(B, HW, Cc)
    dev = a.device
    n = C.c_int64(0)
    lib.call("vae_changrad_workspace", B, HW, Cc, nch, C.byref(n))
    ws = torch.empty((n.value,), device=dev, dtype=torch.int32)
    sums = torch.empty((3, Cc), device=dev, dtype=torch.float64)
    absmax = torch.empty((Cc,), device=dev, dtype=torch.float32)
    lib.call("vae_changrad_partial", _p(a), _b16(a), lda, _p(g), _b16(g), ldg, B, HW, Cc, nch, _p(ws), _stream())
    lib.call("vae_changrad_final", _p(ws), B, HW, Cc, nch, _p(sums), _p(absmax), _stream())
    return sums, absmax


ACTREG_KINDS = ("ceiling", "floor")  # the C ABI's kind 0 / 1


def actreg_chunks(B: int, HW: int, Cc: int) -> int:
    """pixel chunks per image of actreg_stats(): the rule of changrad_chunks (one operand instead of two changes nothing in it):
    B * nchunk * (tiles of 256 channels) workgroups near _GN_TARGET, a chunk no shorter than 16 pixels per pixel row of a
    workgroup, and every chunk non-empty"""
    return changrad_chunks(B, HW, Cc)


def _actreg_kind(who: str, kind: str, threshold: float) -> int:
    if kind not in ACTREG_KINDS:
        raise ValueError(f"{who}: kind {kind!r} is not one of {ACTREG_KINDS}")
    t = float(threshold)
    if not (t > 0.0 and t < float("inf")):
        raise ValueError(f"{who}: threshold {threshold!r} is not a finite number > 0")
    return ACTREG_KINDS.index(kind)


def _actreg_act(who: str, name: str, t: torch.Tensor):
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16):
        what = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{who}: {name}: expected a 4-D NHWC fp32 / bf16 CUDA tensor, got {what}")


def actreg_stats(a: torch.Tensor, kind: str, threshold: float, weight: float, mask: Optional[torch.Tensor] = None,
                 grad_scale: float = 1.0):
    """statistics of an activation penalty (vaehip.actreg.ActivationPenalty) on a module output `a` in one read of it:
    (sums float64 [3, C], pen float64 [C], coef fp32 [C]) on the device.  sums[0] = sum relu(|a| - threshold)^2, sums[1] =
    sum |a|, sums[2] = the number of elements over the threshold (a NaN counts), each per channel over the N = B * H * W pixel
    rows.  pen[c] is the channel's share of the penalty P, pen.sum() is P:
        ceiling: P = weight / (N C) sum_c w_c sum relu(|a| - threshold)^2
        floor:   P = weight / C sum_c w_c relu(threshold - m_c)^2, m_c = sums[1, c] / N
    coef[c] = k_c with dP/da * grad_scale = k_c psi(a), what actreg_inject adds to a gradient.  mask: fp32 [C] of w_c (0 or 1),
    None for all ones; weight * w_c == 0 gives pen and coef exactly 0.  a: 4-D NHWC fp32 or bf16, channels contiguous, pixel
    stride >= C (a channel-prefix view is read in place).  The threshold is compared in fp32; differences and squares are rounded
    once and summed in fp32 inside a workgroup (csrc/actreg.hip), everything after is float64 in a fixed order: two calls agree
    bitwise.  Nothing synchronises the host."""
    k = _actreg_kind("actreg_stats", kind, threshold)
    _actreg_act("actreg_stats", "a", a)
    w = float(weight)
    if not (w >= 0.0 and w < float("inf")):
        raise ValueError(f"actreg_stats: weight {weight!r} is not a finite number >= 0")
    gs = float(grad_scale)
    if not abs(gs) < float("inf"):
        raise ValueError(f"actreg_stats: grad_scale {grad_scale!r} is not finite")
    lda = _nhwc_ld("actreg_stats", a)
    B, H, W, Cc = a.shape
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.float32 or mask.device != a.device
                             or tuple(mask.shape) != (Cc,) or not mask.is_contiguous()):
        what = f"{tuple(mask.shape)} {mask.dtype} on {mask.device}" if isinstance(mask, torch.Tensor) else type(mask).__name__
        raise ValueError(f"actreg_stats: mask: expected a contiguous fp32 [{Cc}] tensor on {a.device}, got {what}")
    HW = H * W
    nch = actreg_chunks(B, HW, Cc)
    dev = a.device
    n = C.c_int64(0)
    lib.call("vae_actreg_workspace", B, HW, Cc, nch, C.byref(n))
    ws = torch.empty((n.value,), device=dev, dtype=torch.int32)
    sums = torch.empty((3, Cc), device=dev, dtype=torch.float64)
    pen = torch.empty((Cc,), device=dev, dtype=torch.float64)
    coef = torch.empty((Cc,), device=dev, dtype=torch.float32)
    lib.call("vae_actreg_partial", _p(a), _b16(a), lda, B, HW, Cc, nch, float(threshold), _p(ws), _stream())
    lib.call("vae_actreg_final", _p(ws), B, HW, Cc, nch, k, float(threshold), w, _p(mask), gs, _p(sums), _p(pen), _p(coef), _stream())
    return sums, pen, coef


def actreg_inject(a: torch.Tensor, g: torch.Tensor, kind: str, threshold: float, coef: torch.Tensor) -> torch.Tensor:
    """g + coef[c] * psi(a) as a new contiguous tensor with the dtype of g: the gradient of an activation penalty added to the
    gradient g of a module output a.  psi(a) = a - clamp(a, -threshold, threshold) for the ceiling, sign(a) for the floor
    (sign(0) = 0); coef = actreg_stats(...)[2].  a and g: 4-D NHWC of one shape, each fp32 or bf16, each with its own pixel
    stride.  fp32 arithmetic, the product and the sum rounded once each (a bf16 result once more); where the product is zero the
    element of g is passed on bit for bit (a zero coefficient leaves g as it is wherever a is finite; a non-finite a makes its own
    element NaN).  Nothing synchronises the host."""
    k = _actreg_kind("actreg_inject", kind, threshold)
    _actreg_act("actreg_inject", "a", a)
    _actreg_act("actreg_inject", "g", g)
    if tuple(a.shape) != tuple(g.shape) or a.device != g.device:
        raise ValueError(f"actreg_inject: output {tuple(a.shape)} on {a.device} and gradient {tuple(g.shape)} on {g.device} differ")
    lda, ldg = _nhwc_ld("actreg_inject", a), _nhwc_ld("actreg_inject", g)
    B, H, W, Cc = a.shape
    if (not isinstance(coef, torch.Tensor) or coef.dtype != torch.float32 or coef.device != a.device or tuple(coef.shape) != (Cc,)
            or not coef.is_contiguous()):
        what = f"{tuple(coef.shape)} {coef.dtype} on {coef.device}" if isinstance(coef, torch.Tensor) else type(coef).__name__
        raise ValueError(f"actreg_inject: coef: expected a contiguous fp32 [{Cc}] tensor on {a.device}, got {what}")
    out = torch.empty((B, H, W, Cc), device=a.device, dtype=g.dtype)
    lib.call("vae_actreg_inject", _p(a), _b16(a), lda, _p(g), _b16(g), ldg, _p(coef), B * H * W, Cc, k, float(threshold), _p(out),
             _stream())
    return out


CHANCOV_WS_BYTES = 64 << 20  # ceiling of chancov()'s workspace


def chancov_chunks(B: int, HW: int, Cc: int, tile: int = 128) -> int:
    """pixel chunks per image of chancov(): B * nchunk * (tile pairs of the upper triangle) workgroups near _GN_TARGET, a chunk
    no shorter than one 32-pixel step, the workspace (per (image, chunk): one fp32 tile^2 per pair and one float64 row per
    tile) at most CHANCOV_WS_BYTES -- unless one chunk per image already exceeds it -- and every chunk non-empty"""
    tiles = (Cc + tile - 1) // tile
    pairs = tiles * (tiles + 1) // 2
    row_bytes = 4 * (pairs * tile * tile + 2 * tiles * tile)
    nch = max(1, min(_GN_TARGET // max(B * pairs, 1), HW // 32, CHANCOV_WS_BYTES // (B * row_bytes)))
    per = (HW + nch - 1) // nch
    return (HW + per - 1) // per


def chancov(x: torch.Tensor, stats: Optional[Stats] = None, xf: int = XF_NONE):
    """channel covariance and mean of y = XF(x) over batch and pixels in one read of x, no tensor materialised: (cov float64
    [C, C], mean float64 [C]) on the device.  cov is unbiased (N - 1, N = B * H * W), bitwise symmetric, and exactly 0 in the
    row, column and variance of a constant channel; sums are taken of y minus the tensor's first pixel row, so a mean far above
    sigma costs no digits; products are split-bf16 on the matrix pipe (csrc/chancov.hip), the merge is float64 in a fixed order:
    two calls agree bitwise.  x, stats and xf as in moments().  The workspace rule is chancov_chunks(): at most 64 MB at every
    shape of the shipped model (tools/launch_shapes.py).  Nothing synchronises the host."""
    B, HW, Cc, ld, scale, shift = _stat_operand("chancov", x, stats, xf)
    if B * HW < 2:
        raise ValueError(f"chancov: a covariance needs at least two rows, got B * H * W = {B * HW}")
    nch = chancov_chunks(B, HW, Cc)
    dev = x.device
    n = C.c_int64(0)
    lib.call("vae_chancov_workspace", B, HW, Cc, nch, C.byref(n))
    ws = torch.empty((n.value,), device=dev, dtype=torch.float32)
    cov = torch.empty((Cc, Cc), device=dev, dtype=torch.float64)
    mean = torch.empty((Cc,), device=dev, dtype=torch.float64)
    lib.call("vae_chancov_partial", _p(x), _b16(x), _p(scale), _p(shift), xf, B, HW, Cc, ld, nch, _p(ws), _stream())
    lib.call("vae_chancov_final", _p(ws), B, HW, Cc, nch, _p(cov), _p(mean), _stream())
    return cov, mean


def image_metrics(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """per-image quality metrics of `pred` against `target` (evaluate.py's Average MSE / PSNR / SSIM) in one read of both: a
    float64 device tensor [B, 3] = [sum (pred - target)^2, sum (u(pred) - u(target))^2 with u(x) = clamp((x + 1) / 2, 0, 1),
    mean SSIM of u(pred) against u(target) (11 x 11 gaussian, sigma 1.5, border-cropped)].  Both are fp32 (B, C, H, W) tensors
    with any strides (NCHW, a channels-last view, a batch slice: read in place, no copy); nothing synchronises the host."""
    if pred.dim() != 4 or tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"image_metrics: expected two (B, C, H, W) tensors of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"image_metrics: expected float32 tensors, got {pred.dtype} and {target.dtype}")
    if not (pred.is_cuda and target.is_cuda and pred.device == target.device):
        raise ValueError(f"image_metrics: expected two tensors on one GPU, got {pred.device} and {target.device}")
    B, Cc, H, W = pred.shape
    if B < 1 or Cc < 1 or H < 11 or W < 11:
        raise ValueError(f"image_metrics: {tuple(pred.shape)}: needs B >= 1, C >= 1 and images of at least 11 x 11 (the SSIM window)")
    n = C.c_int64(0)
    lib.call("vae_image_metrics_workspace", B, Cc, H, W, C.byref(n))
    ws = torch.empty((n.value,), device=pred.device, dtype=torch.float64)
    out = torch.empty((B, 3), device=pred.device, dtype=torch.float64)
    lib.call("vae_image_metrics_partial", _p(pred), *pred.stride(), _p(target), *target.stride(), B, Cc, H, W, _p(ws), _stream())
    lib.call("vae_image_metrics_final", _p(ws), B, Cc, H, W, _p(out), _stream())
    return out


def _lens_operands(who: str, x: torch.Tensor, samples: int, channels: torch.Tensor, channels_host):
    """shape / stride checks shared by the logit-lens wrappers -> the leading arguments of their entry points, K, and the
    host list (kept alive by the caller until the call returns)"""
    if x.dim() != 4 or not x.is_cuda or x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{who}: expected a 4-D NHWC fp32 / bf16 CUDA tensor, got {tuple(x.shape)} {x.dtype} on {x.device}")
    B, H, W, Cc = x.shape
    ld = x.stride(2)
    if x.stride(3) != 1 or ld < Cc or x.stride(1) != W * ld or x.stride(0) != H * W * ld:
        raise ValueError(f"{who}: expected NHWC rows with contiguous channels, strides {x.stride()}")
    if not (isinstance(channels, torch.Tensor) and channels.dim() == 1 and channels.dtype == torch.int32 and channels.is_contiguous()
            and channels.device == x.device):
        raise ValueError(f"{who}: channels must be a contiguous 1-D int32 tensor on {x.device}")
    K = channels.numel()
    samples = int(samples)
    if B < 1 or H < 1 or W < 1 or Cc < 1 or K < 1 or not 1 <= samples <= B:
        raise ValueError(f"{who}: {tuple(x.shape)} with {samples} samples and {K} channels: needs 1 <= samples <= B, at least one "
                         f"channel and a non-empty map")
    host = None
    if channels_host is not None:
        idx = [int(c) for c in channels_host]
        if len(idx) != K:
            raise ValueError(f"{who}: channels_host has {len(idx)} entries, channels {K}")
        if any(not 0 <= c < Cc for c in idx):
            raise ValueError(f"{who}: channel indices {idx} are not all inside [0, {Cc})")
        host = (C.c_int32 * K)(*idx)
    return (_p(x), _b16(x), B, H, W, Cc, ld, samples, _p(channels), host, K), (B, H, W, K, samples)


def lens_planes(x: torch.Tensor, samples: int, channels: torch.Tensor, channels_host=None):
    """the logit lens's channel maps of the first `samples` samples of x and the channels a device int32 list names, read in
    place: (maps [S, K, H, W] fp32 -- bf16 storage widened exactly --, range [S, K, 2] = per-plane min and max, norm
    [S, K, H, W] = (x - min) / (max - min), or 0 on a plane with max - min <= 1e-6).  x: NHWC, fp32 or bf16 storage, channels
    contiguous; a channel-prefix view of a wider buffer is read in place.  channels_host: the same indices as a host sequence,
    for the range check a device list cannot get (an index outside [0, C) reads zeros otherwise).  Non-finite values are
    outside the contract.  Nothing synchronises the host."""
    args, (B, H, W, K, S) = _lens_operands("lens_planes", x, samples, channels, channels_host)
    n = C.c_int64(0)
    lib.call("vae_lens_workspace", S, K, H, W, C.byref(n))
    dev = x.device
    ws = torch.empty((n.value,), device=dev, dtype=torch.float32)
    maps = torch.empty((S, K, H, W), device=dev, dtype=torch.float32)
    rng = torch.empty((S, K, 2), device=dev, dtype=torch.float32)
    norm = torch.empty((S, K, H, W), device=dev, dtype=torch.float32)
    lib.call("vae_lens_planes_partial", *args, _p(maps), _p(ws), _stream())
    lib.call("vae_lens_planes_final", _p(maps), _p(ws), S, K, H, W, _p(rng), _p(norm), _stream())
    return maps, rng, norm


def lens_project(x: torch.Tensor, samples: int, channels: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
                 b2: torch.Tensor, full_map: bool, channels_host=None) -> torch.Tensor:
    """the logit lens's mini-decoder Sigmoid(ConvT2(ReLU(ConvT1(.)))) (ConvTranspose2d k 3, stride 2, padding 1, output_padding 1;
    Cin -> 16 -> 3) on the same operand as lens_planes, in one launch with the hidden image in LDS: full_map False projects
    each listed channel on its own (w1 [1, 16, 3, 3]) -> [S, K, 4H, 4W, 3]; full_map True takes the listed channels as the input
    (w1 [K, 16, 3, 3]) -> [S, 4H, 4W, 3].  fp32, HWC.  Weights: torch's ConvTranspose2d layout, contiguous fp32 on x's device."""
    args, (B, H, W, K, S) = _lens_operands("lens_project", x, samples, channels, channels_host)
    cin = K if full_map else 1
    for t, shape, name in ((w1, (cin, 16, 3, 3), "w1"), (b1, (16,), "b1"), (w2, (16, 3, 3, 3), "w2"), (b2, (3,), "b2")):
        if not (t.device == x.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"lens_project: {name} must be a contiguous float32 tensor of shape {shape} on {x.device}, got "
                             f"{tuple(t.shape)} {t.dtype} on {t.device}")
    out = torch.empty((S, 4 * H, 4 * W, 3) if full_map else (S, K, 4 * H, 4 * W, 3), device=x.device, dtype=torch.float32)
    lib.call("vae_lens_project", *args, int(bool(full_map)), _p(w1), _p(b1), _p(w2), _p(b2), _p(out), _stream())
    return out


def map_snapshot(t: torch.Tensor) -> torch.Tensor:
    """fp32 NHWC device copy of an activation (full_activation_map): bf16 storage widened by vae_unpack_bf16"""
    if t.dtype == torch.bfloat16:
        return to_f32(t)
    return t.clone(memory_format=torch.contiguous_format)


def conv_track_buffer(M: int, Co: int, device) -> torch.Tensor:
    return torch.empty(((M + 127) // 128, Co), device=device, dtype=torch.float32)


def track_final(ws: torch.Tensor, count: int) -> torch.Tensor:
    rows, Cc = ws.shape
    out = torch.empty((Cc,), device=ws.device, dtype=torch.float32)
    lib.call("vae_track_final", _p(ws), rows, Cc, 1.0 / float(count), _p(out), _stream())
    return out


def gn_bwd(x: torch.Tensor, g: torch.Tensor, st: Stats, gamma: torch.Tensor, beta: torch.Tensor, silu: bool,
           add: Optional[torch.Tensor], dgamma: torch.Tensor, dbeta: torch.Tensor, G: int = GN_GROUPS,
           want32: bool = True, want16: bool = False) -> torch.Tensor:
    """x: the GroupNorm input as stored (fp32 or bf16); g: fp32 or bf16; add (the residual-path gradient) is brought to x's
    storage.  Returns dx as fp32 (want32; with the bf16 image attached as `_b16` when want16 too) or as a bf16 tensor alone
    (want16 only: bf16 storage mode, or a gradient that feeds bf16 convolution kernels and nothing else)."""
    _chk_act(x, "gn_bwd.x")
    g16 = g.dtype == torch.bfloat16
    _chk_act(g, "gn_bwd.g")
    assert g.shape == x.shape and (add is None or add.shape == x.shape) and (want32 or want16)
    if add is not None:
        add = _like(add.contiguous(), x.dtype == torch.bfloat16)
    B, H, W, Cc = x.shape
    HW = H * W
    dev = x.device
    coef = torch.empty((B, G, 2), device=dev, dtype=torch.float32)
    dx = torch.empty(x.shape, device=dev, dtype=torch.float32) if want32 else None
    dx16 = torch.empty(x.shape, device=dev, dtype=torch.bfloat16) if want16 else None
    s = _stream()
    fused = getattr(g, "_gnb", None)  # the dgrad that produced g left the first pass's sums (conv_dgrad(gnb=...))
    if fused is not None and fused[2] == _gnb_key(x, st, gamma, beta, silu):
        ws, nch = fused[0], fused[1]
    else:
        nch = _gn_nchunk(B, HW, Cc)
        ws = torch.empty((B, nch, Cc, 2), device=dev, dtype=torch.float32)
        lib.call("vae_gn_bwd_partial", _p(x), _b16(x), _p(g), _p(st.mean), _p(st.rstd), _p(gamma), _p(beta), B, HW, Cc, G, nch,
                 int(silu), int(g16), _p(ws), s)
    lib.call("vae_gn_bwd_final", _p(ws), _p(st.rstd), _p(gamma), B, HW, Cc, G, nch, _p(dgamma), _p(dbeta), _p(coef), s)
    lib.call("vae_gn_bwd_apply", _p(x), _b16(x), _p(g), _p(st.mean), _p(st.rstd), _p(gamma), _p(beta), _p(coef), _p(add), B, HW,
             Cc, G, int(silu), int(g16), _p(dx), _p(dx16), s)
    if dx is None:
        return dx16
    if dx16 is not None:
        dx._b16 = dx16
    return dx


# ------------------------------------------------------------------ batched GEMMs (attention)
def _gemm_rows(A: torch.Tensor, Bm: torch.Tensor, N: int, bkm: bool, alpha: float) -> torch.Tensor:
    z, M, K = A.shape
    out = torch.empty((z, M, N), device=A.device, dtype=torch.float32)
    a = gemm_rows_args(M, N, K, bkm, alpha, z)
    a.A, a.W, a.C = _p(A), _p(Bm), _p(out)
    _launch_igemm(a)
    return out


def gemm_nt(A: torch.Tensor, Bm: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """out[z] = alpha * A[z] @ Bm[z]^T ; A [z,M,K], Bm [z,N,K]."""
    return _gemm_rows(A, Bm, Bm.shape[1], False, alpha)


def gemm_nn(A: torch.Tensor, Bm: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """out[z] = alpha * A[z] @ Bm[z] ; A [z,M,K], Bm [z,K,N]."""
    return _gemm_rows(A, Bm, Bm.shape[2], True, alpha)


def gemm_tn(A: torch.Tensor, Bm: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """out[z] = alpha * A[z]^T @ Bm[z] ; A [z,K,M], Bm [z,K,N]."""
    z, K, M = A.shape
    N = Bm.shape[2]
    out = torch.empty((z, M, N), device=A.device, dtype=torch.float32)
    a = gemm_tn_args(M, N, K, alpha, z)
    a.dY, a.X, a.out = _p(A), _p(Bm), _p(out)
    _launch_wgrad(a)
    return out


# ------------------------------------------------------------------ blockwise attention (no T x T tensor)
# sequences of at least this many tokens run the blockwise kernels (R >= 512: T >= 4096); shorter ones keep the
# materialised scores, which are small there (T = 1024: 4 MB per image).  Tests lower it to compare the two paths.
ATTN_BLOCKWISE_MIN_T = 4096
ATTN_CALLS = {"blockwise_fwd": 0, "blockwise_bwd": 0, "materialised_fwd": 0}


def attn_blockwise_ok(T: int, Cc: int) -> bool:
    return T >= ATTN_BLOCKWISE_MIN_T and bool(lib.query("vae_attn_supported", int(T), int(Cc)))


def _attn_operand(t: torch.Tensor) -> torch.Tensor:
    """operand of the attention kernels in the arithmetic's precision: the fp32 tensor itself, or its bf16 image"""
    if PRECISION != PREC_BF16:
        return t
    return pack_bf16(t, torch.empty(t.shape, device=t.device, dtype=torch.bfloat16))


def attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float):
    """q, k, v [B,T,C] fp32 -> (o [B,T,C] fp32, saved = operands + row log-sum-exp for attn_bwd)"""
    B, T, Cc = q.shape
    for t in (q, k, v):
        _chk_c(t, "attn_fwd")
    qe, ke, ve = _attn_operand(q), _attn_operand(k), _attn_operand(v)
    o = torch.empty_like(q)
    lse = torch.empty((B, T), device=q.device, dtype=torch.float32)
    fl = 4.0 * B * T * T * Cc  # Q K^T and P V
    _timed(f"attn_fwd_kernel<{'bf16' if PRECISION == PREC_BF16 else 'f32'}>", fl, fl, "vae_attn_fwd", _p(qe), _p(ke), _p(ve), B, T, Cc,
           float(scale), PRECISION, _p(o), _p(lse), _stream())
    ATTN_CALLS["blockwise_fwd"] += 1
    return o, (qe, ke, ve, lse, PRECISION)


def attn_bwd(saved, o: torch.Tensor, do: torch.Tensor, scale: float):
    """-> dq, dk, dv [B,T,C] fp32; P is recomputed blockwise from the saved log-sum-exp"""
    qe, ke, ve, lse, prec = saved
    B, T, Cc = o.shape
    _chk_c(do, "attn_bwd.do")
    with precision(prec):
        doe = _attn_operand(do)
    dq, dk, dv = torch.empty_like(o), torch.empty_like(o), torch.empty_like(o)
    dsum = torch.empty((B, T), device=o.device, dtype=torch.float32)
    # algorithmic: dP, dV, dQ, dK and one recomputation of S = 10 T^2 d; executed: S is recomputed in each of the 3 launches
    _timed(f"attn_bwd_kernels<{'bf16' if prec == PREC_BF16 else 'f32'}>", 10.0 * B * T * T * Cc, 16.0 * B * T * T * Cc, "vae_attn_bwd",
           _p(qe), _p(ke), _p(ve), _p(doe), _p(o), _p(do), _p(lse), B, T, Cc, float(scale), prec,
           _p(dq), _p(dk), _p(dv), _p(dsum), _stream())
    ATTN_CALLS["blockwise_bwd"] += 1
    return dq, dk, dv


def softmax_rows_(S: torch.Tensor):
    cols = S.shape[-1]
    lib.call("vae_softmax_rows", _p(S), S.numel() // cols, cols, _stream())
    return S


def softmax_bwd_rows_(P: torch.Tensor, dP: torch.Tensor):
    cols = P.shape[-1]
    lib.call("vae_softmax_bwd_rows", _p(P), _p(dP), P.numel() // cols, cols, _stream())
    return dP


# ------------------------------------------------------------------ loss / sample / layout / optimizer
def nchw_to_nhwc(x: torch.Tensor, cpad: Optional[int] = None) -> torch.Tensor:
    _chk_c(x, "nchw_to_nhwc")
    B, Cc, H, W = x.shape
    cp = cpad or Cc
    out = torch.empty((B, H, W, cp), device=x.device, dtype=torch.float32)
    lib.call("vae_nchw_to_nhwc", _p(x), B, Cc, H * W, cp, _p(out), _stream())
    return out


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    _chk_c(x, "nhwc_to_nchw")
    B, H, W, Cc = x.shape
    out = torch.empty((B, Cc, H, W), device=x.device, dtype=torch.float32)
    lib.call("vae_nhwc_to_nchw", _p(x), B, Cc, H * W, _p(out), _stream())
    return out


def sample_kl(moments: torch.Tensor, eps: Optional[torch.Tensor]):
    """moments [B,h,w,2L], eps [B,h,w,L] or None (mode) -> z [B,h,w,L], kl_partial [B,nblk]."""
    _chk_c(moments, "sample_kl.moments")
    B, h, w, L2 = moments.shape
    L = L2 // 2
    nblk = (h * w * L + 255) // 256
    z = torch.empty((B, h, w, L), device=moments.device, dtype=torch.float32)
    klp = torch.empty((B, nblk), device=moments.device, dtype=torch.float32)
    lib.call("vae_sample_kl", _p(moments), _p(eps), B, h * w, L, _p(z), _p(klp), _stream())
    return z, klp


def sample_kl_bwd(moments, eps, dz, kl_weight: float):
    B, h, w, L2 = moments.shape
    L = L2 // 2
    dm = torch.empty_like(moments)
    lib.call("vae_sample_kl_bwd", _p(moments), _p(eps), _p(dz), B, h * w, L, float(kl_weight), _p(dm), _stream())
    return dm


def mse_kl_loss(recon: torch.Tensor, target: torch.Tensor, kl_partial: torch.Tensor, kl_weight: float) -> torch.Tensor:
    """-> device scalars [mse_mean, kl_mean, total] (train.py:289-291)."""
    n = recon.numel()
    nblk = max(1, min(1024, (n + 4095) // 4096))
    ws = torch.empty((nblk,), device=recon.device, dtype=torch.float32)
    sc = torch.empty((3,), device=recon.device, dtype=torch.float32)
    s = _stream()
    lib.call("vae_mse_partial", _p(recon), _p(target), n, _p(ws), nblk, s)
    B, kb = kl_partial.shape
    lib.call("vae_loss_final", _p(ws), nblk, n, _p(kl_partial), B, kb, float(kl_weight), _p(sc), s)
    return sc


def mse_bwd(recon: torch.Tensor, target: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    d = torch.empty_like(recon)
    lib.call("vae_mse_bwd", _p(recon), _p(target), recon.numel(), float(scale), _p(d), _stream())
    return d


def ssim_tile():
    """(rows, columns) of the tile one workgroup of the SSIM kernels covers (window positions forward, pixels backward)"""
    return lib.query("vae_ssim_tile", 0), lib.query("vae_ssim_tile", 1)


def _ssim_pair(who: str, pred: torch.Tensor, target: torch.Tensor):
    """checks of a (B, C, H, W) fp32 pair for the SSIM kernels (any strides), before anything is allocated"""
    if pred.dim() != 4 or tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"{who}: expected two (B, C, H, W) tensors of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"{who}: expected float32 tensors, got {pred.dtype} and {target.dtype}")
    if not (pred.is_cuda and target.is_cuda and pred.device == target.device):
        raise ValueError(f"{who}: expected two tensors on one GPU, got {pred.device} and {target.device}")
    B, Cc, H, W = pred.shape
    if B < 1 or Cc < 1 or H < 11 or W < 11:
        raise ValueError(f"{who}: {tuple(pred.shape)}: needs B >= 1, C >= 1 and images of at least 11 x 11 (the SSIM window)")
    npart, nmaps = C.c_int64(0), C.c_int64(0)
    lib.call("vae_ssim_workspace", B, Cc, H, W, C.byref(npart), C.byref(nmaps))
    return B, Cc, H, W, npart.value, nmaps.value


def ssim_index(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """float64 [B]: per image the mean SSIM index of (pred + 1) / 2 against (target + 1) / 2, NOT clamped (the training term of
    vaehip.losses; image_metrics clamps), 11 x 11 gaussian window, positions wholly inside the image.  fp32 (B, C, H, W) tensors
    with any strides, read in place; float64 throughout; nothing synchronises the host."""
    B, Cc, H, W, npart, _ = _ssim_pair("ssim_index", pred, target)
    part = torch.empty((npart,), device=pred.device, dtype=torch.float64)
    out = torch.empty((B,), device=pred.device, dtype=torch.float64)
    lib.call("vae_ssim_fwd", _p(pred), *pred.stride(), _p(target), *target.stride(), B, Cc, H, W, _p(part), None, _stream())
    lib.call("vae_ssim_index", _p(part), B, Cc, H, W, _p(out), _stream())
    return out


def recon_loss(recon: torch.Tensor, target: torch.Tensor, kl_partial: torch.Tensor, kl_weight: float, spec, grad_scale: float = 1.0,
               want_grad: bool = True, layout: str = "nhwc"):
    """the reconstruction loss `spec` (vaehip.losses.ReconLoss) of two contiguous fp32 tensors of one shape, with the KL partials
    of sample_kl -> (scalars [3] = rec, kl, total; terms [2] = pixel term, SSIM index (NaN without an SSIM term);
    drecon = grad_scale * d rec / d recon, or None when want_grad is False).  With an SSIM term the tensors are 4-D images,
    [B, H, W, C] as the engine holds them (layout "nhwc") or [B, C, H, W] ("nchw").  csrc/recon_loss.hip: float64 sums, no atomics."""
    if tuple(recon.shape) != tuple(target.shape) or recon.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"recon_loss: expected two float32 tensors of one shape, got {tuple(recon.shape)} {recon.dtype} and "
                         f"{tuple(target.shape)} {target.dtype}")
    if not (recon.is_cuda and target.is_cuda and recon.device == target.device and kl_partial.device == recon.device):
        raise ValueError(f"recon_loss: expected tensors on one GPU, got {recon.device}, {target.device} and {kl_partial.device}")
    if not (recon.is_contiguous() and target.is_contiguous()) or recon.numel() < 1:
        raise ValueError("recon_loss: expected contiguous, non-empty tensors")
    if kl_partial.dim() != 2 or kl_partial.dtype != torch.float32 or not kl_partial.is_contiguous() or kl_partial.numel() < 1:
        raise ValueError(f"recon_loss: kl_partial must be a contiguous float32 [B, blocks] tensor, got {tuple(kl_partial.shape)}")
    if layout not in ("nhwc", "nchw"):
        raise ValueError(f"recon_loss: layout {layout!r}: expected 'nhwc' or 'nchw'")
    n = recon.numel()
    B, kb = kl_partial.shape
    dev = recon.device
    ssim = spec.ssim_weight > 0.0
    if ssim:
        if recon.dim() != 4 or recon.shape[0] != B:
            raise ValueError(f"recon_loss: an SSIM term needs 4-D images with the batch of kl_partial ({B}), got {tuple(recon.shape)}")
        pv, tv = (recon.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)) if layout == "nhwc" else (recon, target)
        _, Cc, H, W, npart, nmaps = _ssim_pair("recon_loss", pv, tv)
    s = _stream()
    part = torch.empty((lib.query("vae_pixel_loss_blocks", n),), device=dev, dtype=torch.float64)
    d = torch.empty_like(recon) if want_grad else None
    sc = torch.empty((3,), device=dev, dtype=torch.float32)
    terms = torch.empty((2,), device=dev, dtype=torch.float32)
    _timed("pixel_loss_kernel", 0.0, 0.0, "vae_pixel_loss", _p(recon), _p(target), n, spec.kind_id, float(spec.huber_delta),
           float(grad_scale), _p(part), _p(d), s)
    spart = None
    if ssim:
        spart = torch.empty((npart,), device=dev, dtype=torch.float64)
        maps = torch.empty((nmaps,), device=dev, dtype=torch.float64) if want_grad else None
        _timed("ssim_fwd_kernel", 0.0, 0.0, "vae_ssim_fwd", _p(pv), *pv.stride(), _p(tv), *tv.stride(), B, Cc, H, W, _p(spart),
               _p(maps), s)
        if want_grad:
            dv = d.permute(0, 3, 1, 2) if layout == "nhwc" else d
            _timed("ssim_bwd_kernel", 0.0, 0.0, "vae_ssim_bwd", _p(pv), *pv.stride(), _p(tv), *tv.stride(), _p(maps), B, Cc, H, W,
                   float(grad_scale) * float(spec.ssim_weight), _p(dv), *dv.stride(), s)
    else:
        Cc = H = W = 0
    _timed("recon_final_kernel", 0.0, 0.0, "vae_recon_loss_final", _p(part), n, _p(spart), B, Cc, H, W, float(spec.ssim_weight),
           _p(kl_partial), kb, float(kl_weight), _p(sc), _p(terms), s)
    return sc, terms, d


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a + b; two bf16 tensors (or a mixed pair, brought to bf16) give a bf16 sum rounded once from the fp32 sum"""
    if a.dtype == torch.bfloat16 or b.dtype == torch.bfloat16:
        a, b = to_bf16(a), to_bf16(b)
        o = torch.empty_like(a)
        lib.call("vae_add_bf16", _p(a), _p(b), a.numel(), _p(o), _stream())
        return o
    o = torch.empty_like(a)
    lib.call("vae_add", _p(a), _p(b), a.numel(), _p(o), _stream())
    return o


def sqnorm(g: torch.Tensor, out: torch.Tensor, ws: Optional[torch.Tensor] = None):
    n = g.numel()
    nblk = 2048
    if ws is None:
        ws = torch.empty((nblk,), device=g.device, dtype=torch.float32)
    lib.call("vae_sqnorm", _p(g), n, _p(ws), nblk, _p(out), _stream())
    return out


def adamw(p, g, m, v, sqn: Optional[torch.Tensor], max_norm: float, lr: float, beta1: float, beta2: float, eps: float,
          wd: float, step: int):
    lib.call("vae_adamw", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(sqn), float(max_norm), float(lr), float(beta1),
             float(beta2), float(eps), float(wd), int(step), _stream())


def adamw_ema(p, g, m, v, e, sqn: Optional[torch.Tensor], max_norm: float, lr: float, beta1: float, beta2: float, eps: float,
              wd: float, step: int, ema_decay: float):
    """adamw plus e <- e + (1 - ema_decay) (p' - e) in the same pass (ema_decay == 0: e <- p')"""
    lib.call("vae_adamw_ema", _p(p), _p(g), _p(m), _p(v), _p(e), p.numel(), _p(sqn), float(max_norm), float(lr), float(beta1),
             float(beta2), float(eps), float(wd), int(step), float(ema_decay), _stream())


def sqnorm_ranges(g: torch.Tensor, table, out: torch.Tensor):
    """sum of g*g over the ranges of `table` (a trainable.RangeTable, which checked them when it was built; nothing is checked
    here) -> out[0]; nothing outside them is read"""
    lib.call("vae_sqnorm_ranges", _p(g), _p(table.seg_off), _p(table.seg_chunk0), table.nseg, table.nchunk, _p(table.ws), _p(out),
             _stream())
    return out


def adamw_ranges(p, g, m, v, e: Optional[torch.Tensor], table, sqn: Optional[torch.Tensor], max_norm: float, lr: float,
                 beta1: float, beta2: float, eps: float, wd: float, step: int, ema_decay: float = 0.0):
    """adamw (e None) / adamw_ema on the elements of the table's ranges; everything else is neither read nor written"""
    lib.call("vae_adamw_ranges", _p(p), _p(g), _p(m), _p(v), _p(e), _p(table.seg_off), _p(table.seg_chunk0), table.nseg, table.nchunk,
             _p(sqn), float(max_norm), float(lr), float(beta1), float(beta2), float(eps), float(wd), int(step), float(ema_decay),
             _stream())


def weight_dynamics(flat: torch.Tensor, grad: Optional[torch.Tensor], exp_avg: Optional[torch.Tensor],
                    exp_avg_sq: Optional[torch.Tensor], table, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                    step: int = 1):
    """per output slice and per input slice of every tensor of `table` (a weight_table.WeightTable, which checked itself when it
    was built), in one read of the four flat fp32 arenas: raw (out_sums float64 [n_out, 6], in_sums float64 [n_in, 6], out_absmax
    fp32 [n_out], in_absmax fp32 [n_in]) on the device.  The six sums are S_ww, S_gg, S_wg, S_mm, S_gm, S_uu with
    u = (m / bc1) / (sqrt(v) / bc2_sqrt + eps) the Adam direction after `step` updates; the maxima are max |w| (NaN if the slice
    holds one).  grad None, or exp_avg and exp_avg_sq None, are the modes w and w+g: the sums they cannot form come out NaN.
    fp32 in one fixed order inside a workgroup (csrc/wdyn.hip), float64 in chunk order after it: two calls agree bitwise.
    Nothing synchronises the host, no arena is written."""
    if (exp_avg is None) != (exp_avg_sq is None) or (exp_avg is not None and grad is None):
        raise ValueError("weight_dynamics: the modes are w, w+g and w+g+m+v")
    for name, t in (("flat", flat), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if t is None:
            continue
        if t.dim() != 1 or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.device != flat.device:
            raise ValueError(f"weight_dynamics: {name} must be a flat contiguous fp32 CUDA tensor on one device, got "
                             f"{tuple(t.shape)} {t.dtype} on {t.device}")
        if t.numel() < table.extent:
            raise ValueError(f"weight_dynamics: {name} holds {t.numel()} elements, the table reaches {table.extent}")
        if t.data_ptr() % 16:
            raise ValueError(f"weight_dynamics: {name} is not 16-byte aligned")
    if table.tab.device != flat.device:
        raise ValueError(f"weight_dynamics: the table lives on {table.tab.device}, the arenas on {flat.device}")
    if exp_avg is not None and int(step) < 1:
        raise ValueError(f"weight_dynamics: step {step} with Adam moments (the bias corrections need step >= 1)")
    mode = 2 if exp_avg is not None else (1 if grad is not None else 0)
    dev = flat.device
    # everything is checked: allocate
    ws = torch.empty((max(table.nwords, 4),), device=dev, dtype=torch.int32)
    out_sums = torch.empty((table.n_out, 6), device=dev, dtype=torch.float64)
    out_absmax = torch.empty((table.n_out,), device=dev, dtype=torch.float32)
    in_sums = torch.empty((table.n_in, 6), device=dev, dtype=torch.float64)
    in_absmax = torch.empty((table.n_in,), device=dev, dtype=torch.float32)
    lib.call("vae_wdyn_partial", _p(flat), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(table.tab), table.nseg, table.nchunk, table.n_out,
             float(beta1), float(beta2), float(eps), int(step), _p(ws), _p(out_sums), _p(out_absmax), _stream())
    if table.n_in:
        lib.call("vae_wdyn_final", _p(ws), _p(table.tab), table.nseg, table.n_in, mode, _p(in_sums), _p(in_absmax), _stream())
    return out_sums, in_sums, out_absmax, in_absmax
