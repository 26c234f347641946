"""A/B of two (or more) builds of the fp32 Winograd convolutions -- or, `--only bf16`, of the bf16 halo-tile family -- in one process: this build against the parent commit's
libvaehip.so (built in a scratch worktree; nothing of it is committed), further builds optional (a lever of
one kernel switched the other way, e.g. conv3_wino4.hip compiled with -DVAE_W4_SWAVE=0 and linked into another file).

Per case the operands are filled once; every library builds its own transformed weights (vae_wino_weights) and launches
vae_igemm_rows into its own output, `gstat` workspace and `gnb` workspace, which start as NaN and are compared with the FIRST
library's BIT FOR BIT, as is the transformed-weight image U itself.  Then the arms are timed alternately with device events
around the convolution launch alone (warm-up, `--launches` launches per arm, interleaved launch by launch, the arm that opens a
round rotating): median, quartiles and extremes per arm.

Cases: F(4x4) forward and dgrad of the plain 3x3 layers of the fp32 step (256^2, batch 16), each bare and with the epilogue it
runs with in the step (forward: bias + residual + GroupNorm moments; dgrad: GroupNorm(+SiLU)-backward sums); the small cases
of tests/test_wino4_seat_gpu.py (bitwise only); the upsampler convolutions (csrc/conv3_upwino.hip forward and dgrad,
csrc/wgrad3_upwino.hip through vae_wgrad_wino); the small forwards also with GroupNorm + SiLU fused into the staging (epilogue
"xf": XF_AFFINE_SILU + bias + residual + moments).  `--only wino2` runs the small cases and the F(2x2)-only shapes of the kernel
tests under the library option no_wino4 (set on every library), so that csrc/conv3_wino.hip serves them.

With a third library named parent2 (a second copy of the parent's file) the run derives its own noise floor: per kernel the margin
is twice the largest |median(parent2) / median(parent) - 1| over that kernel's timed cases, and `within_margin` says whether
the new build's median stays inside it on every case (exit status 2 if not; 1 if anything differs in a bit).

`--only bf16`: csrc/conv3_tile_bf16.hip, conv3_wide_bf16.hip and wgrad3_tile_bf16.hip at prec = PREC_BF16 through vae_igemm_rows /
vae_wgrad (weight image from each library's vae_pack_bf16, operand images tensor.bfloat16(), split count of vae_wgrad_plan unless
the case fixes one): outputs, `gstat` workspaces, slabs and bias partials bit for bit on the small cases (BF16_SMALL: every path the
shared header csrc/bf16_tile_common.h owns), which together must launch every instantiation the dispatcher can reach (exit status
1 otherwise); timed on the 3x3 layers of the bf16 step at 256^2, batch 32 (BF16_STEP).

`--only thin`: the six kernels of the <= 4-channel convolutions (csrc/skinny.hip, conv_thin_bf16.hip, wgrad_thin_bf16.hip; what they
share is csrc/thin_common.h).  The small cases are the tables of tests/thin_refs.py (ROWS_CASES, THIN_LARGE, WG_CASES: operands, argument
blocks and split counts as the tests build them): outputs, tracker buffers, slabs (the output itself with one split) and bias
partials bit for bit; together they must launch all 16 instantiations (exit status 1 otherwise).  Timed: every launch of one fp32
step (256^2, batch 16) and one bf16 step (256^2, batch 32) that one of these kernels serves (THIN_STEP, copied from the output of
tools/launch_shapes.py --flags).

`--only stream`: the streaming kernels (csrc/norm.hip, track.hip, lens.hip, image_metrics.hip, elementwise.hip; what they share is
csrc/stream_common.h).  Every launch goes through the package's loader with its library swapped per arm, so the small cases are the
tests' own: the tables of tests/norm_refs.py and tests/streaming_refs.py through the launch helpers of tests/test_norm_edges_gpu.py,
and the case lists of test_tracker_metrics_gpu.py, test_logit_lens_gpu.py, test_image_metrics_gpu.py and test_trainable_gpu.py.
Every tensor a case hands to the library (operands, results, workspaces; the helpers poison them) is compared bit for bit, and
together the cases must launch every instantiation of the five files (STREAM_NAMES, named from each call's own arguments; exit
status 1 otherwise).  Timed (--launches 0 skips it), one call of a C entry point per case on workspaces allocated beforehand: the GroupNorm entry
points at the step's four shapes, fp32 storage at batch 16 and bf16 storage at batch 32, over a ring of operands larger than the
memory-side cache, the moments passes, and the optimizer kernels, vae_sqnorm and the dead-weight scans at the arena's size; each case carries its own margin (twice |parent2 / parent - 1|, at least one rounding unit of the recorded medians).

`--only chanstat`: the per-channel statistics kernels (csrc/track.hip's moments, chanhist.hip, chancov.hip, changrad.hip, changroup.hip,
actreg.hip; what they share is csrc/chanstat_common.h), run like the streaming family.  A case is one call of an ops entry point
(moments, chanhist, changroup, chancov, changrad, actreg_stats, actreg_inject) at the frame's edge shapes (tests/chanhist_refs.py
FRAME_CASES) in every storage, transform and penalty kind; every tensor the call hands to the library -- operands, workspace,
results -- is compared with the first arm's.  The timed cases are the same calls on rings of step-sized operands.

usage: python tools/wino_seat_ab.py NEW.so PARENT.so [name=OTHER.so ...] [--launches 20] [--out FILE] [--only wino4|wino2|up|bf16|thin|stream|chanstat]"""
import argparse
import ctypes as C
import functools
import itertools
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vae-channel-dynamics_amd", "src"))
import torch  # noqa: E402
from vaehip import ops  # noqa: E402
from vaehip.lib import SIGNATURES, IgemmArgs, WgradArgs, lib  # noqa: E402

# kind, mode, B, H, W, Ci, Co, epilogue, timed      (H, W: the layer's forward input map)
STEP = [("c3", m, 16, hw, hw, ci, co, e, True) for ci, co, hw in [(128, 128, 256), (256, 128, 256), (256, 256, 128), (512, 256, 128), (512, 512, 64), (512, 512, 32)]
        for m in ("fwd", "dgrad") for e in (False, True)]
SMALL = ([("c3", "fwd", B, H, W, K, Co, False, False) for K in (64, 72, 80, 136) for B, H, W, Co in [(1, 16, 32, 64), (2, 32, 64, 128)]]
         + [("c3", "dgrad", B, H, W, 64, K, False, False) for K in (64, 72, 80, 136) for B, H, W in [(1, 16, 32), (2, 32, 64)]]
         + [("c3", "fwd", 1, 48, 96, 72, 64, False, False), ("c3", "dgrad", 1, 48, 96, 64, 72, False, False),
            ("c3", "fwd", 2, 32, 64, 128, 128, True, False), ("c3", "dgrad", 2, 16, 32, 128, 64, True, False),
            ("c3", "fwd", 2, 32, 64, 128, 128, "xf", False), ("c3", "fwd", 1, 16, 32, 72, 128, "xf", False)])
# under no_wino4: the small cases and the shapes only F(2x2) takes (partial 16 x 32 tiles, channel tails of 32 and 160)
WINO2 = SMALL + [("c3", m, B, H, W, Ci, Co, e, False) for B, H, W, Ci, Co in [(6, 16, 48, 128, 160), (2, 8, 16, 128, 32), (1, 48, 32, 256, 64)]
                 for m, e in (("fwd", False), ("dgrad", False), ("fwd", "xf")) if not (m == "dgrad" and Co < 64)]  # (K >= 64)
# ... and, timed, two layers of the step with the epilogues F(2x2) runs with (moments; GroupNorm-backward sums; fused GroupNorm + SiLU)
WINO2 += [("c3", m, 16, hw, hw, ci, co, e, True) for ci, co, hw in [(128, 128, 256), (512, 512, 64)]
          for m, e in (("fwd", True), ("dgrad", True), ("fwd", "xf"))]
UP = [("c3up", m, 16, hw, hw, ci, co, False, True) for ci, co, hw in [(512, 512, 32), (512, 512, 64), (256, 256, 128)] for m in ("fwd", "dgrad", "wgrad")]

# ---- the bf16 halo-tile family: ("bf16", form, B, H, W, Cin, Cout, knobs, timed).  Forms: fwd / dgrad of a "c3" layer, up2x (forward
# over the virtual upsample; its one-pass dgrad is a flat-kernel launch), phase_fwd / phase_dgrad (one phase convolution of an upsampler), wgrad of kind c3 / c3s2 /
# c3up, wgrad_phase.  Knobs: a16 / x16 / y16 operand as a bf16 image, xf, out16, res, gstat, nobias, pad (ldc = N + pad), ns (split
# count), opts (library options for the case).  (H, W: the layer's forward input map)
def _b(form, B, H, W, Ci, Co, timed=False, **knobs):
    return ("bf16", form, B, H, W, Ci, Co, knobs, timed)


_XF3 = (ops.XF_NONE, ops.XF_AFFINE, ops.XF_AFFINE_SILU)
BF16_SMALL = (
    # conv3_tile_bf16_kernel: a grid of 30 (no multiple of 8); 640 tiles on 512 workgroups; channel tails; both outputs; residual;
    # statistics at 4, 8, 16 channels per group; the three transforms; operand images; up2x; a tap-masked phase
    [_b("fwd", 1, 40, 96, 64, 128, xf=xf) for xf in _XF3] + [_b("up2x", 1, 20, 48, 64, 128, xf=xf) for xf in _XF3]
    + [_b("fwd", 5, 128, 128, 32, 128, xf=ops.XF_AFFINE_SILU, res=True, gstat=True), _b("fwd", 1, 40, 96, 72, 136, out16=True, res=True),
       _b("dgrad", 1, 40, 96, 136, 72), _b("dgrad", 1, 40, 96, 64, 128, a16=True, out16=True), _b("fwd", 1, 40, 96, 64, 128, a16=True, out16=True, nobias=True),
       _b("up2x", 1, 20, 48, 64, 128, a16=True), _b("phase_fwd", 1, 40, 96, 64, 128), _b("phase_dgrad", 1, 40, 96, 64, 128)]
    + [_b("fwd", 1, 8, 32, 32, Co, gstat=True, out16=o16, res=o16) for Co, o16 in ((128, False), (256, True), (512, False), (512, True))]
    # conv3_wide_bf16_kernel: 192 tiles (one per workgroup), 320 (one and two), a grid of 253; both directions; the epilogue variants
    + [_b("fwd", B, 64, 64, 64, 512, a16=True, out16=True, **kn) for B, kn in ((3, {}), (5, {}), (5, {"opts": {"wide_reserved_cus": 3}}), (3, {"pad": 2}))]
    + [_b("dgrad", B, 64, 64, 512, 64, a16=True, out16=True, **kn) for B, kn in ((3, {}), (5, {"opts": {"wide_reserved_cus": 3}}))]
    + [_b("fwd", 3, 64, 64, 256, 512, a16=True, out16=o16, res=True, gstat=gs) for o16, gs in ((False, False), (True, False), (True, True), (False, True))]
    + [_b("fwd", B, 64, 64, 64, Co, a16=True, out16=o16, gstat=True) for B, Co, o16 in ((12, 128, True), (6, 256, False), (6, 256, True))]
    + [_b("phase_fwd", 3, 64, 64, 64, 512, a16=True, out16=True), _b("phase_dgrad", 3, 64, 64, 512, 64, a16=True, out16=True)]
    # weight gradients: 0, 1, 2, 5 units per split; split counts that are and are not multiples of 8; a row tail; bias partials on
    # and off; up2x, stride 2, a tap-masked phase; the storage combinations and transforms of the register-staged kernel
    + [_b("wgrad", B, H, 32, 64, 128, x16=True, y16=True, ns=ns, nobias=nb) for B, H, ns, nb in ((1, 2, 2, False), (2, 2, 1, True), (1, 10, 1, False), (2, 8, 8, False), (2, 8, 3, True))]
    + [_b("wgrad", 2, 4, 32, 64, 136, x16=True, y16=True, ns=2), _b("wgrad_c3up", 2, 2, 16, 64, 128, x16=True, y16=True, ns=2),
       _b("wgrad_c3s2", 2, 8, 64, 64, 128, x16=True, y16=True, ns=3), _b("wgrad_phase", 2, 4, 32, 64, 128, x16=True, y16=True, ns=2)]
    + [_b(f, 2, 4, 32, 64, 136, x16=x16, y16=y16, xf=xf, ns=2, nobias=x16, opts={"no_wgrad_dma": 1}) for f in ("wgrad", "wgrad_c3up")
       for x16, xf in ((False, ops.XF_NONE), (True, ops.XF_NONE), (False, ops.XF_AFFINE), (False, ops.XF_AFFINE_SILU)) for y16 in (False, True)])
_STEP16 = [(128, 128, 256), (256, 128, 256), (256, 256, 128), (512, 256, 128), (512, 512, 64)]
BF16_STEP = ([_b(m, 32, hw, hw, ci, co, True, a16=True, out16=True, nobias=not e, res=e and m == "fwd", gstat=e and m == "fwd")
              for ci, co, hw in _STEP16 for m, e in (("fwd", False), ("fwd", True), ("dgrad", False))]
             + [_b("wgrad", 32, hw, hw, ci, co, True, x16=True, y16=True) for ci, co, hw in _STEP16]
             + [_b("wgrad_c3s2", 32, hw, hw, c, c, True, x16=True, y16=True) for c, hw in ((128, 256), (256, 128), (512, 64))]
             + [_b("wgrad_c3up", 32, 64, 64, 256, 256, True, x16=True, y16=True)])
# every instantiation of the three files that the dispatcher selects (conv3_tile_eligible refuses a fused transform on a dgrad)
TF = ("false", "true")
BF16_NAMES = ({f"conv3_tile_bf16_kernel<{TF[dg]},{TF[up]},{xf},{TF[i]}>" for dg, up in ((0, 0), (0, 1), (1, 0)) for xf, i in ((0, 0), (0, 1), (1, 0), (2, 0))
               if not (dg and xf)}
              | {f"conv3_wide_bf16_kernel<{TF[dg]},{ks}>" for dg in (0, 1) for ks in (2, 3)}
              | {f"wgrad3_tile_bf16_kernel<{TF[up]},{xf},{TF[x]},{TF[y]}>" for up in (0, 1) for xf, x in ((0, 0), (0, 1), (1, 0), (2, 0)) for y in (0, 1)}
              | {"wgrad3_dma_bf16_kernel<false,1>", "wgrad3_dma_bf16_kernel<false,2>", "wgrad3_dma_bf16_kernel<true,1>"})


def thin_cases():
    """-> (thin_refs, [("thin", id, B, H, W, Ci, Co, case, timed)]): the tables of tests/thin_refs.py, then the launches of the two
    steps as rows of the same tables.  One line of `launch_shapes.py --dtype no --batch 16 --flags` / `--dtype bf16 --batch 32
    --flags` each: the layer, the map, the channel counts and storage, the transform, bias on or off and the split count are
    the ones printed there (bf16: a wide operand the step hands over as a bf16 image is, after the dispatcher's canonical
    form, the same operand stored as bf16 -- out16 / a16 / wide16 here)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import thin_refs as T
    R, G = T.Rows, T.Wg
    step = []
    for tag, B, bf in (("f32", 16, False), ("bf16", 32, True)):
        big, lat = (B, 256, 256), (B, 32, 32)
        sk, wk = ("conv_thin_bf16_kernel", "wgrad_thin_bf16_kernel") if bf else ("conv_smallk_kernel", "wgrad_smallk_kernel")
        sn = "conv_thinn_bf16_kernel<2>" if bf else "conv_smalln_kernel<2>"
        step += [
            R(f"step-{tag}-conv_in", sk, "fwd", "c3", big, 4, 128, 3, bf16=bf, out16=bf),
            R(f"step-{tag}-post_quant", "conv_smallk_kernel", "fwd", "c1", lat, 4, 4, 4, bf16=bf),
            R(f"step-{tag}-decoder_conv_in", sk, "fwd", "c3", lat, 4, 512, 4, bf16=bf, out16=bf),
            R(f"step-{tag}-conv_out", sn, "fwd", "c3", big, 128, 3, 128, xf=T.XF_AFFINE_SILU, bf16=bf, a16=bf),
            G(f"step-{tag}-conv_out-wgrad", wk + "<false,2>", 2, "c3", big, 128, 3, 128, 1024, xf=T.XF_AFFINE_SILU, bf16=bf, wide16=bf),
            R(f"step-{tag}-conv_out-dgrad", sk, "dgrad", "c3", big, 3, 3, 128, bias=False, bf16=bf, out16=bf),
            G(f"step-{tag}-decoder_conv_in-wgrad", wk + "<true,0>", 1, "c3", lat, 4, 512, 4, 8 * B, bf16=bf, wide16=bf),
            G(f"step-{tag}-post_quant-wgrad", "wgrad_smallk_kernel<true,0>", 1, "c1", lat, 4, 4, 4, 8 * B, bf16=bf),
            R(f"step-{tag}-post_quant-dgrad", "conv_smallk_kernel", "dgrad", "c1", lat, 4, 4, 4, bias=False, bf16=bf),
            G(f"step-{tag}-conv_in-wgrad", wk + "<true,0>", 1, "c3", big, 4, 128, 3, 1024, bf16=bf, wide16=bf),
        ]
    small = list(T.ROWS_CASES) + [T.THIN_LARGE] + list(T.WG_CASES)
    return T, [("thin", c.id, *c.shape, c.Ci, c.Co, c, timed) for cs, timed in ((small, False), (step, True)) for c in cs]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _open(path):
    lib.load()  # (one HIP runtime per process: the package's loader opens torch's copy first)
    dll = C.CDLL(os.path.abspath(path))
    ia, wa, vp = C.POINTER(IgemmArgs), C.POINTER(WgradArgs), C.c_void_p
    for fn, res, argt in (("vae_igemm_rows", C.c_int, [ia, vp]), ("vae_wino_ok", C.c_int, [ia]), ("vae_wino_weight_bytes", C.c_int64, [ia]),
                          ("vae_wino_weights", C.c_int, [ia, vp, vp]), ("vae_conv_gstat_chunks", C.c_int, [ia]), ("vae_conv_gnb_chunks", C.c_int, [ia]),
                          ("vae_igemm_kernel_name", C.c_int, [ia, C.c_char_p, C.c_int32]), ("vae_wgrad_wino", C.c_int, [wa, vp]),
                          ("vae_wgrad_wino_plan", C.c_int, [wa, C.POINTER(C.c_int32)]), ("vae_wgrad_wino_positions", C.c_int, [wa]),
                          ("vae_set_option", C.c_int, [C.c_char_p, C.c_int32]), ("vae_pack_bf16", C.c_int, [vp, C.c_int64, vp, vp]),
                          ("vae_wgrad", C.c_int, [wa, vp]), ("vae_wgrad_plan", C.c_int, [wa, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
                          ("vae_wgrad_kernel_name", C.c_int, [wa, C.c_char_p, C.c_int32])):
        getattr(dll, fn).restype, getattr(dll, fn).argtypes = res, argt
    return dll


def _bits(a, b):
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return bool(torch.equal(a.view(v), b.view(v)))


class Case:
    """operands of one case, filled once; arm(dll) -> (launch function, outputs of that arm)"""

    def __init__(self, dev, kind, mode, B, H, W, Ci, Co, epi):
        self.dev, self.kind, self.mode, self.epi = dev, kind, mode, epi
        self.dims = (B, H, W, Ci, Co)
        g = torch.Generator(device=dev).manual_seed(7 + Ci + 3 * Co + H + B + (mode != "fwd"))
        Hy, Wy = ops.out_hw(kind, H, W)
        self.w = torch.randn((Co, 3, 3, Ci), device=dev, generator=g) / math.sqrt(9 * Ci)
        self.x = torch.randn((B, H, W, Ci), device=dev, generator=g) * 1.3 + 0.2
        self.dy = torch.randn((B, Hy, Wy, Co), device=dev, generator=g) if mode != "fwd" else None
        self.bias = torch.randn((Co,), device=dev, generator=g)
        self.res = torch.randn((B, Hy, Wy, Co), device=dev, generator=g) if (epi and mode == "fwd") else None
        if epi == "xf":
            self.scale, self.shift = torch.rand((B, Ci), device=dev, generator=g) + 0.5, torch.randn((B, Ci), device=dev, generator=g)
        if epi and mode == "dgrad":
            self.mean, self.rstd = torch.randn((B, 32), device=dev, generator=g) * 0.1, torch.rand((B, 32), device=dev, generator=g) + 0.5
            self.gamma, self.beta = 1 + 0.3 * torch.randn((Ci,), device=dev, generator=g), 0.2 * torch.randn((Ci,), device=dev, generator=g)
        if mode != "fwd":
            self.x = self.x if (mode == "wgrad" or (epi and mode == "dgrad")) else None

    def arm(self, dll, st):
        B, H, W, Ci, Co = self.dims
        dev, nan = self.dev, float("nan")
        if self.mode == "wgrad":
            a = ops.wgrad_args(self.kind, B, H, W, Ci, Co, Ci, prec=ops.PREC_F32)
            a.dY, a.X = _p(self.dy), _p(self.x)
            n = C.c_int32(0)
            assert dll.vae_wgrad_wino_plan(C.byref(a), C.byref(n)) == 0 and n.value > 0, "no Winograd weight gradient for this case"
            npos = dll.vae_wgrad_wino_positions(C.byref(a))
            slab, bpart = torch.full((n.value, npos * Ci * Co), nan, device=dev), torch.full((n.value, Co), nan, device=dev)
            a.nsplit, a.partial, a.bias_partial = n.value, _p(slab), _p(bpart)
            self.kernel = "wgrad3_upwino_kernel" if npos == 9 else "wgrad3_wino_kernel<0>"

            def launch():
                rc = dll.vae_wgrad_wino(C.byref(a), st)
                assert rc == 0, rc
            return launch, {"slab": slab, "bias_partial": bpart}, (a,)
        if self.mode == "fwd":
            a = ops.fwd_args(self.kind, B, H, W, Ci, Co, Ci, xf=ops.XF_AFFINE_SILU if self.epi == "xf" else ops.XF_NONE, prec=ops.PREC_F32)
            src, oshape = self.x, (B, *ops.out_hw(self.kind, H, W), Co)
            a.bias, a.res = _p(self.bias), _p(self.res)
            if self.epi == "xf":
                a.scale, a.shift = _p(self.scale), _p(self.shift)
        else:
            a = ops.up2x_dgrad_args(B, H, W, Co, Ci, prec=ops.PREC_F32) if self.kind == "c3up" else ops.dgrad_args(self.kind, B, H, W, Co, Ci, prec=ops.PREC_F32)
            src, oshape = self.dy, (B, H, W, Ci)
        out = torch.full(oshape, nan, device=dev)
        a.A, a.W, a.C = _p(src), _p(self.w), _p(out)
        assert dll.vae_wino_ok(C.byref(a)), "no Winograd kernel for this case"
        wu = torch.full(((int(dll.vae_wino_weight_bytes(C.byref(a))) + 3) // 4,), nan, device=dev)
        assert dll.vae_wino_weights(C.byref(a), _p(wu), st) == 0
        outs = {"out": out, "U": wu}
        a.Wu = _p(wu)  # (the epilogue queries below are about the kernel the transformed weights select)
        if self.epi and self.mode == "fwd":
            a.gstat_groups = 32
            nch = dll.vae_conv_gstat_chunks(C.byref(a))
            assert nch > 0 or self.epi == "xf"  # (the F(2x2)-only channel counts have no moments epilogue: 5, 1, 2 channels per group)
            if nch > 0:
                outs["gstat"] = torch.full((B, nch, 32, 2), nan, device=dev)
                a.gstat = _p(outs["gstat"])
            else:
                a.gstat_groups = 0
        if self.epi and self.mode == "dgrad":
            a.gnb_x, a.gnb_mean, a.gnb_rstd, a.gnb_gamma, a.gnb_beta = _p(self.x), _p(self.mean), _p(self.rstd), _p(self.gamma), _p(self.beta)
            a.gnb_groups, a.gnb_silu = 32, 1
            nch = dll.vae_conv_gnb_chunks(C.byref(a))
            assert nch > 0
            outs["gnb"] = torch.full((B, nch, Ci, 2), nan, device=dev)
            a.gnb_ws = _p(outs["gnb"])
        buf = C.create_string_buffer(128)
        dll.vae_igemm_kernel_name(C.byref(a), buf, 128)
        self.kernel = buf.value.decode()

        def launch():
            rc = dll.vae_igemm_rows(C.byref(a), st)
            assert rc == 0, rc
        return launch, outs, (a, wu)


class Bf16Case:
    """operands of one case of the bf16 halo-tile family, filled once; arm(dll) -> (launch function, outputs of that arm)"""

    def __init__(self, dev, kind, form, B, H, W, Ci, Co, kn):
        self.dev, self.form, self.kn, self.dims, self.opts = dev, form, kn, (B, H, W, Ci, Co), kn.get("opts", {})
        g = torch.Generator(device=dev).manual_seed(11 + Ci + 3 * Co + H + B + len(form))
        self.wkind = form.split("_")[1] if form.startswith("wgrad_c3") else "c3"
        up = form in ("up2x", "phase_fwd", "phase_dgrad") or self.wkind == "c3up"
        Hy, Wy = (2 * H, 2 * W) if up else ops.out_hw(self.wkind, H, W)
        if form == "wgrad_phase":
            Hy, Wy = 2 * H, 2 * W  # (dY is read at every second pixel)
        self.w = torch.randn((Co, 3, 3, Ci), device=dev, generator=g) / math.sqrt(9 * Ci)
        self.x = torch.randn((B, H, W, Ci), device=dev, generator=g) * 1.3 + 0.2
        self.dy = torch.randn((B, Hy, Wy, Co), device=dev, generator=g)
        self.bias = torch.randn((Co,), device=dev, generator=g)
        self.scale, self.shift = torch.rand((B, Ci), device=dev, generator=g) + 0.5, torch.randn((B, Ci), device=dev, generator=g)
        self.x16, self.dy16 = self.x.bfloat16(), self.dy.bfloat16()
        self.res = None

    def _wgrad_arm(self, dll, st):
        B, H, W, Ci, Co = self.dims
        kn, dev, nan = self.kn, self.dev, float("nan")
        a = (ops.wgrad_phase_args(B, H, W, Co, Ci, prec=ops.PREC_BF16) if self.form == "wgrad_phase"
             else ops.wgrad_args(self.wkind, B, H, W, Ci, Co, Ci, xf=kn.get("xf", ops.XF_NONE), prec=ops.PREC_BF16))
        a.dY, a.X = _p(self.dy16 if kn.get("y16") else self.dy), _p(self.x)
        a.dY16, a.X16 = _p(self.dy16) if kn.get("y16") else None, _p(self.x16) if kn.get("x16") else None
        if a.xf:
            a.scale, a.shift = _p(self.scale), _p(self.shift)
        n, fus = C.c_int32(0), C.c_int32(0)
        assert dll.vae_wgrad_plan(C.byref(a), C.byref(n), C.byref(fus)) == 0 and n.value > 0 and (fus.value or not a.xf)
        ns = kn.get("ns", n.value)
        slab = torch.full((ns, 9 * Ci * Co), nan, device=dev)
        a.nsplit, a.partial, a.out = ns, _p(slab), _p(slab)
        outs = {"slab": slab}
        if not kn.get("nobias"):
            outs["bias_partial"] = torch.full((ns, Co), nan, device=dev)
            a.bias_partial = _p(outs["bias_partial"])
        buf = C.create_string_buffer(128)
        dll.vae_wgrad_kernel_name(C.byref(a), buf, 128)
        self.kernel = buf.value.decode()

        def launch():
            rc = dll.vae_wgrad(C.byref(a), st)
            assert rc == 0, rc
        return launch, outs, (a,)

    def arm(self, dll, st):
        if self.form.startswith("wgrad"):
            return self._wgrad_arm(dll, st)
        B, H, W, Ci, Co = self.dims
        kn, dev, form = self.kn, self.dev, self.form
        dg = form in ("dgrad", "phase_dgrad")
        if form in ("phase_fwd", "phase_dgrad"):
            a = ops.phase_args(B, H, W, Co, Ci, dg, prec=ops.PREC_BF16)
        elif dg:
            a = ops.dgrad_args("c3", B, H, W, Co, Ci, prec=ops.PREC_BF16)
        else:
            a = ops.fwd_args("c3up" if form == "up2x" else "c3", B, H, W, Ci, Co, Ci, xf=kn.get("xf", ops.XF_NONE), prec=ops.PREC_BF16)
        src, src16 = (self.dy, self.dy16) if dg else (self.x, self.x16)
        full = form not in ("phase_fwd",) and not kn.get("pad")  # (a phase forward writes every second pixel, a padded row its first N columns)
        oshape = (B, H, W, a.N + kn.get("pad", 0)) if dg else (B, *self.dy.shape[1:3], a.N + kn.get("pad", 0))
        odt = torch.bfloat16 if kn.get("out16") else torch.float32
        out = torch.full(oshape, float("nan") if full else 0.0, device=dev, dtype=odt)
        wh = torch.full((self.w.numel(),), float("nan"), device=dev, dtype=torch.bfloat16)
        assert dll.vae_pack_bf16(_p(self.w), self.w.numel(), _p(wh), st) == 0
        a.A, a.A16, a.W, a.Wh, a.C, a.ldc = _p(src), _p(src16) if kn.get("a16") else None, _p(self.w), _p(wh), _p(out), oshape[-1]
        a.out_bf16 = int(bool(kn.get("out16")))
        a.bias = None if (kn.get("nobias") or dg) else _p(self.bias)
        if a.xf:
            a.scale, a.shift = _p(self.scale), _p(self.shift)
        outs = {"out": out, "Wh": wh}
        if kn.get("res"):
            if self.res is None:
                self.res = torch.randn(oshape, device=dev, generator=torch.Generator(device=dev).manual_seed(5)).to(odt)
            a.res, a.res_bf16 = _p(self.res), a.out_bf16
        if kn.get("gstat"):
            a.gstat_groups = 32
            nch = dll.vae_conv_gstat_chunks(C.byref(a))
            assert nch > 0, "no statistics epilogue for this case"
            outs["gstat"] = torch.full((B, nch, 32, 2), float("nan"), device=dev)
            a.gstat = _p(outs["gstat"])
        buf = C.create_string_buffer(128)
        dll.vae_igemm_kernel_name(C.byref(a), buf, 128)
        self.kernel = buf.value.decode()

        def launch():
            rc = dll.vae_igemm_rows(C.byref(a), st)
            assert rc == 0, rc
        return launch, outs, (a, wh)


class ThinCase:
    """one row of the tables of tests/thin_refs.py (T): a small case with the operands the tests use, or a launch of the step with
    operands drawn on the device; arm(dll) -> (launch function, outputs of that arm)"""
    T = None

    def __init__(self, dev, kind, cid, B, H, W, Ci, Co, c):
        T = self.T
        self.dev, self.c, self.rows = dev, c, isinstance(c, T.Rows)
        self.opts = {"no_thin_mfma": 1} if c.no_thin else {}
        if not cid.startswith("step-"):
            o = T.rows_operands(c) if self.rows else T.wg_operands(c)
            self.ops = {k: (None if v is None else v.to(dev)) for k, v in o._asdict().items()}
            return
        g = torch.Generator(device=dev).manual_seed(T._seed(cid))
        rnd = lambda *s: torch.randn(s, device=dev, generator=g)  # noqa: E731
        Hy, Wy = T.out_hw(c.kind, H, W)
        self.ops = {"scale": torch.rand((B, c.Cs), device=dev, generator=g) + 0.5, "shift": rnd(B, c.Cs) * 0.5}
        if self.rows:
            src = rnd(B, H, W, c.Cs) if c.form == "fwd" else rnd(B, Hy, Wy, Co)
            self.ops.update(src=src.bfloat16() if c.a16 else src, w=rnd(Co, T.taps_of(c.kind), Ci) * 0.2, bias=rnd(T.rows_dims(c)[1]) * 0.5)
        else:
            x, dy = rnd(B, H, W, c.Cs), rnd(B, Hy, Wy, Co)
            self.ops.update(x=x.bfloat16() if (c.wide16 and c.side == 2) else x, dy=dy.bfloat16() if (c.wide16 and c.side == 1) else dy)

    def arm(self, dll, st):
        T, c, o, dev, nan = self.T, self.c, self.ops, self.dev, float("nan")
        xf = c.xf != T.XF_NONE
        if self.rows:
            a = T.rows_block(c, ops)
            M, N, _, _ = T.rows_dims(c)
            outs = {"out": torch.full((M, N), nan, device=dev, dtype=torch.bfloat16 if c.out16 else torch.float32)}
            if c.track:
                outs["track"] = torch.full(((M + T.TP - 1) // T.TP, N), nan, device=dev)
            a.A, a.W, a.C, a.bias, a.track = _p(o["src"]), _p(o["w"]), _p(outs["out"]), _p(o["bias"]) if c.bias else None, _p(outs.get("track"))
            name, fn = dll.vae_igemm_kernel_name, dll.vae_igemm_rows
        else:
            a = T.wg_block(c, ops)
            outs = {"slab": torch.full((c.ns, c.Co * T.taps_of(c.kind) * c.Ci), nan, device=dev)}
            if c.bias:
                outs["bias_partial"] = torch.full((c.ns, c.Co), nan, device=dev)
            a.dY, a.X, a.bias_partial = _p(o["dy"]), _p(o["x"]), _p(outs.get("bias_partial"))
            a.out, a.partial = (_p(outs["slab"]), None) if c.ns == 1 else (None, _p(outs["slab"]))
            name, fn = dll.vae_wgrad_kernel_name, dll.vae_wgrad
        a.scale, a.shift = (_p(o["scale"]), _p(o["shift"])) if xf else (None, None)
        buf = C.create_string_buffer(128)
        name(C.byref(a), buf, 128)
        self.kernel = buf.value.decode()
        assert self.kernel == c.kernel, (c.id, self.kernel, c.kernel)

        def launch():
            rc = fn(C.byref(a), st)
            assert rc == 0, rc
        return launch, outs, (a,)


# ---- the streaming family (`--only stream`): every launch goes through vaehip.lib.lib, whose library is swapped per arm, so the
# cases are the tests' own helpers and tables.  ops._p records every tensor handed to the library: operands, results, workspaces.
_TF = ("false", "true")


def _w_moments(a):  # vae_moments_partial picks W = 4 from C, ld and the operand's alignment
    return 4 if (a[7] % 4 == 0 and a[8] % 4 == 0 and (getattr(a[0], "value", 0) or 0) & (7 if a[1] else 15) == 0) else 1


# entry point -> the kernel instantiations one call launches, from the call's own arguments
STREAM_KERNELS = {
    "vae_gn_stats_partial": lambda a: [f"gn_stats_partial_kernel<{_TF[a[1]]}>"], "vae_gn_stats_final": lambda a: ["gn_stats_final_kernel"],
    "vae_gn_apply": lambda a: [f"gn_apply_kernel<{_TF[a[1]]}>"], "vae_gn_apply_bf16": lambda a: [f"gn_apply_bf16_kernel<{_TF[a[1]]}>"],
    "vae_gn_track_partial": lambda a: [f"gn_track_partial_kernel<{_TF[a[1]]}>"], "vae_track_final": lambda a: ["track_final_kernel"],
    "vae_gn_bwd_partial": lambda a: [f"gn_bwd_partial_kernel<{_TF[a[12]]},{_TF[a[13]]},{_TF[a[1]]}>"], "vae_gn_bwd_final": lambda a: ["gn_bwd_final_kernel"],
    "vae_gn_bwd_apply": lambda a: [f"gn_bwd_apply_rows_kernel<{_TF[a[13]]},{_TF[a[14]]},{_TF[a[1]]}>"],
    "vae_moments_partial": lambda a: [f"moments_partial_kernel<{_w_moments(a)},{_TF[a[1]]}>"],
    "vae_moments_final": lambda a: ["moments_channel_kernel", "moments_total_kernel"],
    "vae_lens_planes_partial": lambda a: ["lens_planes_partial_kernel"], "vae_lens_planes_final": lambda a: ["lens_planes_final_kernel"],
    "vae_lens_project": lambda a: ["lens_project_kernel"],
    "vae_image_metrics_partial": lambda a: ["image_metrics_partial_kernel"], "vae_image_metrics_final": lambda a: ["image_metrics_final_kernel"],
    "vae_softmax_rows": lambda a: ["softmax_rows_kernel"], "vae_softmax_bwd_rows": lambda a: ["softmax_bwd_rows_kernel"],
    "vae_sample_kl": lambda a: ["sample_kl_kernel"], "vae_sample_kl_bwd": lambda a: ["sample_kl_bwd_kernel"],
    "vae_mse_partial": lambda a: ["mse_partial_kernel"], "vae_loss_final": lambda a: ["loss_final_kernel"], "vae_mse_bwd": lambda a: ["mse_bwd_kernel"],
    "vae_nchw_to_nhwc": lambda a: ["nchw_to_nhwc_kernel"], "vae_nhwc_to_nchw": lambda a: ["nhwc_to_nchw_kernel"], "vae_sumpool2x2": lambda a: ["sumpool2x2_kernel"],
    "vae_add": lambda a: ["add_kernel"], "vae_add_bf16": lambda a: ["add_bf16_kernel"], "vae_unpack_bf16": lambda a: ["unpack_bf16_kernel"],
    "vae_pack_bf16": lambda a: ["pack_bf16_kernel"], "vae_upconv_phase_weights": lambda a: ["upconv_phase_weights_kernel"],
    "vae_upconv_fold_wgrad": lambda a: ["upconv_fold_wgrad_kernel"], "vae_sqnorm": lambda a: ["sqnorm_partial_kernel", "sqnorm_final_kernel"],
    "vae_adamw": lambda a: ["adamw_kernel<false>"], "vae_adamw_ema": lambda a: ["adamw_kernel<true>"],
    "vae_sqnorm_ranges": lambda a: ["sqnorm_ranges_kernel", "sqnorm_final_kernel"],
    "vae_adamw_ranges": lambda a: [f"adamw_ranges_kernel<{_TF[a[4] is not None]}>"],
    "vae_dead_scan": lambda a: ["dead_scan_chunk_kernel<false>", "dead_scan_final_kernel"],
    "vae_dead_scan_adaptive": lambda a: ["dead_scan_chunk_kernel<true>", "dead_scan_final_kernel"],
}
# every __global__ instantiation of norm.hip, track.hip, lens.hip, image_metrics.hip and elementwise.hip
STREAM_NAMES = ({f"{k}<{_TF[x]}>" for k in ("gn_stats_partial_kernel", "gn_apply_kernel", "gn_apply_bf16_kernel", "gn_track_partial_kernel", "adamw_kernel",
                                           "adamw_ranges_kernel", "dead_scan_chunk_kernel") for x in (0, 1)}
                | {f"{k}<{_TF[s]},{_TF[g]},{_TF[x]}>" for k in ("gn_bwd_partial_kernel", "gn_bwd_apply_rows_kernel") for s in (0, 1) for g in (0, 1) for x in (0, 1)}
                | {f"moments_partial_kernel<{w},{_TF[x]}>" for w in (1, 4) for x in (0, 1)}
                | {k + "_kernel" for k in ("gn_stats_final", "track_final", "gn_bwd_final", "moments_channel", "moments_total", "lens_planes_partial",
                                           "lens_planes_final", "lens_project", "image_metrics_partial", "image_metrics_final", "softmax_rows", "softmax_bwd_rows",
                                           "sample_kl", "sample_kl_bwd", "mse_partial", "loss_final", "mse_bwd", "nchw_to_nhwc", "nhwc_to_nchw", "sumpool2x2", "add",
                                           "add_bf16", "unpack_bf16", "pack_bf16", "upconv_phase_weights", "upconv_fold_wgrad", "sqnorm_partial", "sqnorm_final",
                                           "sqnorm_ranges", "dead_scan_final")})
GN_STEP = [(16, 256, 256, 128), (16, 128, 128, 256), (16, 64, 64, 512), (16, 32, 32, 512)]  # (B, H, W, C): the GroupNorms of the 256^2 step
ARENA_N = 83_653_863   # parameters of the model: the optimizer kernels' size
RING_BYTES = 320 << 20  # operands rotate over more than the 256 MB memory-side cache


def stream_small(dev):
    """-> [(id, fn)]: fn() runs one case's launches through the package's loader; the tables of tests/norm_refs.py and
    tests/streaming_refs.py and the case lists of four GPU test files, with the helpers of the tests that own them"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import lens_refs as LR
    import norm_refs as nr
    import streaming_refs as sr
    import test_image_metrics_gpu as IM
    import test_norm_edges_gpu as NE
    import test_tracker_metrics_gpu as TM
    import test_trainable_gpu as TR
    from vaehip.trainable import RangeTable
    cases = []
    build_case = functools.lru_cache(maxsize=1)(nr.build_case)  # (one build serves the arms of a case)

    def case(cid):
        return lambda fn: cases.append((cid, fn))

    for name in nr.SHAPES:
        for values in ("plain", "large_mean_30"):
            for x16 in (False, True):
                @case(f"gn/{name}/{values}/{'bf16' if x16 else 'f32'}")
                def _(name=name, values=values, x16=x16):
                    c = build_case(name, values)
                    st16 = lambda t: t.to(dev).bfloat16() if x16 else t.to(dev)  # noqa: E731
                    x, gamma, beta = st16(c.x), c.gamma.to(dev), c.beta.to(dev)
                    st = NE.k_stats(x, gamma, beta)
                    for xf in (NE.XF_AFFINE, NE.XF_AFFINE_SILU):
                        NE.k_apply(x, st, xf)
                        if x.shape[-1] % 8 == 0:
                            NE.k_apply16(x, st, xf)
                    NE.k_track(x, st)
                    for silu in (False, True):
                        for g16 in (False, True):
                            g = c.g.to(dev).bfloat16() if g16 else c.g.to(dev)
                            NE.k_bwd(x, g, st, gamma, beta, silu, st16(c.add) if silu else None, want32=not g16, want16=g16 or x16)
    for rows in nr.TRACK_ROWS:
        for Cc in nr.TRACK_C:
            @case(f"track_final/{rows}x{Cc}")
            def _(rows=rows, Cc=Cc):
                NE.k_track_final(nr.track_ws(rows, Cc).to(dev), rows, torch.full((Cc,), float("nan"), device=dev))

    @case("dead_scan")
    def _():
        flat, segs, _ = nr.dead_layout(0.0)
        flat = flat.to(dev)
        NE.k_dead_scan(flat, segs, nr.DEAD_THR)
        for fixed in (0, 1):
            NE.k_dead_scan(flat, segs, nr.DEAD_THR, [0.01 * (1 + s % 5) for s in range(len(segs))], fixed)
    for cols in sr.SOFTMAX_COLS:
        @case(f"softmax/{cols}")
        def _(cols=cols):
            S, dP = (t.to(dev) for t in sr.softmax_inputs(cols))
            ops.softmax_bwd_rows_(ops.softmax_rows_(S), dP)
    for shape in sr.SAMPLE_SHAPES:
        @case(f"sample_kl/{shape}")
        def _(shape=shape):
            mom, eps, dz, _ = (t.to(dev) for t in sr.sample_inputs(*shape, True))
            ops.sample_kl(mom, eps)
            ops.sample_kl(mom, None)
            ops.sample_kl_bwd(mom, eps, dz, 1e-3)
    for n in sr.MSE_SIZES:
        @case(f"mse/{n}")
        def _(n=n):
            recon, target, klp = (t.to(dev) for t in sr.mse_inputs(n))
            ops.mse_kl_loss(recon, target, klp, 1e-3)
            ops.mse_bwd(recon, target)
            ops.add(recon, target)
    for n in (sr.ADAM_N, sr.ADAM_GRID_N):
        @case(f"adamw/{n}")
        def _(n=n):
            for ema in (False, True):
                p, g = sr.adam_params(n).to(dev), sr.adam_grad(n, 3.0, 1).to(dev)
                m, v, e, sq = torch.zeros_like(p), torch.zeros_like(p), p.clone(), torch.full((1,), float("nan"), device=dev)
                ops.sqnorm(g, sq, torch.full((2048,), float("nan"), device=dev))
                hp = (sq, 1.0, 1e-3, *sr.ADAM["betas"], sr.ADAM["eps"], sr.ADAM["wd"])
                for step in (1, 2):
                    if ema:
                        ops.adamw_ema(p, g, m, v, e, *hp, step, 0.9 * (step - 1))
                    else:
                        ops.adamw(p, g, m, v, *hp, step)
    for n in sr.BF16_LENGTHS:
        @case(f"bf16_pack/{n}")
        def _(n=n):
            for rot in sr.bf16_rotations(n):
                src = sr.bf16_table(n, rot).to(dev)
                h = ops.pack_bf16(src, torch.full((n,), float("nan"), device=dev, dtype=torch.bfloat16))
                lib.call("vae_unpack_bf16", ops._p(h), n, ops._p(torch.full((n,), float("nan"), device=dev)), ops._stream())

    @case("bf16_add")
    def _():
        a, b = (t.to(dev) for t in sr.bf16_add_pairs())
        ops.add(a, b)

    @case("layout")
    def _():
        g = torch.Generator().manual_seed(3)
        x = torch.randn((2, 3, 9, 13), generator=g).to(dev)
        ops.nhwc_to_nchw(ops.nchw_to_nhwc(x, 4))
        src, dst = torch.randn((2, 10, 14, 8), generator=g).to(dev), torch.full((2, 5, 7, 8), float("nan"), device=dev)
        lib.call("vae_sumpool2x2", ops._p(src), 2, 5, 7, 8, ops._p(dst), ops._stream())
        w, we = torch.randn((5, 3, 3, 7), generator=g).to(dev), torch.full((4, 5, 3, 3, 7), float("nan"), device=dev)
        lib.call("vae_upconv_phase_weights", ops._p(w), 5, 7, ops._p(we), ops._stream())
        dbe, dw, db = torch.randn((4, 5), generator=g).to(dev), torch.full((5, 3, 3, 7), float("nan"), device=dev), torch.full((5,), float("nan"), device=dev)
        lib.call("vae_upconv_fold_wgrad", ops._p(we), ops._p(dbe), 5, 7, ops._p(dw), ops._p(db), ops._stream())
    for Cc, dt, xf, B, H, W in TM._cases():
        @case(f"moments/C{Cc}/{str(dt)[6:]}/xf{xf}/{B}x{H}x{W}")
        def _(Cc=Cc, dt=dt, xf=xf, B=B, H=H, W=W):
            g = torch.Generator(device="cpu").manual_seed(Cc * 131 + xf * 7 + B)
            x = (torch.randn((B, H, W, Cc), generator=g) * 1.3 + 0.4).to(dev).to(dt)
            ops.moments(x, TM._stats(B, Cc, dev, Cc + xf) if xf else None, xf)
    for lc in LR.plane_cases():
        @case(f"lens/{LR.case_id(lc)}")
        def _(lc=lc):
            H, W, cc, B, S, bf16 = lc
            buf, Cn = LR.make_input(H, W, cc, B, bf16)
            x, wd = buf.to(dev)[..., :Cn], [t.to(dev) for t in LR.decoder_weights(1)]
            for ch in LR.channel_lists(Cn):
                idx = torch.tensor(ch, dtype=torch.int32, device=dev)
                ops.lens_planes(x, S, idx, ch)
                ops.lens_project(x, S, idx, *wd, False, ch)
    for lc in LR.full_map_cases():
        @case(f"lens_full/{LR.case_id(lc)}")
        def _(lc=lc):
            Cn, H, W, B, S, bf16 = lc
            x = LR.make_input(H, W, str(Cn), B, bf16)[0].to(dev)
            ops.lens_project(x, S, torch.arange(Cn, dtype=torch.int32, device=dev), *[t.to(dev) for t in LR.decoder_weights(Cn)], True, list(range(Cn)))
    for shape in IM.SHAPES:
        for variant in ("noisy", "flat"):
            @case(f"image_metrics/{'x'.join(map(str, shape))}/{variant}")
            def _(shape=shape, variant=variant):
                p, t = IM._inputs(shape, variant)
                ops.image_metrics(p.to(dev), t.to(dev))
    chunk = lib.query("vae_dead_scan_chunk")
    for rc, (ranges, n) in TR._range_cases(chunk).items():
        @case(f"ranges/{rc}")
        def _(rc=rc, ranges=ranges, n=n):
            gen = torch.Generator().manual_seed(len(rc) * 131 + n)
            host = dict(p=sr.adam_params(n, seed=n), g=torch.randn(n, generator=gen) * 3.0, m=torch.randn(n, generator=gen) * 0.1,
                        v=torch.rand(n, generator=gen) * 1e-2, e=sr.adam_params(n, seed=n + 1))
            tab, out = RangeTable(ranges, dev, n), torch.full((1,), float("nan"), device=dev)
            tab.ws.fill_(float("nan"))
            g = host["g"].to(dev)
            ops.sqnorm_ranges(g, tab, out)
            for ema, max_norm, decay in ((False, 1.0, 0.0), (True, 1.0, 0.9), (True, 0.0, 0.0)):
                t = {k: host[k].to(dev) for k in ("p", "m", "v") + (("e",) if ema else ())}
                ops.adamw_ranges(t["p"], g, t["m"], t["v"], t.get("e"), tab, out, max_norm, 1e-3, *sr.ADAM["betas"], sr.ADAM["eps"], sr.ADAM["wd"], 2, decay)
    return cases


def stream_timed(dev):
    """-> [(id, setup)]: setup() -> (ring length, fn(i)); fn(i) is ONE call of a C entry point (lib.call) on operand set i of a
    ring of more than RING_BYTES, every workspace and result allocated beforehand -- nothing but the launch lies between the
    events.  The GroupNorm entry points at GN_STEP in fp32 storage and, at batch 32, in bf16 storage (the final passes, whose
    operands are workspaces of a few hundred KB, have no ring); vae_moments_partial / vae_moments_final at the widest shape; the
    optimizer kernels, vae_sqnorm (also at 2^20 elements, where its final pass is a third of the time) and the dead-weight scans
    at ARENA_N."""
    G, cases, st = 32, [], ops._stream
    p = ops._p
    for B16, H, W, Cc in GN_STEP:
        for x16 in (False, True):
            B, dt = (2 * B16, torch.bfloat16) if x16 else (B16, torch.float32)
            tag = f"{B}x{H}x{W}x{Cc}/{'bf16' if x16 else 'f32'}"
            HW = H * W
            ring = max(2, -(-RING_BYTES // (B * HW * Cc * (2 if x16 else 4))))

            def setup(entry, silu=False, g16=False, ring=ring, B=B, HW=HW, H=H, W=W, Cc=Cc, dt=dt, x16=x16):
                g = torch.Generator(device=dev).manual_seed(Cc + H)
                f32 = lambda *s: torch.empty(s, device=dev)  # noqa: E731
                xs = [(torch.randn((B, H, W, Cc), device=dev, generator=g) * 1.7 + 0.3).to(dt) for _ in range(ring)]
                gamma, beta = 1 + 0.3 * torch.randn((Cc,), device=dev, generator=g), 0.2 * torch.randn((Cc,), device=dev, generator=g)
                s = ops.gn_stats(xs[0], gamma, beta)  # (statistics of one set serve all: timing only)
                nch, xb = ops._gn_nchunk(B, HW, Cc), int(x16)
                if entry == "vae_gn_stats_partial":
                    ws = f32(B, nch, G, 2)
                    return ring, lambda i: lib.call(entry, p(xs[i]), xb, B, HW, Cc, G, nch, p(ws), st())
                if entry == "vae_gn_stats_final":
                    ws, o = f32(B, nch, G, 2), [f32(B, G), f32(B, G), f32(B, Cc), f32(B, Cc)]
                    lib.call("vae_gn_stats_partial", p(xs[0]), xb, B, HW, Cc, G, nch, p(ws), st())
                    return 1, lambda i: lib.call(entry, p(ws), B, HW, Cc, G, nch, p(gamma), p(beta), 1e-6, p(o[0]), p(o[1]), p(o[2]), p(o[3]), st())
                if entry in ("vae_gn_apply", "vae_gn_apply_bf16"):
                    y = torch.empty((B, H, W, Cc), device=dev, dtype=torch.bfloat16 if entry.endswith("bf16") else torch.float32)
                    return ring, lambda i: lib.call(entry, p(xs[i]), xb, p(s.scale), p(s.shift), B, HW, Cc, ops.XF_AFFINE_SILU, p(y), st())
                if entry == "vae_gn_track_partial":
                    ws = f32(B * nch, Cc)
                    return ring, lambda i: lib.call(entry, p(xs[i]), xb, p(s.scale), p(s.shift), B, HW, Cc, nch, p(ws), st())
                if entry == "vae_moments_partial":
                    mch = min(nch, 1024 // B)
                    ws = f32(Cc, B * mch, 4)
                    return ring, lambda i: lib.call(entry, p(xs[i]), xb, p(s.scale), p(s.shift), ops.XF_AFFINE_SILU, B, HW, Cc, Cc, mch, p(ws), st())
                if entry == "vae_moments_final":
                    mch = min(nch, 1024 // B)
                    ws, chan, out = f32(Cc, B * mch, 4), torch.empty((Cc, 2), device=dev, dtype=torch.float64), f32(Cc + 2)
                    lib.call("vae_moments_partial", p(xs[0]), xb, p(s.scale), p(s.shift), ops.XF_AFFINE_SILU, B, HW, Cc, Cc, mch, p(ws), st())
                    return 1, lambda i: lib.call(entry, p(ws), B, HW, Cc, mch, p(chan), p(out), st())
                gs = [torch.randn((B, H, W, Cc), device=dev, generator=g).to(torch.bfloat16 if g16 else torch.float32) for _ in range(2)]
                ws, coef, dg, db = f32(B, nch, Cc, 2), f32(B, G, 2), f32(Cc), f32(Cc)
                lib.call("vae_gn_bwd_partial", p(xs[0]), xb, p(gs[0]), p(s.mean), p(s.rstd), p(gamma), p(beta), B, HW, Cc, G, nch, int(silu), int(g16), p(ws), st())
                lib.call("vae_gn_bwd_final", p(ws), p(s.rstd), p(gamma), B, HW, Cc, G, nch, p(dg), p(db), p(coef), st())
                if entry == "vae_gn_bwd_partial":
                    return ring, lambda i: lib.call(entry, p(xs[i]), xb, p(gs[i % 2]), p(s.mean), p(s.rstd), p(gamma), p(beta), B, HW, Cc, G, nch, int(silu),
                                                    int(g16), p(ws), st())
                if entry == "vae_gn_bwd_final":
                    return 1, lambda i: lib.call(entry, p(ws), p(s.rstd), p(gamma), B, HW, Cc, G, nch, p(dg), p(db), p(coef), st())
                dx = torch.empty((B, H, W, Cc), device=dev, dtype=torch.bfloat16 if g16 else torch.float32)
                return ring, lambda i: lib.call("vae_gn_bwd_apply", p(xs[i]), xb, p(gs[i % 2]), p(s.mean), p(s.rstd), p(gamma), p(beta), p(coef), None, B, HW,
                                                Cc, G, int(silu), int(g16), None if g16 else p(dx), p(dx) if g16 else None, st())
            for entry in ("vae_gn_stats_partial", "vae_gn_stats_final", "vae_gn_apply", "vae_gn_apply_bf16", "vae_gn_track_partial", "vae_gn_bwd_final"):
                cases.append((f"{entry}/{tag}", functools.partial(setup, entry)))
            if (H, Cc) == (256, 128):
                cases += [(f"{entry}/{tag}", functools.partial(setup, entry)) for entry in ("vae_moments_partial", "vae_moments_final")]
            for silu in (False, True):
                for g16 in (False, True):
                    if g16 != x16 and (H, Cc) != (64, 512):
                        continue  # the step stores g like x; the mixed storages are timed at one shape
                    for entry in ("vae_gn_bwd_partial", "vae_gn_bwd_apply"):
                        cases.append((f"{entry}/silu{int(silu)}/g{'bf16' if g16 else 'f32'}/{tag}", functools.partial(setup, entry, silu, g16)))

    def optimizer(ema):
        def setup():
            t = [torch.randn((ARENA_N,), device=dev) * (0.05 if k != 3 else 0.0) for k in range(5)]
            t[3].add_(1e-4)
            sq = torch.zeros((1,), device=dev)
            hp = (sq, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 2)
            if ema:
                return 1, lambda i: ops.adamw_ema(t[0], t[1], t[2], t[3], t[4], *hp, 0.999)
            return 1, lambda i: ops.adamw(t[0], t[1], t[2], t[3], *hp)
        return setup
    cases += [("vae_adamw/arena", optimizer(False)), ("vae_adamw_ema/arena", optimizer(True))]

    def sqnorm_setup(n):
        def setup():
            g, sq, ws = torch.randn((n,), device=dev), torch.zeros((1,), device=dev), torch.empty((2048,), device=dev)
            return 1, lambda i: lib.call("vae_sqnorm", p(g), n, p(ws), 2048, p(sq), st())
        return setup
    cases += [("vae_sqnorm/arena", sqnorm_setup(ARENA_N)), ("vae_sqnorm/2^20", sqnorm_setup(1 << 20))]

    def add16_setup():  # the residual add of the bf16 step at [32, 128, 128, 256]
        n = 32 * 128 * 128 * 256
        a, b, o = (torch.randn((3, n), device=dev).bfloat16() for _ in range(3))
        return 3, lambda i: lib.call("vae_add_bf16", p(a[i]), p(b[i]), n, p(o[i]), st())
    cases.append(("vae_add_bf16/32x128x128x256", add16_setup))

    def dead_setup(adaptive):
        def setup():
            chunk = lib.query("vae_dead_scan_chunk")
            nchunk = -(-ARENA_N // chunk)
            w = torch.randn((ARENA_N,), device=dev) * 0.05
            seg, chunk0 = torch.tensor([0, ARENA_N], dtype=torch.int64, device=dev), torch.tensor([0, nchunk], dtype=torch.int32, device=dev)
            pcnt, psum = torch.zeros((nchunk,), dtype=torch.int64, device=dev), torch.zeros((nchunk,), dtype=torch.float64, device=dev)
            cnt, asum, at = torch.zeros((1,), dtype=torch.int64, device=dev), torch.zeros((1,), dtype=torch.float64, device=dev), torch.full((1,), 0.01, device=dev)
            if adaptive:
                return 1, lambda i: lib.call("vae_dead_scan_adaptive", p(w), p(seg), p(chunk0), 1, nchunk, 1e-5, 1, p(at), p(pcnt), p(cnt), st())
            return 1, lambda i: lib.call("vae_dead_scan", p(w), p(seg), p(chunk0), 1, nchunk, 1e-5, p(pcnt), p(psum), p(cnt), p(asum), st())
        return setup
    cases += [("vae_dead_scan/arena", dead_setup(False)), ("vae_dead_scan_adaptive/arena", dead_setup(True))]
    return cases


# ---- the per-channel statistics family (`--only chanstat`): one ops entry point per case, run like the streaming family
def _w4(ptr, bf16, C, ld):  # vec4_ok of csrc/chanstat_common.h
    return C % 4 == 0 and ld % 4 == 0 and (getattr(ptr, "value", 0) or 0) & (7 if bf16 else 15) == 0


def _w_changrad(a):
    return 4 if _w4(a[0], a[1], a[8], a[2]) and _w4(a[3], a[4], a[8], a[5]) else 1


def _w_inject(a):
    return 4 if (_w4(a[0], a[1], a[8], a[2]) and _w4(a[3], a[4], a[8], a[5]) and _w4(a[11], a[4], a[8], a[8]) and _w4(a[6], 0, 4, 4)) else 1


CHANSTAT_KERNELS = {
    "vae_moments_partial": STREAM_KERNELS["vae_moments_partial"], "vae_moments_final": STREAM_KERNELS["vae_moments_final"],
    "vae_chanhist_partial": lambda a: [f"chanhist_partial_kernel<{_w_moments(a)},{_TF[a[1]]}>"], "vae_chanhist_final": lambda a: ["chanhist_final_kernel"],
    "vae_changroup_partial": lambda a: [f"changroup_partial_kernel<{_w_moments(a)},{_TF[a[1]]}>"], "vae_changroup_final": lambda a: ["changroup_final_kernel"],
    "vae_chancov_partial": lambda a: [f"chancov_partial_kernel<{_TF[_w_moments(a) == 4]},{_TF[a[1]]}>"], "vae_chancov_final": lambda a: ["chancov_final_kernel"],
    "vae_changrad_partial": lambda a: [f"changrad_partial_kernel<{_w_changrad(a)},{_TF[a[1]]},{_TF[a[4]]}>"], "vae_changrad_final": lambda a: ["changrad_final_kernel"],
    "vae_actreg_partial": lambda a: [f"actreg_partial_kernel<{4 if _w4(a[0], a[1], a[5], a[2]) else 1},{_TF[a[1]]}>"], "vae_actreg_final": lambda a: ["actreg_final_kernel"],
    "vae_actreg_inject": lambda a: [f"actreg_inject_kernel<{a[9]},{_w_inject(a)},{_TF[a[1]]},{_TF[a[4]]}>"],
}
# every __global__ instantiation of track.hip's moments, chanhist.hip, chancov.hip, changrad.hip, changroup.hip and actreg.hip
CHANSTAT_NAMES = ({f"{k}_partial_kernel<{w},{_TF[x]}>" for k in ("moments", "chanhist", "changroup", "actreg") for w in (1, 4) for x in (0, 1)}
                  | {f"chancov_partial_kernel<{_TF[v]},{_TF[x]}>" for v in (0, 1) for x in (0, 1)}
                  | {f"changrad_partial_kernel<{w},{_TF[x]},{_TF[g]}>" for w in (1, 4) for x in (0, 1) for g in (0, 1)}
                  | {f"actreg_inject_kernel<{k},{w},{_TF[x]},{_TF[g]}>" for k in (0, 1) for w in (1, 4) for x in (0, 1) for g in (0, 1)}
                  | {k + "_kernel" for k in ("moments_channel", "moments_total", "chanhist_final", "chancov_final", "changrad_final", "changroup_final", "actreg_final")})
BF, F32 = torch.bfloat16, torch.float32


def _chanstat_operands(dev, Cc, B, H, W, layout, dt, seed):
    import chanhist_refs as HR
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = HR.frame_layout((torch.randn((B, H, W, Cc), generator=g) * 1.3 + 0.4).to(dev).to(dt), layout)
    sc, sh = HR.stats_rows(B, x.stride(2), seed + 1)
    return x, ops.Stats(None, None, sc.to(dev), sh.to(dev))


def chanstat_small(dev):
    """-> [(id, fn)]: fn() is one call of an ops entry point of the family: FRAME_CASES x storage x transform (both kinds for
    actreg, the four storage pairs for changrad and actreg_inject)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import chanhist_refs as HR
    cases = []
    for Cc, B, H, W, layout in HR.FRAME_CASES:
        tag = f"C{Cc}/{B}x{H}x{W}/{layout}"
        for dt in (F32, BF):
            x, st = _chanstat_operands(dev, Cc, B, H, W, layout, dt, Cc * 131 + B)
            sd = str(dt)[6:]
            for xf in ((0,) if layout == "offset" else (0, ops.XF_AFFINE, ops.XF_AFFINE_SILU)):
                for name in ("moments", "chanhist", "changroup", "chancov"):
                    cases.append((f"{name}/{tag}/{sd}/xf{xf}", functools.partial(getattr(ops, name), x, st if xf else None, xf)))
            for kind, thr in (("ceiling", 0.5), ("floor", 0.3)):
                cases.append((f"actreg_stats/{kind}/{tag}/{sd}", functools.partial(ops.actreg_stats, x, kind, thr, 1.0)))
            for dg in (F32, BF):
                gr = _chanstat_operands(dev, Cc, B, H, W, layout if dg == dt else "plain", dg, Cc * 17 + B)[0]
                cases.append((f"changrad/{tag}/a{sd}/g{str(dg)[6:]}", functools.partial(ops.changrad, x, gr)))
                coef = torch.linspace(-0.5, 0.5, Cc, device=dev)
                for kind, thr in (("ceiling", 0.5), ("floor", 0.3)):
                    cases.append((f"actreg_inject/{kind}/{tag}/a{sd}/g{str(dg)[6:]}", functools.partial(ops.actreg_inject, x, gr, kind, thr, coef)))
    return cases


def chanstat_timed(dev):
    """-> [(id, setup)]: one ops call per launch on a ring of operands at the widest GroupNorm of the 256^2 step and at its
    narrowest tensor (the decoder's 3-channel output as the prefix view of a 4-channel buffer); an ops call allocates its
    workspace and results from the caching allocator, which every arm does alike"""
    cases = []
    for (B, H, W, Cc, view), dt in itertools.product(((16, 256, 256, 128, False), (16, 32, 32, 512, False), (16, 256, 256, 3, True)), (F32, BF)):
        tag = f"{B}x{H}x{W}x{Cc}/{'bf16' if dt == BF else 'f32'}"
        ring = max(2, -(-RING_BYTES // (B * H * W * (Cc + view) * (2 if dt == BF else 4))))

        def setup(name, ring=ring, B=B, H=H, W=W, Cc=Cc, view=view, dt=dt):
            g = torch.Generator(device=dev).manual_seed(Cc + H)
            xs = [(torch.randn((B, H, W, Cc + view), device=dev, generator=g) * 1.7 + 0.3).to(dt)[..., :Cc] for _ in range(ring)]
            sc, sh = torch.rand((B, Cc + view), device=dev, generator=g) + 0.5, torch.randn((B, Cc + view), device=dev, generator=g) * 0.2
            st = ops.Stats(None, None, sc, sh)
            if name in ("moments", "chanhist", "changroup", "chancov"):
                return ring, lambda i: getattr(ops, name)(xs[i], st, ops.XF_AFFINE_SILU)
            if name == "actreg_stats":
                return ring, lambda i: ops.actreg_stats(xs[i], "ceiling", 0.5, 1.0)
            gs = [torch.randn((B, H, W, Cc), device=dev, generator=g).to(dt) for _ in range(2)]
            if name == "changrad":
                return ring, lambda i: ops.changrad(xs[i], gs[i % 2])
            coef = torch.linspace(-0.5, 0.5, Cc, device=dev)
            return ring, lambda i: ops.actreg_inject(xs[i], gs[i % 2], "ceiling", 0.5, coef)
        for name in ("moments", "chanhist", "changroup", "chancov", "actreg_stats", "changrad", "actreg_inject"):
            if name == "chancov" and Cc == 512 and dt == BF:
                continue  # (ten tile pairs: the family's slowest case; fp32 storage times the same kernel body)
            cases.append((f"{name}/{tag}", functools.partial(setup, name)))
    return cases


def _stream_run(fn, dll, record, kernels=STREAM_KERNELS):
    """one run of fn on library dll -> the tensors it handed to the library, in order; record: set of launched instantiations"""
    seen, order, p0, call0 = set(), [], ops._p, lib.call

    def p(t):
        if t is not None and id(t) not in seen:
            seen.add(id(t))
            order.append(t)
        return p0(t)

    def call(name, *a):
        if name in kernels:
            assert len(a) == len(SIGNATURES[name]), (name, len(a))  # (the argument positions `kernels` reads are those of this signature)
            record.update(kernels[name](a))
        return call0(name, *a)
    lib._dll, ops._p, lib.call = dll, p, call
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops._p, lib.call = p0, call0
        del lib.call  # (the instance attribute: the class's method is back)
    return order


def stream_main(arg, names, paths, small=stream_small, timed_cases=stream_timed, kernels=STREAM_KERNELS, all_names=STREAM_NAMES):
    dev = torch.device("cuda:0")
    lib.load()
    home, dlls = lib._dll, []
    for s in paths:
        d = C.CDLL(os.path.abspath(s))
        d.vae_last_error.restype = C.c_char_p
        for fn, argt in SIGNATURES.items():
            getattr(d, fn).restype, getattr(d, fn).argtypes = (C.c_int64 if fn in ("vae_wino_weight_floats", "vae_wino_weight_bytes") else C.c_int), argt
        dlls.append(d)
    rows, launched, all_equal = [], set(), True
    try:
        for cid, fn in small(dev):
            first, eq, here = None, {}, set()
            for i, d in enumerate(dlls):
                got = _stream_run(fn, d, here, kernels)
                if i == 0:
                    first = got
                else:
                    eq[names[i]] = len(got) == len(first) and all(a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
                                                                    for a, b in zip(got, first))
            launched |= here
            all_equal = all_equal and all(eq.values())
            rows.append({"case": cid, "kernels": sorted(here), "tensors_compared": len(first), "bitwise_equal_to_new": eq, "bitwise": all(eq.values())})
            print(json.dumps(rows[-1]), flush=True)
            del first, got
            torch.cuda.empty_cache()
        timed = []
        for cid, setup in ([] if arg.launches <= 0 else timed_cases(dev)):
            lib._dll = home
            ring, fn = setup()
            here = set()
            for d in dlls:  # warm-up, and the instantiations the case launches
                _stream_run(lambda: [fn(i) for i in range(min(ring, 2))], d, here, kernels)
            ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(arg.launches)] for _ in dlls]
            for k in range(arg.launches):
                for i in ((k + j) % len(dlls) for j in range(len(dlls))):  # (every arm takes every place in the round equally often)
                    lib._dll = dlls[i]
                    ev[i][k][0].record()
                    fn((k * len(dlls) + i) % ring)
                    ev[i][k][1].record()
            torch.cuda.synchronize()
            row = {"case": cid, "kernels": sorted(here), "ring": ring}
            for i, nm in enumerate(names):
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[i])
                row[nm] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}
            for nm in names:
                if nm != "parent":
                    row[f"{nm}_over_parent"] = round(row[nm]["median_ms"] / row["parent"]["median_ms"], 4)
            if "parent2" in names:  # the case's own floor, never below one rounding unit of the recorded medians
                row["margin"] = round(max(2 * abs(row["parent2_over_parent"] - 1), 1e-4 / row["parent"]["median_ms"]), 4)
                row["within_margin"] = row["new"]["median_ms"] / row["parent"]["median_ms"] - 1 <= row["margin"]
            print(json.dumps(row), flush=True)
            timed.append(row)
            del fn, setup
            torch.cuda.empty_cache()
    finally:
        lib._dll = home
    missing = sorted(all_names - launched) + sorted("unknown: " + k for k in launched - all_names)
    res = {"libs": dict(zip(names, [os.path.basename(s) for s in paths])), "launches_per_arm": arg.launches, "all_bitwise_equal": all_equal, "rows": rows,
           "timed": timed, "instantiations_not_launched": missing, "all_within_margin": all(r.get("within_margin", True) for r in timed)}
    print("instantiations not launched:", missing)
    print("all outputs and workspaces bitwise equal:", all_equal)
    if arg.out:
        with open(arg.out, "w") as f:
            json.dump(res, f, indent=1)
    return 1 if (not all_equal or missing) else 0 if res["all_within_margin"] else 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="NEW.so PARENT.so [name=OTHER.so ...]")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=["", "wino4", "wino2", "up", "bf16", "thin", "stream", "chanstat"])
    arg = ap.parse_args()
    assert len(arg.libs) >= 2, "two libraries: this build and the parent's"
    names = ["new", "parent"] + [s.split("=", 1)[0] for s in arg.libs[2:]]
    if arg.only == "stream":
        return stream_main(arg, names, [s.split("=", 1)[-1] for s in arg.libs])
    if arg.only == "chanstat":
        return stream_main(arg, names, [s.split("=", 1)[-1] for s in arg.libs], chanstat_small, chanstat_timed, CHANSTAT_KERNELS, CHANSTAT_NAMES)
    dlls = [_open(s.split("=", 1)[-1]) for s in arg.libs]
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = WINO2 if arg.only == "wino2" else (STEP + SMALL if arg.only != "up" else []) + (UP if arg.only != "wino4" else [])
    if arg.only == "bf16":
        cases = BF16_SMALL + BF16_STEP
    if arg.only == "thin":
        ThinCase.T, cases = thin_cases()
    for d in dlls:  # (an option of the library, so of every copy)
        d.vae_set_option(b"no_wino4", 1 if arg.only == "wino2" else 0)
    rows, all_equal = [], True
    for kind, mode, B, H, W, Ci, Co, epi, timed in cases:
        c = {"bf16": Bf16Case, "thin": ThinCase}.get(kind, Case)(dev, kind, mode, B, H, W, Ci, Co, epi)
        first, eq, launches, keep = None, {}, [], []
        for i, d in enumerate(dlls):  # one arm's outputs at a time beside the first's
            for o, v in getattr(c, "opts", {}).items():  # (a library option the case runs under: set on every copy, cleared below)
                d.vae_set_option(o.encode(), v)
            launch, outs, alive = c.arm(d, st)
            launch()
            torch.cuda.synchronize()
            if i == 0:
                first = outs
                finite = all(bool(torch.isfinite(t).all()) for t in outs.values())
            else:
                eq[names[i]] = all(_bits(outs[k], first[k]) for k in first)
            launches.append(launch)
            keep.append((alive, outs) if timed else None)  # (the timed launches keep writing their outputs)
            if i and not timed:
                del outs
        all_equal = all_equal and all(eq.values()) and finite
        row = {"kernel": c.kernel, "mode": mode, "B": B, "H": H, "W": W, "Cin": Ci, "Cout": Co, "epilogue": epi, "compared": sorted(first),
               "bitwise_equal_to_new": eq, "bitwise": all(eq.values()), "finite": finite}
        if timed:
            for _ in range(3):
                for launch in launches:
                    launch()
            ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(arg.launches)] for _ in dlls]
            for k in range(arg.launches):
                for i in ((k + j) % len(launches) for j in range(len(launches))):  # (every arm takes every place in the round equally often)
                    ev[i][k][0].record()
                    launches[i]()
                    ev[i][k][1].record()
            torch.cuda.synchronize()
            for i, nm in enumerate(names):
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[i])
                q = statistics.quantiles(ms, n=4)
                row[nm] = {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(ms[0], 4),
                           "max_ms": round(ms[-1], 4)}
            for nm in names:
                if nm != "parent":
                    row[f"{nm}_over_parent"] = round(row[nm]["median_ms"] / row["parent"]["median_ms"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        for d in dlls:
            for o in getattr(c, "opts", {}):
                d.vae_set_option(o.encode(), 0)
        del c, first, launches, keep
        torch.cuda.empty_cache()
    res = {"libs": dict(zip(names, [os.path.basename(s.split("=", 1)[-1]) for s in arg.libs])), "launches_per_arm": arg.launches,
           "all_bitwise_equal": all_equal, "rows": rows}
    if "parent2" in names and any("parent" in r for r in rows):  # the run's own floor: what two copies of one file differ by, doubled
        floor = {}
        for r in rows:
            if "parent" in r:
                floor[r["kernel"]] = max(floor.get(r["kernel"], 0.0), abs(r["parent2"]["median_ms"] / r["parent"]["median_ms"] - 1))
        res["margin"] = {k: round(2 * v, 4) for k, v in floor.items()}
        for r in rows:
            if "parent" in r:
                r["within_margin"] = r["new"]["median_ms"] / r["parent"]["median_ms"] - 1 <= res["margin"][r["kernel"]]
        res["all_within_margin"] = all(r["within_margin"] for r in rows if "parent" in r)
        print("margins:", json.dumps(res["margin"]), "new within them on every case:", res["all_within_margin"])
    timed_rows = [r for r in rows if "parent" in r and "wino4" in r["kernel"]]
    if timed_rows:  # the step's F(4x4) launches, one of each: sum of the medians per arm
        res["wino4_sum_of_medians_ms"] = {nm: round(sum(r[nm]["median_ms"] for r in timed_rows), 4) for nm in names}
    if arg.only in ("bf16", "thin"):  # the small cases together reach every instantiation the dispatcher selects
        every = BF16_NAMES if arg.only == "bf16" else set(ThinCase.T.INSTANTIATIONS)
        res["instantiations_not_launched"] = sorted(every - {r["kernel"] for r in rows if "parent" not in r})
        print("instantiations not launched:", res["instantiations_not_launched"])
        all_equal = all_equal and not res["instantiations_not_launched"]
    if arg.out:
        with open(arg.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res.get("wino4_sum_of_medians_ms", {})))
    print("all outputs and workspaces bitwise equal:", all_equal)
    return 1 if not all_equal else 0 if res.get("all_within_margin", True) else 2


if __name__ == "__main__":
    sys.exit(main())
