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

usage: python tools/wino_seat_ab.py NEW.so PARENT.so [name=OTHER.so ...] [--launches 20] [--out FILE] [--only wino4|wino2|up|bf16|thin]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vae-channel-dynamics_amd", "src"))
import torch  # noqa: E402
from vaehip import ops  # noqa: E402
from vaehip.lib import IgemmArgs, WgradArgs, lib  # noqa: E402

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
    for fn, res, argt in (("vae_igemm_rows", C.c_int, [ia, vp]), ("vae_wino_ok", C.c_int, [ia]), ("vae_wino_weight_floats", C.c_int64, [ia]),
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
        wu = torch.full((int(dll.vae_wino_weight_floats(C.byref(a))),), nan, device=dev)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="NEW.so PARENT.so [name=OTHER.so ...]")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=["", "wino4", "wino2", "up", "bf16", "thin"])
    arg = ap.parse_args()
    assert len(arg.libs) >= 2, "two libraries: this build and the parent's"
    names = ["new", "parent"] + [s.split("=", 1)[0] for s in arg.libs[2:]]
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
