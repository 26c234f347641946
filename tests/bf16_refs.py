"""Float64 restatements of the engine's bf16 blocks that round where the engine rounds (vaehip/engine.py, vaehip/ops.py).

r16() is round-to-nearest-even to bf16, bit for bit torch.Tensor.bfloat16() on an fp32 tensor.  It stands at every point where
the engine stores or reads a bf16 value; products are of rounded operands, every sum is float64.

One evaluator (Ev) serves three uses:
  free       Ev()                 runs a block and stores each result as the engine would (bf16 or fp32); it also keeps the record
                                  a recorder of the engine's ops-level calls would have taken;
  stand-in   Ev(acc=float32) /    the same with fp32 sums in torch's CPU order (a correct engine with another summation order), or
             Ev(off={...})        with ONE rounding point switched off or moved (a wrong engine): tests/test_bf16_blocks_host.py;
  forced     Ev(forced=record)    "teacher forcing": every stage is computed from the STORED values of the stages that the
                                  reference's wiring says feed it, taken from the record (the engine's, or a stand-in's), and the
                                  stored result of the stage is compared with the float64 value v before any storage rounding.
                                  A stage fed by the wrong tensor, a stale image or an unrounded operand disagrees with its v;
                                  a rounding flip upstream does not blur the stages after it.

Rounding points (name of the switch in Ev(off=...): what it is, and the line that makes it)
  act            the convolution's activation operand is bf16: the image bf16(SiLU(GN(x))) made once by ops.gn_apply_bf16
                 (engine.py:317-319, read again by the weight gradient through _take16, engine.py:436/440/448/452), a bf16-stored
                 tensor that is its own image (ops.py:582-583, 807-808), or an fp32 tensor rounded when the kernel stages it
                 (engine.py:89-90).  off: the forward reads the unrounded transformed tensor                       [mutant 1]
  weight         weights are read from the bf16 image of the parameter arena (engine.py:113-114, ops.py:32-37)  [mutant 2]
  wgrad_act      the weight gradient reads the same image as the forward (engine.py:371, ops.py:805-806)         [mutant 3]
  out_store      a conv output of >= ACT16_MIN_C channels is stored as bf16, rounded ONCE from conv + bias + residual
                 (ops.py:561, 610; the residual is brought to the output's storage first, ops.py:590, 608).
                 moved 'bias_late': rounded before the bias is added                                              [mutant 4]
                 moved 'res_late': the residual added after the rounding                                          [mutant 5]
  stats_stored   GroupNorm statistics describe the tensor AS STORED: the conv epilogue's partial sums are of the rounded values
                 (ops.py:613-619, 856-858; csrc/conv3_tile_bf16.hip:367, conv3_wide_bf16.hip:456); a re-stored result goes
                 without them (ops.py:603-604).  off: statistics of the unrounded output                         [mutant 6]
  dgrad_store    an input gradient is stored as bf16 with bf16 storage (ops.py:656, 700) or, with fp32 storage, when it only
                 feeds a GroupNorm backward and the halo-tile kernel can write it (engine.py:448/452 dx_to_gn, ops.py:672-674).
                 off: kept unrounded into the GroupNorm backward                                                  [mutant 7]
  gnbwd_store    the GroupNorm backward writes bf16 (engine.py:380-387 want32 / want16, ops.py:1046-1047), rounded once from
                 the fp32 sum with the residual-path gradient, which is brought to x's storage first (ops.py:1040-1041).
                 moved 'twice': rounded, added, rounded again                                                     [mutant 8]
  dh_operand     dL/dh reaches conv1's two backward kernels as the bf16 tensor / image (engine.py:451-452).
                 off: conv1's backward reads it unrounded                                                         [mutant 9]
  grad_image     fp32 storage: an fp32 output gradient gets its bf16 image `_b16` where the layer's kernels take one
                 (engine.py:363-367; ops.py:1062-1063 for a GroupNorm backward that continues the residual stream,
                 engine.py:386-387 feeds_conv3).  moved 'stale': the image of the other sample's gradient (bf16 storage: conv2's
                 backward reads the other sample's gradient)                                                      [mutant 10]
  x_store        the block input is stored as bf16 and the shortcut reads it as stored (engine.py:438).
                 off: the shortcut reads the fp32 value it was rounded from                                       [mutant 11]
  phase_weights  the upsampler's four 2x2 effective kernels are rounded after the fp32 taps are summed
                 (ops.py:434-438, 507).  moved 'per_tap': each tap rounded, then summed                           [mutant 12]
  add_store      ops.add of a bf16 and any tensor brings both to bf16 and rounds the fp32 sum once (ops.py:1217-1223)
  attn_operand   the attention products read bf16 images of q, k, v, dO while the tensors stay fp32 (ops.py:1109-1113,
                 engine.py:474-479); the materialised form's GEMMs round their fp32 operands when staged (ops.py:286-298).
                 Inside the blockwise kernels P and dS are rounded for the second products: covered by those kernels' bars
  exact          no rounding at all: a <= 4-channel contraction (post_quant_conv, quant_conv's dgrad) is served by the fp32
                 small-k kernels, which read the operands as stored (the kernel name says so; ops.py:596-605 keeps their storage fp32)

Storage regimes: act16 True is ops.ACT_BF16 = True (activations and their gradients bf16 from ACT16_MIN_C channels up); False
is fp32 storage with bf16 images attached (`_b16`, conv_only, feeds_conv3 run only there).

Blocks restated: ResnetBlock2D (with / without conv_shortcut), Attention (materialised and blockwise), Downsample2D,
Upsample2D (plain and phase form), _norm_act_conv, a plain convolution.

Criterion (ratio() <= 1): with v the float64 value before storage rounding and bar the serving kernel family's existing bar,
  fp32 result   max |got - v| <= bar max|v|
  bf16 result   every element |got - v| <= ulp_bf16(v) / 2 + bar max|v|,  ulp_bf16(v) = 2^(floor(log2 |v|) - 7)
  image         bit-equal to r16 of the fp32 tensor as stored
Bars: conv forward / dgrad 2e-5, weight gradient 3e-5, statistics 1e-5 (tests/conv_routes.py); GroupNorm transform 1e-5 and
GroupNorm backward 2e-5 (tests/test_norm_edges_gpu.py); an elementwise fp32 sum 2^-23 (one fp32 rounding); the attention
kernels' own (tests/test_attention_gpu.py) for what they compute internally.
"""
import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

BAR_DIRECT, BAR_WGRAD, BAR_WGRAD_GN, BAR_STATS = 2e-5, 3e-5, 5e-5, 1e-5   # tests/conv_routes.py
BAR_GN_APPLY, BAR_GN_BWD = 1e-5, 2e-5                                       # tests/test_norm_edges_gpu.py
BAR_ADD = 2.0 ** -23
# tests/test_attention_gpu.py: the blockwise kernels round P and dS to bf16 for their second products (o 4e-3, gradients 1e-2),
# the row log-sum-exp is exact products in fp32 (1e-5).  The materialised form's softmax kernels are elementwise fp32: an fp32
# exp at |x| <= 20 is good to about 1e-6 relative, the row sum adds 1e-7: 1e-5, the bar of the other elementwise kernels
BAR_ATTN_O, BAR_ATTN_G, BAR_ATTN_LSE, BAR_SOFTMAX = 4e-3, 1e-2, 1e-5, 1e-5
XF_NONE, XF_AFFINE, XF_AFFINE_SILU = 0, 1, 2
G, EPS = 32, 1e-6
ACT16_MIN_C = 32

SWITCHES = ("act", "weight", "wgrad_act", "out_store", "stats_stored", "dgrad_store", "gnbwd_store", "dh_operand", "grad_image",
            "x_store", "phase_weights", "add_store")


def r16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).bfloat16()


def ulp_bf16(v: torch.Tensor) -> torch.Tensor:
    """2^(floor(log2 |v|) - 7); the smallest normal's ulp below it"""
    a = v.double().abs()
    _, e = torch.frexp(a)      # |v| = m 2^e, m in [0.5, 1)
    e = torch.where(a > 0, e - 1, torch.full_like(e, -126))
    return torch.exp2(e.clamp_min(-126).double() - 7.0)


class Stage(NamedTuple):
    name: str
    op: str
    v: Optional[torch.Tensor]    # float64, before storage rounding (None: an image)
    got: torch.Tensor            # the stored result under test
    kind: str                    # f32 | bf16 | image
    bar: float
    of: Optional[torch.Tensor]   # image: the fp32 tensor it must be the rounding of
    scale: Optional[float] = None  # what `bar` is relative to when max|v| is no scale (a sum that cancels exactly: to_k's bias gradient)


def ratio(s: Stage) -> float:
    """worst |got - v| / allowed over every element (an image: 0 when bit-equal, else inf)"""
    if s.kind == "image":
        return 0.0 if torch.equal(s.got, r16(s.of)) else math.inf
    v = s.v.double()
    assert s.got.numel() == v.numel(), (s.name, tuple(s.got.shape), tuple(v.shape))   # (never a broadcast)
    err = (s.got.double().reshape(v.shape) - v).abs()
    allowed = torch.full_like(v, s.bar * (float(v.abs().max()) if s.scale is None else s.scale))
    if s.kind == "bf16":
        allowed = allowed + 0.5 * ulp_bf16(v)
    if not bool(torch.isfinite(err).all()):
        return math.inf
    bad = err > 0
    if not bool(bad.any()):
        return 0.0
    return float((err[bad] / allowed[bad]).max())


def bar_used(s: Stage) -> float:
    """the share of the `bar max|v|` term a stage uses: max (|got - v| - ulp / 2) / (bar max|v|) for a bf16 result (0 when one
    rounding explains every element), ratio() for an fp32 one.  A figure for the record: ratio() is what is asserted"""
    if s.kind == "image" or s.bar == 0.0:
        return 0.0
    v = s.v.double()
    err = (s.got.double().reshape(v.shape) - v).abs()
    if s.kind == "bf16":
        err = (err - 0.5 * ulp_bf16(v)).clamp_min(0.0)
    den = s.bar * (float(v.abs().max()) if s.scale is None else s.scale)
    return float(err.max() / den) if den > 0 else (0.0 if float(err.max()) == 0 else math.inf)


def worst(stages):
    """-> {stage name: ratio}"""
    return {s.name: ratio(s) for s in stages}


class Stats(NamedTuple):
    mean: torch.Tensor
    rstd: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def conv_nchw(x, w, kind):
    if kind == "c1":
        return F.conv2d(x, w)
    if kind == "c3s2":
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, None, 2, 0)
    if kind == "c3up":
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return F.conv2d(x, w, None, 1, 1)


def phase_weights(w, per_tap_round=False):
    """w [Co,Ci,3,3] -> the four effective kernels [4,Co,Ci,3,3] on the low-resolution grid: output parity (pa, pb) sees taps
    kh, kw of the 3x3 kernel land on low-resolution offsets floor((pa + kh - 1) / 2), floor((pb + kw - 1) / 2)"""
    we = torch.zeros((4,) + tuple(w.shape), dtype=w.dtype)
    for pa in (0, 1):
        for pb in (0, 1):
            for kh in range(3):
                for kw in range(3):
                    dh, dw = (pa + kh - 1) // 2, (pb + kw - 1) // 2
                    t = w[:, :, kh, kw]
                    we[pa * 2 + pb, :, :, dh + 1, dw + 1] += r16(t).to(w.dtype) if per_tap_round else t
    return we


def phase_conv_nchw(x, we):
    ys = [F.conv2d(x, we[p], None, 1, 1) for p in range(4)]
    B, Co, H, W = ys[0].shape
    y = torch.zeros(B, Co, 2 * H, 2 * W, dtype=x.dtype)
    for pa in (0, 1):
        for pb in (0, 1):
            y[:, :, pa::2, pb::2] = ys[pa * 2 + pb]
    return y


class Ev:
    """the stage evaluator.  Tensors are NHWC CPU tensors, stored as the engine stores them (fp32 or bf16); weights are the
    logical OIHW fp32 parameters.  device: forced mode on values a GPU made -- an object with gn_apply_bf16(x, st, xf) and
    upconv_phase_weights(w), the device's own transform / tap sums, whose rounding a kernel with a fused transform reads (a
    host transform would differ by one-ulp flips of single operands; tests/conv_routes.py does the same)."""

    def __init__(self, acc=torch.float64, forced=None, off=(), moved=None, device=None):
        self.acc = acc
        self.off = set(off)
        self.moved = dict(moved or {})
        assert self.off <= set(SWITCHES) and set(self.moved) <= set(SWITCHES)
        self.forced = list(forced) if forced is not None else None
        self.pos = 0
        self.device = device
        self.record = []
        self.stages = []
        self.unr = {}   # free mode: id(stored tensor) -> (stored tensor, its value before storage rounding)

    # ------------------------------------------------------------------ plumbing
    def _a(self, t):
        return t.to(self.acc)

    def _unrounded(self, t):
        e = self.unr.get(id(t))
        return self._a(e[1]) if e is not None else self._a(t)

    def _op16(self, t, switch="act", exact=False):
        """an operand of a product: rounded to bf16 (exact for a bf16-stored tensor).  exact: the launch is served by an fp32
        kernel (the <= 4-channel contractions, conv_smallk_kernel / wgrad_smallk_kernel), which reads the tensor as stored"""
        if exact:
            return self._a(t)
        if switch in self.off:
            return self._unrounded(t)
        return self._a(r16(t))

    def _w16(self, w, exact=False):
        return self._a(w) if ("weight" in self.off or exact) else self._a(r16(w))

    def _emit(self, name, op, parts, stored=None):
        """parts: [(sub name, v, kind, bar, of)] of one ops-level call -> the stored results (the record's in forced mode)"""
        if self.forced is not None:
            assert self.pos < len(self.forced), f"the record ends before {op} ({name}): {[e['op'] for e in self.forced]}"
            e = self.forced[self.pos]
            assert e["op"] == op, (f"call {self.pos}: the reference's wiring has {op} ({name}), the record {e['op']}: "
                                   f"{[x['op'] for x in self.forced]}")
            self.pos += 1
            outs = list(e["out"])
            assert len(outs) == len(parts), (name, len(outs), len(parts))
        else:
            outs = []
            for i, (sub, v, kind, bar, of) in enumerate(parts):
                if stored is not None and stored[i] is not None:
                    o = stored[i]
                elif kind == "image":
                    o = r16(of)
                else:
                    o = r16(v) if kind == "bf16" else v.to(torch.float32)
                outs.append(o)
                if v is not None:
                    self.unr[id(o)] = (o, v)
            self.record.append({"op": op, "out": tuple(outs)})
        for (sub, v, kind, bar, of), o in zip(parts, outs):
            want = torch.bfloat16 if kind in ("bf16", "image") else torch.float32
            assert o.dtype == want, f"{name}{sub}: stored as {o.dtype}, the reference's wiring stores {want}"
            self.stages.append(Stage(name + sub, op, None if v is None else v.double(), o, kind, bar, of))
        return outs

    def done(self):
        if self.forced is not None:
            assert self.pos == len(self.forced), f"calls the reference's wiring does not have: {[e['op'] for e in self.forced[self.pos:]]}"

    # ------------------------------------------------------------------ GroupNorm
    def gn_stats(self, name, x, gamma, beta):
        xs = self._unrounded(x) if "stats_stored" in self.off else self._a(x)
        B, H, W, C = xs.shape
        xg = xs.reshape(B, H * W, G, C // G)
        mean = xg.mean(dim=(1, 3))
        var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
        rstd = 1.0 / torch.sqrt(var + EPS)
        scale = self._a(gamma)[None, :] * rstd.repeat_interleave(C // G, dim=1)
        shift = self._a(beta)[None, :] - mean.repeat_interleave(C // G, dim=1) * scale
        o = self._emit(name, "gn_stats", [(".mean", mean, "f32", BAR_STATS, None), (".rstd", rstd, "f32", BAR_STATS, None),
                                          (".scale", scale, "f32", BAR_STATS, None), (".shift", shift, "f32", BAR_STATS, None)])
        return Stats(*o)

    def _xf(self, x, st, xf):
        y = self._a(x) * self._a(st.scale)[:, None, None, :] + self._a(st.shift)[:, None, None, :]
        return y * torch.sigmoid(y) if xf == XF_AFFINE_SILU else y

    def gn_apply_bf16(self, name, x, st, xf):
        """the activation image, a recorded call"""
        return self._emit(name, "gn_apply_bf16", [("", self._xf(x, st, xf), "bf16", BAR_GN_APPLY, None)])[0]

    def fused_act(self, name, x, st, xf):
        """the transform a kernel applies while it stages x (no recorded call): what it reads is the device's own transform
        rounded; on the host the float64 one"""
        v = self._xf(x, st, xf)
        if self.device is not None:
            got = self.device.gn_apply_bf16(x, st, xf)
            self.stages.append(Stage(name + "(on load)", "fused", v.double(), got, "bf16", BAR_GN_APPLY, None))
            return got
        if self.forced is not None:   # a stand-in's record carries what its kernel read
            e = self.forced[self.pos]
            assert e["op"] == "fused", (name, e["op"])
            self.pos += 1
            self.stages.append(Stage(name + "(on load)", "fused", v.double(), e["out"][0], "bf16", BAR_GN_APPLY, None))
            return e["out"][0]
        o = r16(v)
        self.unr[id(o)] = (o, v)
        self.record.append({"op": "fused", "out": (o,)})
        return o

    def gn_bwd(self, name, x, g, st, gamma, beta, silu, add, want32, want16):
        xa, ga = self._a(x), self._a(gamma)
        B, H, W, C = xa.shape
        cpg = C // G
        mean = self._a(st.mean).repeat_interleave(cpg, dim=1)[:, None, None, :]
        rstd = self._a(st.rstd).repeat_interleave(cpg, dim=1)[:, None, None, :]
        xhat = (xa - mean) * rstd
        y = xhat * ga + self._a(beta)
        du = self._unrounded(g) if "dgrad_store" in self.off else self._a(g)
        if silu:
            s = torch.sigmoid(y)
            du = du * (s * (1.0 + y * (1.0 - s)))
        dgamma, dbeta = (du * xhat).sum(dim=(0, 1, 2)), du.sum(dim=(0, 1, 2))
        dy = du * ga
        grp = lambda t: t.reshape(B, H * W, G, cpg).mean(dim=(1, 3)).repeat_interleave(cpg, dim=1)[:, None, None, :]  # noqa: E731
        dx = (dy - grp(dy) - xhat * grp(dy * xhat)) * rstd
        x16 = x.dtype == torch.bfloat16
        if add is not None:
            a = self._a(r16(add)) if (x16 and "add_store" not in self.off) else self._a(add)   # brought to x's storage
            if self.moved.get("gnbwd_store") == "twice" and self.forced is None:
                dx = self._a(r16(dx))
            dx = dx + a
        parts, stored = [], []
        if want32:
            parts.append((".dx", dx, "f32", BAR_GN_BWD, None))
            stored.append(None)
        if want16 and not want32:
            parts.append((".dx", dx, "bf16", BAR_GN_BWD, None))
            stored.append(None)
        parts += [(".dgamma", dgamma, "f32", BAR_GN_BWD, None), (".dbeta", dbeta, "f32", BAR_GN_BWD, None)]
        stored += [None, None]
        o = self._emit(name, "gn_bwd", parts, stored)
        dxs = o[0]
        img = None
        if want32 and want16:   # the image the same kernel writes next to the fp32 tensor
            img = self.image(name + ".dx._b16", dxs, op=None)
        return dxs, img, o[-2], o[-1]

    # ------------------------------------------------------------------ images and sums
    def image(self, name, t, op="pack_bf16", stale=False):
        """a bf16 image attached to the fp32 tensor t.  op None: written by the call that made t (no call of its own): the
        record carries it as that call's attachment"""
        st = None
        if stale and self.forced is None:
            st = [r16(t.flip(0))]
        if op is None:
            if self.forced is not None:
                got = self.forced[self.pos - 1].get("b16")
                assert got is not None, f"{name}: the record's call attached no image"
            else:
                got = st[0] if st else r16(t)
                self.record[-1]["b16"] = got
            self.stages.append(Stage(name, "attached", None, got, "image", 0.0, t))
            return got
        return self._emit(name, op, [("", None, "image", 0.0, t)], st)[0]

    def add(self, name, a, b):
        if a.dtype == torch.bfloat16 or b.dtype == torch.bfloat16:
            v = self._a(r16(a)) + self._a(r16(b))
            return self._emit(name, "add", [("", v, "bf16", BAR_ADD, None)])[0]
        return self._emit(name, "add", [("", self._a(a) + self._a(b), "f32", BAR_ADD, None)])[0]

    # ------------------------------------------------------------------ attention
    def gemm(self, name, op, A, Bm, alpha=1.0):
        """ops.gemm_nt / gemm_nn / gemm_tn in bf16 mode: fp32 tensors, rounded while the kernel stages them (ops.py:286-298)"""
        a, b = self._a(r16(A)), self._a(r16(Bm))
        if op == "gemm_nt":
            v, bar = alpha * (a @ b.transpose(1, 2)), BAR_DIRECT
        elif op == "gemm_nn":
            v, bar = alpha * (a @ b), BAR_DIRECT
        else:
            v, bar = alpha * (a.transpose(1, 2) @ b), BAR_WGRAD
        return self._emit(name, op, [("", v, "f32", bar, None)])[0]

    def softmax(self, name, S):
        return self._emit(name, "softmax_rows_", [("", torch.softmax(self._a(S), dim=-1), "f32", BAR_SOFTMAX, None)])[0]

    def softmax_bwd(self, name, P, dP):
        p, d = self._a(P), self._a(dP)
        return self._emit(name, "softmax_bwd_rows_", [("", p * (d - (p * d).sum(dim=-1, keepdim=True)), "f32", BAR_SOFTMAX, None)])[0]

    def _images(self, name, tensors, key):
        """bf16 images a call keeps of its fp32 operands (ops._attn_operand): the record carries them with the call"""
        if self.forced is not None:
            imgs = self.forced[self.pos - 1][key]
        else:
            imgs = tuple(r16(t) for t in tensors)
            self.record[-1][key] = imgs
        for i, (t, im) in enumerate(zip(tensors, imgs)):
            self.stages.append(Stage(f"{name}.image{i}", "attached", None, im, "image", 0.0, t))
        return imgs

    def attn_fwd(self, name, q, k, v, scale):
        """the blockwise forward on the bf16 images of q, k, v -> o, row log-sum-exp, the images (what the backward reads)"""
        qe, ke, ve = (self._a(r16(t)) for t in (q, k, v))
        s = scale * (qe @ ke.transpose(1, 2))
        o = torch.softmax(s, dim=-1) @ ve
        outs = self._emit(name, "attn_fwd", [(".o", o, "f32", BAR_ATTN_O, None), (".lse", torch.logsumexp(s, dim=-1), "f32", BAR_ATTN_LSE, None)])
        return outs[0], self._images(name, (q, k, v), "imgs")

    def attn_bwd(self, name, imgs, o, do, scale):
        qe, ke, ve = (self._a(t) for t in imgs)
        de = self._a(r16(do))
        p = torch.softmax(scale * (qe @ ke.transpose(1, 2)), dim=-1)
        dsum = (de * self._a(o)).sum(dim=-1, keepdim=True)          # D = rowsum(bf16(dO) * O), O as stored
        ds = p * (de @ ve.transpose(1, 2) - dsum)
        parts = [(".dq", scale * (ds @ ke), "f32", BAR_ATTN_G, None), (".dk", scale * (ds.transpose(1, 2) @ qe), "f32", BAR_ATTN_G, None),
                 (".dv", p.transpose(1, 2) @ de, "f32", BAR_ATTN_G, None)]
        return self._emit(name, "attn_bwd", parts)

    # ------------------------------------------------------------------ convolutions
    def _weights(self, w, kind, phase, exact=False):
        if not phase:
            return self._w16(w, exact)
        if self.device is not None:
            we = self.device.upconv_phase_weights(w)                      # the device's fp32 tap sums [4,Co,Ci,3,3] ...
            ref = phase_weights(w.double())
            self.stages.append(Stage("phase_weights(fp32 sums)", "phase", ref, we, "f32", 2 * BAR_ADD, None))
            return self._a(r16(we))                                        # ... rounded once
        if self.moved.get("phase_weights") == "per_tap" and self.forced is None:
            return self._a(phase_weights(w.to(torch.float32), per_tap_round=True))
        return self._a(r16(phase_weights(w.to(torch.float32))))

    def conv_fwd(self, name, act, w, bias, kind, res=None, out16=False, phase=False, ci=None, exact=False, switch="act"):
        """act: what the kernel reads -- an image, a bf16 tensor, or an fp32 tensor it rounds while staging"""
        a = _nchw(self._op16(act, switch, exact))
        if ci is not None:
            a = a[:, :ci]
        wk = self._weights(w, kind, phase, exact)
        y = _nhwc(phase_conv_nchw(a, wk) if phase else conv_nchw(a, wk, kind))
        r = None
        if res is not None:   # brought to the output's storage first
            r = self._a(r16(res)) if out16 else self._a(res)
        stored = None
        mv = self.moved.get("out_store") if self.forced is None else None
        if bias is not None:
            b = self._a(bias)
            if mv == "bias_late" and out16:
                stored = [r16(self._a(r16(y)) + b + (r if r is not None else 0.0))]
            y = y + b
        if r is not None:
            if mv == "res_late" and out16:
                stored = [r16(self._a(r16(y)) + r)]
            y = y + r
        o = self._emit(name, "conv_fwd", [("", y, "bf16" if out16 else "f32", BAR_DIRECT, None)], stored)[0]
        if self.forced is not None and self.forced[self.pos - 1].get("x_b16") is not None:   # an image the call attached to its fp32 input
            self.stages.append(Stage(name + ".x._b16", "attached", None, self.forced[self.pos - 1]["x_b16"], "image", 0.0, act))
        return o

    def conv_dgrad(self, name, dy, w, kind, in_shape, out16=False, phase=False, switch=None, exact=False):
        d = _nchw(self._op16(dy, switch, exact))
        wk = self._weights(w, kind, phase, exact)
        x0 = torch.zeros(in_shape[0], in_shape[3], in_shape[1], in_shape[2], dtype=self.acc, requires_grad=True)
        y = phase_conv_nchw(x0, wk) if phase else conv_nchw(x0, wk, kind)
        (gx,) = torch.autograd.grad(y, x0, d)
        return self._emit(name, "conv_dgrad", [("", _nhwc(gx), "bf16" if out16 else "f32", BAR_DIRECT, None)])[0]

    def conv_wgrad(self, name, dy, act, w_shape, kind, bias=True, dy_rounded_for_bias=True, switch=None, ci=None, xf=False, exact=False, db_scale=None):
        """dW = sum of products of the rounded operands; db = sums of dY as the kernel reads it (the rounded values where it
        reads a bf16 tensor or image, the fp32 tensor as given otherwise)"""
        d = _nchw(self._op16(dy, switch, exact))
        a = _nchw(self._unrounded(act) if "wgrad_act" in self.off else self._a(act if exact else r16(act)))
        if ci is not None:
            a = a[:, :ci]
        w0 = torch.zeros(w_shape, dtype=self.acc, requires_grad=True)
        (gw,) = torch.autograd.grad(conv_nchw(a, w0, kind), w0, d)
        parts = [(".dW", gw, "f32", BAR_WGRAD_GN if xf else BAR_WGRAD, None)]
        if bias:
            src = d if (dy_rounded_for_bias or switch in self.off) else _nchw(self._a(dy))
            parts.append((".db", src.sum(dim=(0, 2, 3)), "f32", BAR_WGRAD, None))
        o = self._emit(name, "conv_wgrad", parts)
        if bias and db_scale is not None:
            self.stages[-1] = self.stages[-1]._replace(scale=db_scale)
        return o[0], (o[1] if bias else None)


# ---------------------------------------------------------------------------------------------------- blocks
class ResnetCfg(NamedTuple):
    act16: bool               # storage regime
    img1: bool                # ops.act_image_ok for conv1 / conv2: the activation image is made
    img2: bool
    gimg1: bool               # ops.grad_image_ok for conv1 / conv2
    gimg2: bool
    gimg_x: bool              # ops.grad_image_ok("c3", x.shape, C, C): feeds_conv3's question
    g16: bool = True          # fp32 storage: the halo-tile dgrad writes the gradient that only feeds a GroupNorm backward as bf16
    after_conv3: bool = False
    live_in: bool = True


def resnet(E: Ev, P: dict, x, dout, c: ResnetCfg, x_pre=None):
    """engine.py:_resnet, forward and backward.  P: norm1.weight ... conv_shortcut.bias (conv_shortcut.* absent without one).
    x_pre: the fp32 value x was rounded from (only the x_store switch reads it).  -> {name: stage name} of the block's results"""
    short = "conv_shortcut.weight" in P
    Co = P["conv1.weight"].shape[0]
    o16 = c.act16 and Co >= ACT16_MIN_C
    i16 = c.act16 and x.shape[3] >= ACT16_MIN_C
    # ---- forward (engine.py:434-440)
    st1 = E.gn_stats("st1", x, P["norm1.weight"], P["norm1.bias"])
    a1 = (E.gn_apply_bf16 if c.img1 else E.fused_act)("a1", x, st1, XF_AFFINE_SILU)
    h = E.conv_fwd("h", a1, P["conv1.weight"], P["conv1.bias"], "c3", out16=o16)
    st2 = E.gn_stats("st2", h, P["norm2.weight"], P["norm2.bias"])
    if short:
        xs = x
        if "x_store" in E.off and x_pre is not None:
            xs = x_pre.to(torch.float32)
            E.unr[id(xs)] = (xs, x_pre)
        sc = E.conv_fwd("sc", xs, P["conv_shortcut.weight"], P["conv_shortcut.bias"], "c1", out16=o16, switch="x_store")
    else:
        sc = x
    a2 = (E.gn_apply_bf16 if c.img2 else E.fused_act)("a2", h, st2, XF_AFFINE_SILU)
    out = E.conv_fwd("out", a2, P["conv2.weight"], P["conv2.bias"], "c3", res=sc, out16=o16)
    # ---- backward (engine.py:447-463)
    stale = E.moved.get("grad_image") == "stale"
    d2 = dout
    if dout.dtype == torch.float32 and c.gimg2:     # engine.py:363-367
        d2 = E.image("dout._b16", dout, stale=stale)
    elif stale and E.forced is None:
        d2 = dout.flip(0)
    img2 = d2.dtype == torch.bfloat16
    E.conv_wgrad("conv2", d2, a2, P["conv2.weight"].shape, "c3", dy_rounded_for_bias=img2, xf=not c.img2)
    g16 = c.act16 or c.g16
    g2 = E.conv_dgrad("g2", d2, P["conv2.weight"], "c3", h.shape, out16=g16)
    dh16 = c.act16 or c.gimg1                      # engine.py:381-385 (conv_only)
    dh, _, _, _ = E.gn_bwd("norm2", h, g2, st2, P["norm2.weight"], P["norm2.bias"], True, None, not dh16, dh16)
    sw = "dh_operand"
    E.conv_wgrad("conv1", dh, a1, P["conv1.weight"].shape, "c3", dy_rounded_for_bias=dh16, switch=sw, xf=not c.img1)
    g1 = E.conv_dgrad("g1", dh, P["conv1.weight"], "c3", x.shape, out16=g16, switch=sw)
    if short:   # dout as given: a 1x1 layer takes no gradient image (ops.grad_image_ok), the kernel rounds what it stages
        E.conv_wgrad("conv_shortcut", dout, x, P["conv_shortcut.weight"].shape, "c1", dy_rounded_for_bias=dout.dtype == torch.bfloat16)
        dsc = E.conv_dgrad("dsc", dout, P["conv_shortcut.weight"], "c1", x.shape, out16=i16) if c.live_in else None
    else:
        dsc = dout
    want16 = c.act16 or (c.after_conv3 and c.gimg_x)   # engine.py:381-387
    E.gn_bwd("norm1", x, g1, st1, P["norm1.weight"], P["norm1.bias"], True, dsc, not c.act16, want16)
    E.done()
    res = {"out": "out"}
    if c.live_in:
        res["dx"] = "norm1.dx"
    for n, s in (("norm1.weight", "norm1.dgamma"), ("norm1.bias", "norm1.dbeta"), ("norm2.weight", "norm2.dgamma"), ("norm2.bias", "norm2.dbeta"),
                 ("conv1.weight", "conv1.dW"), ("conv1.bias", "conv1.db"), ("conv2.weight", "conv2.dW"), ("conv2.bias", "conv2.db")):
        res[n] = s
    if short:
        res["conv_shortcut.weight"], res["conv_shortcut.bias"] = "conv_shortcut.dW", "conv_shortcut.db"
    return res


class AttnCfg(NamedTuple):
    act16: bool
    blockwise: bool
    live_in: bool = True


def attention(E: Ev, P: dict, x, dout, c: AttnCfg):
    """engine.py:_attention.  The three projections read the same GroupNorm output (one transform of x, rounded when staged);
    q, k, v, scores, context and their gradients are stored fp32 (engine.py:474-479) and rounded for every product."""
    B, H, W, C = x.shape
    T, scale = H * W, float(C) ** -0.5
    f3 = lambda t: t.reshape(B, T, C)        # noqa: E731
    f4 = lambda t: t.reshape(B, H, W, C)     # noqa: E731
    st = E.gn_stats("st", x, P["group_norm.weight"], P["group_norm.bias"])
    a = E.fused_act("a", x, st, XF_AFFINE)
    q, k, v = (E.conv_fwd(n, a, P[f"to_{n}.weight"][:, :, None, None], P[f"to_{n}.bias"], "c1") for n in "qkv")
    if c.blockwise:
        o, imgs = E.attn_fwd("attn", f3(q), f3(k), f3(v), scale)
    else:
        Pm = E.softmax("P", E.gemm("S", "gemm_nt", f3(q), f3(k), scale))
        o = E.gemm("o", "gemm_nn", Pm, f3(v))
    o16 = c.act16 and C >= ACT16_MIN_C
    E.conv_fwd("out", f4(o), P["to_out.0.weight"][:, :, None, None], P["to_out.0.bias"], "c1", res=x, out16=o16)
    # ---- backward (engine.py:502-528)
    wshape = (C, C, 1, 1)
    d16 = dout.dtype == torch.bfloat16
    E.conv_wgrad("to_out.0", dout, f4(o), wshape, "c1", dy_rounded_for_bias=d16)
    do = f3(E.conv_dgrad("do", dout, P["to_out.0.weight"][:, :, None, None], "c1", x.shape))
    if c.blockwise:
        dq, dk, dv = E.attn_bwd("attn_bwd", imgs, o, do, scale)
    else:
        dP = E.gemm("dP", "gemm_nt", do, f3(v))
        dv = E.gemm("dv", "gemm_tn", Pm, do)
        dS = E.softmax_bwd("dS", Pm, dP)
        dq = E.gemm("dq", "gemm_nn", dS, f3(k), scale)
        dk = E.gemm("dk", "gemm_tn", dS, f3(q), scale)
    gs = []
    qscale = None
    for n, d in (("q", dq), ("k", dk), ("v", dv)):
        # to_k's bias gradient, the column sums of dk, is zero in exact arithmetic (a shift of every score of a row leaves the
        # softmax alone), so its own maximum is no scale: it is held on the scale of to_q's, the same sums over dq
        # (tests/test_attention_gpu.py does the same)
        E.conv_wgrad(f"to_{n}", f4(d), a, wshape, "c1", dy_rounded_for_bias=False, xf=True, db_scale=qscale if n == "k" else None)
        if n == "q":
            qscale = float(E.stages[-1].v.abs().max())
        gs.append(E.conv_dgrad(f"g{n}", f4(d), P[f"to_{n}.weight"][:, :, None, None], "c1", x.shape))
    g = E.add("g", E.add("gqk", gs[0], gs[1]), gs[2])
    E.gn_bwd("norm", x, g, st, P["group_norm.weight"], P["group_norm.bias"], False, dout, not c.act16, c.act16)
    E.done()
    res = {"out": "out", "group_norm.weight": "norm.dgamma", "group_norm.bias": "norm.dbeta", "to_out.0.weight": "to_out.0.dW", "to_out.0.bias": "to_out.0.db"}
    for n in "qkv":
        res[f"to_{n}.weight"], res[f"to_{n}.bias"] = f"to_{n}.dW", f"to_{n}.db"
    if c.live_in:
        res["dx"] = "norm.dx"
    return res


class ConvCfg(NamedTuple):
    act16: bool = True
    kind: str = "c3"
    need_dx: bool = True
    live_in: bool = True
    phase_fwd: bool = False    # an upsampler served by the four phase convolutions (4 launches) / by the virtual-upsample kernel (1)
    phase_dgrad: bool = False
    db_rounded: bool = True    # the bias gradient sums the ROUNDED dY: a bf16 dY, or images made for the kernel (ops.py:731-737)
    exact: tuple = (False, False, False)  # forward / weight gradient / dgrad served by an fp32 kernel: operands as stored


def plain_conv(E: Ev, P: dict, x, dout, c: ConvCfg):
    """engine.py:_plain_conv (conv_in, quant_conv, post_quant_conv, the samplers' convolutions)"""
    w, b = P["weight"], P["bias"]
    Co, Ci = w.shape[0], w.shape[1]
    o16 = c.act16 and Co >= ACT16_MIN_C
    E.conv_fwd("y", x, w, b, c.kind, out16=o16, phase=c.phase_fwd, ci=Ci, exact=c.exact[0])
    E.conv_wgrad("conv", dout, x, w.shape, c.kind, dy_rounded_for_bias=c.db_rounded, ci=Ci, exact=c.exact[1])
    res = {"out": "y", "weight": "conv.dW", "bias": "conv.db"}
    if c.need_dx and c.live_in:
        E.conv_dgrad("dx", dout, w, c.kind, x.shape[:3] + (Ci,), out16=c.act16 and Ci >= ACT16_MIN_C, phase=c.phase_dgrad,
                     exact=c.exact[2])
        res["dx"] = "dx"
    E.done()
    return res


class TailCfg(NamedTuple):
    act16: bool
    img: bool       # ops.act_image_ok
    gimg: bool      # ops.grad_image_ok for the convolution
    gimg_x: bool    # ops.grad_image_ok("c3", x.shape, C, C)
    g16: bool = False


def norm_act_conv(E: Ev, P: dict, x, dout, c: TailCfg):
    """engine.py:_norm_act_conv: conv_norm_out + SiLU + conv_out.  P: norm.weight, norm.bias, conv.weight, conv.bias"""
    Co, Ci = P["conv.weight"].shape[:2]
    st = E.gn_stats("st", x, P["norm.weight"], P["norm.bias"])
    a = (E.gn_apply_bf16 if c.img else E.fused_act)("a", x, st, XF_AFFINE_SILU)
    E.conv_fwd("y", a, P["conv.weight"], P["conv.bias"], "c3", out16=c.act16 and Co >= ACT16_MIN_C)
    d = dout
    if dout.dtype == torch.float32 and c.gimg:
        d = E.image("dout._b16", dout)
    E.conv_wgrad("conv", d, a, P["conv.weight"].shape, "c3", dy_rounded_for_bias=d.dtype == torch.bfloat16, xf=not c.img)
    g = E.conv_dgrad("g", d, P["conv.weight"], "c3", x.shape, out16=(c.act16 and Ci >= ACT16_MIN_C) or c.g16)
    want16 = c.act16 or c.gimg_x
    E.gn_bwd("norm", x, g, st, P["norm.weight"], P["norm.bias"], True, None, not c.act16, want16)
    E.done()
    return {"out": "y", "dx": "norm.dx", "norm.weight": "norm.dgamma", "norm.bias": "norm.dbeta", "conv.weight": "conv.dW", "conv.bias": "conv.db"}


# ---------------------------------------------------------------------------------------------------- recording the engine
RECORDED = ("gn_stats", "gn_apply_bf16", "gn_apply", "conv_fwd", "conv_dgrad", "conv_wgrad", "gn_bwd", "pack_bf16", "add",
            "gemm_nt", "gemm_nn", "gemm_tn", "softmax_rows_", "softmax_bwd_rows_", "attn_fwd", "attn_bwd")


class OpsRecorder:
    """every ops-level call a block makes (the outermost ones: a call made inside another recorded call belongs to it), with the
    tensors coming out, frozen at the time of the call, and the `_b16` / `_gstat` attachments.  The route is not changed: the
    wrappers pass everything through (no forward hooks, which would change fuse_res and the image decisions).  values False: a
    dry run, only the sequence of calls is kept."""

    def __init__(self, ops, values=True):
        self.ops, self.values, self.calls, self.depth = ops, values, [], 0

    def _keep(self, t):
        if t is None or not self.values:
            return t
        return t.detach().clone()

    def _entry(self, name, a, kw, out):
        if name == "gn_stats":
            outs = tuple(out)
        elif name == "pack_bf16":
            outs = (a[1],)
        elif name == "conv_wgrad":
            outs = (a[3],) + ((a[4],) if a[4] is not None else ())
        elif name == "gn_bwd":
            outs = (out, a[7], a[8])
        elif name == "attn_fwd":
            outs = (out[0], out[1][3])
        elif name == "attn_bwd":
            outs = tuple(out)
        else:
            outs = (out,)
        e = {"op": name, "out": tuple(self._keep(t) for t in outs)}
        if name == "gn_bwd" and out.dtype == torch.float32 and getattr(out, "_b16", None) is not None:
            e["b16"] = self._keep(out._b16)
        if name == "attn_fwd":
            e["imgs"] = tuple(self._keep(t) for t in out[1][:3])
        if name == "conv_fwd":
            e["gstat"] = hasattr(out, "_gstat")
            if a[0].dtype == torch.float32 and getattr(a[0], "_b16", None) is not None:
                e["x_b16"] = self._keep(a[0]._b16)
        return e

    def __enter__(self):
        self._orig = {n: getattr(self.ops, n) for n in RECORDED}

        def wrap(name, fn):
            def w(*a, **kw):
                self.depth += 1
                try:
                    out = fn(*a, **kw)
                finally:
                    self.depth -= 1
                if self.depth == 0:
                    self.calls.append(self._entry(name, a, kw, out))
                return out
            return w

        for n, fn in self._orig.items():
            setattr(self.ops, n, wrap(n, fn))
        return self

    def __exit__(self, *exc):
        for n, fn in self._orig.items():
            setattr(self.ops, n, fn)
        return False

    def record(self):
        """the calls with every tensor on the host"""
        mv = lambda t: None if t is None else t.cpu()  # noqa: E731
        return [{k: (tuple(mv(t) for t in v) if k in ("out", "imgs") else (mv(v) if isinstance(v, torch.Tensor) else v)) for k, v in e.items()}
                for e in self.calls]


# ---------------------------------------------------------------------------------------------------- the cases
class Case(NamedTuple):
    id: str
    block: str          # resnet | up | down | tail | conv | attn
    module: str         # attribute path below the VAE (tail: the encoder / decoder that owns conv_norm_out and conv_out)
    shape: tuple        # B, H, W of the block's input
    arm: str
    names: tuple        # kernel names of the block's launches in order (ops.LaunchProfiler / the argument blocks), pinned
    act16: bool = True
    after_conv3: bool = False
    live_in: bool = True
    need_dx: bool = True
    small: bool = True  # the host module evaluates it a second time


def contrast(vae, seed=11):
    """gamma, beta with some spread and q / k weights that give the softmax contrast (the synthetic init has gamma = 1,
    beta = 0 and nearly uniform attention), in place -> a function that puts the old values back"""
    import torch.nn as nn
    gen = torch.Generator().manual_seed(seed)
    old = []
    with torch.no_grad():
        for name, m in vae.named_modules():
            if isinstance(m, nn.GroupNorm):
                for p, v in ((m.weight, 1.0 + 0.3 * torch.randn(m.weight.shape, generator=gen)), (m.bias, 0.2 * torch.randn(m.bias.shape, generator=gen))):
                    old.append((p, p.detach().clone()))
                    p.copy_(v.to(p.device))
            elif name.endswith(("to_q", "to_k")):
                old.append((m.weight, m.weight.detach().clone()))
                m.weight.mul_(6.0)

    def restore():
        with torch.no_grad():
            for p, v in old:
                p.copy_(v)
    return restore


def module_of(vae, path):
    m = vae
    for p in path.split("."):
        m = m[int(p)] if p.isdigit() else getattr(m, p)
    return m


def params_of(case, vae):
    """{name: fp32 CPU tensor (a conv weight as logical OIHW)} in the reference's names, and {name: nn.Parameter}"""
    m = module_of(vae, case.module)
    if case.block == "tail":
        named = {"norm.weight": m.conv_norm_out.weight, "norm.bias": m.conv_norm_out.bias, "conv.weight": m.conv_out.weight, "conv.bias": m.conv_out.bias}
    elif case.block in ("up", "down"):
        named = {"weight": m.conv.weight, "bias": m.conv.bias}
    else:
        named = dict(m.named_parameters())
    return {n: p.detach().float().cpu().contiguous() for n, p in named.items()}, named


def _seed(case):
    import zlib
    return zlib.crc32(case.id.encode()) & 0x7FFFFFFF


def conv_of(case, vae):
    m = module_of(vae, case.module)
    return m.conv if case.block in ("up", "down") else m


def inputs_of(case, vae, ops):
    """-> x_pre (fp32), x (as stored in the regime), dout (as stored): NHWC CPU tensors"""
    gen = torch.Generator().manual_seed(_seed(case))
    B, H, W = case.shape
    m = module_of(vae, case.module)
    if case.block == "attn":
        ci, co, (Ho, Wo), cs = 512, 512, (H, W), None
    elif case.block == "resnet":
        ci, co, (Ho, Wo), cs = m.conv1.weight.shape[1], m.conv2.weight.shape[0], (H, W), None
    elif case.block == "tail":
        ci, co, (Ho, Wo), cs = m.conv_out.weight.shape[1], m.conv_out.weight.shape[0], (H, W), None
    else:
        cv = conv_of(case, vae)
        ci, co, cs = cv.weight.shape[1], cv.weight.shape[0], None
        Ho, Wo = ops.out_hw(getattr(cv, "kind", "c1"), H, W)
        if ci == 3:
            cs = 4   # the image is stored with a zero fourth channel (ops.nchw_to_nhwc(pv, 4))
    x_pre = torch.randn(B, H, W, ci, generator=gen) * 1.2 + 0.1
    if cs:
        x_pre = F.pad(x_pre, (0, cs - ci))
    dout = torch.randn(B, Ho, Wo, co, generator=gen)
    x = r16(x_pre) if (case.act16 and ci >= ACT16_MIN_C) else x_pre
    dout = r16(dout) if (case.act16 and co >= ACT16_MIN_C) else dout
    return x_pre, x, dout


class Bf16Queries:
    """ops.act_image_ok / grad_image_ok as bf16 mode answers them (pure library queries: no GPU needed)"""

    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        ops = self.ops
        self.keep = (ops.PRECISION, ops.WEIGHTS16)
        ops.PRECISION = ops.PREC_BF16
        if ops.WEIGHTS16 is None:
            ops.WEIGHTS16 = (0, 0, 0)
        return self

    def __exit__(self, *exc):
        self.ops.PRECISION, self.ops.WEIGHTS16 = self.keep
        return False


def cfg_of(case, vae, ops):
    """the reference's configuration of a case from the library's own queries"""
    B, H, W = case.shape
    m = module_of(vae, case.module)
    if case.block == "attn":
        return AttnCfg(act16=case.act16, blockwise="blockwise" in case.id, live_in=case.live_in)
    with Bf16Queries(ops):
        if case.block == "resnet":
            ci, co = m.conv1.weight.shape[1], m.conv1.weight.shape[0]
            return ResnetCfg(act16=case.act16, img1=ops.act_image_ok("c3", (B, H, W, ci), co, ci), img2=ops.act_image_ok("c3", (B, H, W, co), co, co),
                             gimg1=ops.grad_image_ok("c3", (B, H, W, ci), co, ci), gimg2=ops.grad_image_ok("c3", (B, H, W, co), co, co),
                             gimg_x=ops.grad_image_ok("c3", (B, H, W, ci), ci, ci), g16=ops.grad_image_ok("c3", (B, H, W, co), co, co),
                             after_conv3=case.after_conv3, live_in=case.live_in)
        if case.block == "tail":
            co, ci = m.conv_out.weight.shape[:2]
            return TailCfg(act16=case.act16, img=ops.act_image_ok("c3", (B, H, W, ci), co, ci), gimg=ops.grad_image_ok("c3", (B, H, W, ci), co, ci),
                           gimg_x=ops.grad_image_ok("c3", (B, H, W, ci), ci, ci))
    cv = conv_of(case, vae)
    kind = getattr(cv, "kind", "c1")
    # an upsampler's route shows in its launches: four phase convolutions, or one launch of the virtual-upsample kernel
    nf = sum(1 for n in case.names if n.startswith(("conv3_", "igemm_", "conv_")))
    fwd4 = kind == "c3up" and nf in (5, 8)
    dg4 = kind == "c3up" and nf == 8
    _, _, dout = inputs_of(case, vae, ops)
    wg = [n for n in case.names if n.startswith("wgrad")]
    dbr = dout.dtype == torch.bfloat16 or any(n.startswith("wgrad3_dma_bf16") or (n.startswith("wgrad3_tile_bf16") and n.endswith(",true>")) for n in wg)
    rows = [n for n in case.names if not n.startswith("wgrad")]
    exact = ("bf16" not in rows[0], "bf16" not in wg[0], len(rows) > 1 and "bf16" not in rows[-1])
    return ConvCfg(act16=case.act16, kind=kind, need_dx=case.need_dx, live_in=case.live_in, phase_fwd=fwd4, phase_dgrad=dg4, db_rounded=dbr,
                   exact=exact)


def reference(E: Ev, case, cfg, P, x_pre, x, dout):
    if case.block == "resnet":
        return resnet(E, P, x, dout, cfg, x_pre=x_pre)
    if case.block == "tail":
        return norm_act_conv(E, P, x, dout, cfg)
    if case.block == "attn":
        return attention(E, P, x, dout, cfg)
    return plain_conv(E, P, x, dout, cfg)


def run_engine_block(case, vae, ops, x, dout, gbuf):
    """the engine's own block on device (or dry-run) tensors, under the caller's _mode(): forward with a tape, then run_tape
    -> (out, dx)"""
    eng = vae.engine
    m = module_of(vae, case.module)
    tape = []
    eng._sync_trainable()
    eng._live = case.live_in
    min_t = ops.ATTN_BLOCKWISE_MIN_T
    try:
        if case.block == "attn":
            ops.ATTN_BLOCKWISE_MIN_T = 64 if "blockwise" in case.id else min_t
            out = eng._attention(m, x, tape, notify=False, after_conv3=case.after_conv3)
        elif case.block == "resnet":
            out = eng._resnet(m, x, tape, notify=False, after_conv3=case.after_conv3)
        elif case.block == "tail":
            out = eng._norm_act_conv(m, x, tape)
        elif case.block in ("up", "down"):
            out = eng._sampler(m, x, tape)
        else:
            out = eng._plain_conv(m, x, tape, need_dx=case.need_dx)
    finally:
        eng._live = True
        ops.ATTN_BLOCKWISE_MIN_T = min_t
    dx = eng.run_tape(tape, dout, gbuf)
    return out, dx


def dry_run(case, vae, ops, lib):
    """the engine's block without a GPU, as tests/conv_routes.py runs a conv call: the real library answers every dispatch
    query, nothing is launched, values are never read -> (kernel names in launch order, the sequence of ops-level calls)"""
    import conv_routes as cr
    _, x, dout = inputs_of(case, vae, ops)
    eng = vae.engine
    keep = (eng.precision, ops.ACT_BF16)
    rec = cr.Recorder(ops, lib, True)
    chk = ops._chk_c
    ops._chk_c = lambda t, name: None   # (the attention wrappers' storage check: dry tensors live on the host)
    try:
        with rec:
            eng.set_precision("bf16")
            ops.ACT_BF16 = case.act16
            with eng._mode():
                with OpsRecorder(ops, values=False) as orec:
                    run_engine_block(case, vae, ops, x, dout, torch.zeros_like(vae.arena.grad))
    finally:
        eng.precision, ops.ACT_BF16, ops._chk_c = *keep, chk
    return tuple(rec.names), [e["op"] for e in orec.calls]


# kernel names as the argument blocks give them (ops._kernel_name: what ops.LaunchProfiler records)
_FLAT, _FLAT_D, _FLAT_XF = "igemm_rows_bf16_kernel<128,128,4,2,false,0>", "igemm_rows_bf16_kernel<128,128,4,2,true,0>", "igemm_rows_bf16_kernel<128,128,4,2,false,2>"
_WG2, _WG0 = "wgrad_bf16_kernel<128,128,4,2,2>", "wgrad_bf16_kernel<128,128,4,2,0>"
_TILE, _TILE_D, _DMA = "conv3_tile_bf16_kernel<false,false,0,true>", "conv3_tile_bf16_kernel<true,false,0,true>", "wgrad3_dma_bf16_kernel<false,1>"
_WIDE, _WIDE_D = "conv3_wide_bf16_kernel<false,3>", "conv3_wide_bf16_kernel<true,3>"
_HALO = (_TILE, _TILE, _DMA, _TILE_D, _DMA, _TILE_D)
_HALO_SC = (_TILE, _FLAT, _TILE, _DMA, _TILE_D, _DMA, _TILE_D, _WG0, _FLAT_D)
_UP = "decoder.up_blocks.2.upsamplers.0"   # (the model's upsamplers keep their width: 512, 512 and 256 channels; the 256-channel
#                                             one has the tile counts of the 128 -> 256 layer at the same map: Co / 128 = 2)
_DOWN = "encoder.down_blocks.0.downsamplers.0"

# Smallest shapes that take each arm, re-derived with the library's queries (tests/test_bf16_blocks_host.py holds every one).
# With bf16 storage a bf16 x is refused by the halo-tile phase kernels (ops.py:499), so the upsampler below 192 wide tiles runs
# the virtual-upsample kernel forward and in the dgrad, and phases only in the weight gradient; the halo-tile phases serve fp32
# storage, where the case for them is.
CASES = [
    Case("resnet-flat-512", "resnet", "encoder.mid_block.resnets.0", (2, 8, 8), "flat bf16 kernels; the transform is materialised (64 pixels per image)",
         (_FLAT, _FLAT, _WG2, _FLAT_D, _WG2, _FLAT_D)),
    Case("resnet-ragged-256-128", "resnet", "decoder.up_blocks.3.resnets.0", (1, 5, 7), "flat bf16 kernels, ragged map, shortcut, transform fused on load",
         (_FLAT_XF, _FLAT, _FLAT_XF, _WG2, _FLAT_D, _WG2, _FLAT_D, _WG0, _FLAT_D)),
    Case("resnet-halo-128", "resnet", "encoder.down_blocks.0.resnets.0", (2, 8, 32), "128-pixel halo-tile kernels", _HALO, after_conv3=True),
    Case("resnet-halo-128-256", "resnet", "encoder.down_blocks.1.resnets.0", (1, 8, 64), "128-pixel halo-tile kernels, shortcut", _HALO_SC),
    Case("resnet-wide-128", "resnet", "encoder.down_blocks.0.resnets.0", (4, 128, 96),
         "192 tiles: conv1 and both dgrads on the wide kernel; conv2 with its residual on a 128-channel contraction stays on the 128-pixel kernel",
         (_WIDE, _TILE, _DMA, _WIDE_D, _DMA, _WIDE_D), small=False),
    Case("resnet-wide-256", "resnet", "encoder.down_blocks.1.resnets.1", (3, 64, 128),
         "conv2 with residual on the wide kernel: bf16 residual, bf16 output, statistics epilogue", (_WIDE, _WIDE, _DMA, _WIDE_D, _DMA, _WIDE_D), small=False),
    Case("resnet-halo-128-f32store", "resnet", "encoder.down_blocks.0.resnets.0", (2, 8, 32), "halo-tile kernels, fp32 storage: image attachments, feeds_conv3",
         _HALO, act16=False, after_conv3=True),
    Case("resnet-halo-128-256-f32store", "resnet", "encoder.down_blocks.1.resnets.0", (1, 8, 64), "halo-tile kernels, fp32 storage, shortcut, input gradient not wanted",
         _HALO_SC[:-1], act16=False, live_in=False),
    Case("up-halo", "up", _UP, (2, 4, 32), "bf16 storage below 192 wide tiles: virtual-upsample kernel, phase weight gradient",
         ("conv3_tile_bf16_kernel<false,true,0,true>",) + (_DMA,) * 4 + (_TILE_D,)),
    Case("up-halo-f32store", "up", _UP, (2, 4, 32), "halo-tile phases (fp32 storage)",
         ("conv3_tile_bf16_kernel<false,false,0,false>",) * 4 + (_DMA,) * 4 + ("conv3_tile_bf16_kernel<true,false,0,false>",) * 4, act16=False),
    Case("up-ragged", "up", _UP, (1, 5, 6), "ragged map: flat kernels", (_FLAT, _WG0, _FLAT_D)),
    Case("up-7", "up", _UP, (7, 32, 64), "just below 192 wide tiles in the forward (112); its dgrad has 224",
         ("conv3_tile_bf16_kernel<false,true,0,true>",) + (_DMA,) * 4 + (_WIDE_D,)),
    Case("up-13", "up", _UP, (13, 32, 64), "wide-tile phases (208 tiles)",
         ("conv3_wide_bf16_kernel<false,2>",) * 4 + (_DMA,) * 4 + ("conv3_wide_bf16_kernel<true,2>",) * 4, small=False),
    Case("down-16", "down", _DOWN, (2, 16, 16), "stride 2, parity-class dgrad", (_FLAT, _WG0, _FLAT_D)),
    Case("down-ragged", "down", _DOWN, (1, 10, 14), "stride 2, ragged: gather dgrad", (_FLAT, _WG0, _FLAT_D)),
    Case("tail-dec", "tail", "decoder", (2, 16, 16), "decoder tail 128 -> 3: thin kernels, transform fused",
         ("igemm_rows_bf16_kernel<128,32,4,1,false,2>", "wgrad_thin_bf16_kernel<false,2>", "conv_thin_bf16_kernel")),
    Case("tail-enc", "tail", "encoder", (2, 4, 4), "encoder tail 512 -> 8: transform materialised",
         ("igemm_rows_bf16_kernel<128,32,4,1,false,0>", "wgrad_bf16_kernel<32,128,1,4,2>", _FLAT_D)),
    Case("conv-in", "conv", "encoder.conv_in", (2, 16, 16), "3 -> 128 on the matrix-pipe thin kernels, no input gradient",
         ("conv_thin_bf16_kernel", "wgrad_thin_bf16_kernel<true,0>"), need_dx=False, live_in=False),
    Case("post-quant", "conv", "post_quant_conv", (2, 4, 4), "4 -> 4, 1x1: the fp32 small-k kernels read the operands unrounded",
         ("conv_smallk_kernel", "wgrad_smallk_kernel<true,0>", "conv_smallk_kernel")),
]
_ATT = "encoder.mid_block.attentions.0"
_FLAT_A, _WG1 = "igemm_rows_bf16_kernel<128,128,4,2,false,1>", "wgrad_bf16_kernel<128,128,4,2,1>"
_ATT_BWD = (_WG0, _FLAT_D) + (_WG1, _FLAT_D) * 3   # to_out's backward, then the three projections' (their transform fused in the wgrad)
# (the blockwise kernels are not launched through an argument block: ops.ATTN_CALLS and the profiler's attn_* records hold them)
CASES += [
    Case("attn-materialised", "attn", _ATT, (2, 8, 8), "materialised scores (T = 64 below ops.ATTN_BLOCKWISE_MIN_T)",
         (_FLAT,) * 4 + (_FLAT_D, _FLAT, _WG0, _FLAT_D, _FLAT, _WG0, _FLAT_D, _WG0) + (_WG1, _FLAT_D) * 3),
    Case("attn-blockwise-64", "attn", _ATT, (2, 8, 8), "blockwise kernels, one row block (ATTN_BLOCKWISE_MIN_T lowered to 64)",
         (_FLAT,) * 4 + _ATT_BWD),
    Case("attn-blockwise-192", "attn", _ATT, (1, 8, 24), "blockwise kernels, three row blocks; the projections' transform fused on load",
         (_FLAT_A,) * 3 + (_FLAT,) + _ATT_BWD),
]
BY_ID = {c.id: c for c in CASES}
