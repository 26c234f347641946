"""The routes of the conv host ops (vaehip/ops.py: conv_fwd, conv_dgrad, conv_wgrad and their helpers), one case per arm.

A case names one call of ops.conv_fwd / conv_dgrad / conv_wgrad, the ROUTE it must take (kernel names, helper entry points,
entries into the three conv functions = recursions, storage and attributes of the result) and is checked against a float64
CPU convolution of the operands as the serving kernel reads them (tests/test_conv_routes_gpu.py).

The same call can be made without a GPU (`run(case, dry=True)`): every launching entry point is replaced by a recorder, the
pure dispatch queries are answered by the real library, and the tensors are host tensors whose addresses are never
dereferenced (the fake-pointer technique of tests/golden/make_dispatch_table.py).  tests/test_conv_routes_host.py holds every
case's route that way, so a change of the dispatcher that re-routes a case fails there and cannot hollow out the GPU module.

    python tests/conv_routes.py      prints, for every case whose dry run leaves the pinned route, the route it takes now
"""
import ast
import inspect
import math
import sys
import textwrap
import zlib
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn.functional as F

# entry points that only answer (no launch, no device access): passed through in a dry run
PURE = {"vae_igemm_kernel_name", "vae_wgrad_kernel_name", "vae_wgrad_plan", "vae_wgrad_wino_plan", "vae_set_option"}
# the helper entry points a route is made of besides its kernels
HELPERS = ("vae_gn_apply", "vae_unpack_bf16", "vae_pack_bf16", "vae_sumpool2x2", "vae_reduce_splits", "vae_reduce_splits2",
           "vae_upconv_fold_wgrad", "vae_wgrad_wino_reduce")
TRACED = ("_upconv_wino", "_upconv_wino_fwd", "_upconv_wino_dgrad", "_upconv_phase_fwd", "_upconv_phase_dgrad", "_upconv_phase_wgrad",
          "conv_fwd", "conv_dgrad", "conv_wgrad", "_wgrad_wino", "_reduce_splits", "_phase_weights", "_phases", "_like", "to_f32", "to_bf16",
          "_grad16", "act_image_ok", "act_image32_ok", "grad_image_ok",
          # the launch descriptions the conv entry points build their argument blocks from
          "out_hw", "_fwd_geom", "_rows_args", "_wgrad_form", "fwd_args", "dgrad_args", "up2x_dgrad_args", "phase_args", "wgrad_args",
          "wgrad_phase_args")

# statements of the traced functions that no case can execute: {source text: why}.  At most 5, each shown unreachable by a
# library query on the host (tests/test_conv_routes_host.py); everything else runs inside a case whose value is compared.
ALLOWED = {}

# the project's own bars, relative to the reference's max (tests/test_kernels_gpu.py, tests/test_act16_gpu.py)
BAR_DIRECT, BAR_WINO, BAR_WINO4, BAR_WGRAD, BAR_WGRAD_GN, BAR_STATS = 2e-5, 1e-5, 4e-5, 3e-5, 5e-5, 1e-5


@dataclass
class Case:
    id: str
    op: str                      # fwd | dgrad | wgrad
    kind: str
    shape: tuple                 # B, H, W, Ci, Co
    mode: str = "f32"            # f32 | bf16 (bf16 arithmetic, fp32 storage) | act16 (bf16 arithmetic and storage)
    # the route the call must take
    names: tuple = ()            # prefix of each recorded kernel name, in launch order
    helpers: tuple = ()          # helper entry points in call order
    entries: int = 1             # entries into conv_fwd / conv_dgrad / conv_wgrad (> 1: a recursion)
    dtype: str = "f32"           # storage of the result (fwd, dgrad)
    attr: Optional[bool] = None  # fwd: `_gstat` attached; dgrad: `_gnb` attached (None: not asked for)
    makes_b16: bool = False      # the call attaches a bf16 image (`_b16`) to its fp32 operand
    raises: bool = False         # the library refuses the launch (VaeHipError) before anything runs
    # the call
    options: tuple = ()          # library options set for the call
    attrs: dict = field(default_factory=dict)  # ops globals set for the call (PHASE_UPCONV, WINOGRAD)
    x: str = "f32"               # storage of x
    Cs: Optional[int] = None     # channels of x's storage (> Ci: the extra ones are zero-weighted)
    xf: int = 0
    a16: bool = False            # fwd: a16 = / wgrad: x16 = the bf16 image of XF(x)
    res: Optional[str] = None    # f32 | bf16
    track: bool = False
    gstat: bool = False
    out: Optional[str] = None    # out_dtype
    dy: str = "f32"              # f32 | bf16 | f32+img (fp32 with a bf16 image attached as `_b16`)
    out_bf16: bool = False
    gnb: Optional[str] = None    # match | shape (a GroupNorm whose input has another shape)
    x_img: bool = False          # wgrad: the fp32 x carries its bf16 image as `_b16`
    bias: bool = True
    reads_img: bool = False      # dy = f32+img: the kernel reads the image (else the fp32 tensor)
    image_ok: Optional[tuple] = None  # fwd: what (act_image_ok, act_image32_ok, grad_image_ok) answer for the layer
    why: str = ""                # the arm the case is there for


def _c(id, op, kind, shape, mode="f32", **kw):
    return Case(id, op, kind, shape, mode, **kw)


# B, H, W, Ci, Co: the smallest shapes that take each arm
HALO, WINO4, RAGGED = (2, 8, 32, 128, 128), (1, 16, 32, 128, 128), (1, 5, 7, 128, 128)  # halo tiles / F(4x4) / ragged (flat kernels)
UNVEC, UNFUS, SMALLK = (2, 5, 7, 102, 128), (2, 4, 4, 512, 128), (2, 4, 4, 4, 128)      # Ci % 4 != 0 / GroupNorm unfusable / <= 4-channel contraction
WIDE, WIDE_D = (13, 32, 64, 128, 256), (13, 32, 64, 256, 128)  # >= 192 wide tiles for the upsampler's forward / its dgrad
UPS, UPR, UP7 = (2, 4, 32, 128, 128), (1, 5, 6, 128, 128), (7, 32, 64, 128, 256)      # upsampler: halo-tile phases / ragged / just below 192 wide tiles


# ------------------------------------------------------------------------------------------------ recording
class Recorder:
    """what one call did: kernel names (from the argument block of every launch), helper entry points, entries into the conv
    functions.  dry: nothing is launched."""

    def __init__(self, ops, lib, dry):
        self.ops, self.lib, self.dry = ops, lib, dry
        self.names, self.helpers, self.entries = [], [], 0

    def __enter__(self):
        ops, lib = self.ops, self.lib
        self._call = lib.call
        self._fns = {n: getattr(ops, n) for n in ("conv_fwd", "conv_dgrad", "conv_wgrad")}
        self._dry = {n: getattr(ops, n) for n in ("_chk_act", "_stream")}

        def call(name, *args):
            if name == "vae_igemm_rows":
                self.names.append(ops._kernel_name("vae_igemm_kernel_name", args[0]._obj))
            elif name == "vae_wgrad":
                self.names.append(ops._kernel_name("vae_wgrad_kernel_name", args[0]._obj))
            elif name == "vae_wgrad_wino":
                self.names.append("wgrad3_upwino_kernel" if lib.query("vae_wgrad_wino_positions", args[0]) == 9 else "wgrad3_wino_kernel")
            elif name in HELPERS:
                self.helpers.append(name)
            if name in PURE or not self.dry:
                return self._call(name, *args)

        def counted(fn):
            def wrapper(*a, **kw):
                self.entries += 1
                return fn(*a, **kw)
            return wrapper

        lib.call = call
        for n, fn in self._fns.items():
            setattr(ops, n, counted(fn))
        if self.dry:
            ops._chk_act = lambda t, name: None
            ops._stream = lambda: None
        return self

    def __exit__(self, *exc):
        del self.lib.call
        for n, fn in {**self._fns, **self._dry}.items():
            setattr(self.ops, n, fn)
        return False


# ------------------------------------------------------------------------------------------------ line coverage
def traced_codes(ops):
    return {getattr(ops, n).__code__ for n in TRACED}


class LineTracer:
    """records the executed lines of the given code objects into `seen` ((function name, line) pairs); the previous trace
    function is restored on exit"""

    def __init__(self, codes, seen):
        self.codes, self.seen = set(codes), seen

    def _local(self, frame, event, arg):
        if event == "line":
            self.seen.add((frame.f_code.co_name, frame.f_lineno))
        return self._local

    def _global(self, frame, event, arg):
        if frame.f_code in self.codes:
            self.seen.add((frame.f_code.co_name, frame.f_lineno))
            return self._local
        return None

    def __enter__(self):
        self.prev = sys.gettrace()
        sys.settrace(self._global)
        return self

    def __exit__(self, *exc):
        sys.settrace(self.prev)
        return False


def statements(fn):
    """{(function name, line in its file): source text} of every statement of `fn` (docstrings and `raise` lines aside); the
    text is the statement's first line, stripped"""
    src = textwrap.dedent(inspect.getsource(fn))
    lines, first = src.splitlines(), fn.__code__.co_firstlineno
    fdef = ast.parse(src).body[0]
    out = {}
    for node in ast.walk(fdef):
        if not isinstance(node, ast.stmt) or node is fdef or isinstance(node, ast.Raise):
            continue
        if isinstance(node, ast.Expr) and isinstance(node.value, ast.Constant) and isinstance(node.value.value, str):
            continue
        out[(fn.__name__, first + node.lineno - 1)] = lines[node.lineno - 1].strip()
    return out


def missed(fns, seen):
    """source texts of the statements of `fns` that never executed, in file order"""
    stm = {}
    for fn in fns:
        stm.update(statements(fn))
    return [stm[k] for k in sorted(stm, key=lambda k: k[1]) if k not in seen]


# ------------------------------------------------------------------------------------------------ running a case
def _seed(case):
    return zlib.crc32(case.id.encode()) & 0x7FFFFFFF


class Mode:
    """ops.PRECISION / ACT_BF16 / WEIGHTS16, library options and ops globals of a case, restored on exit"""

    def __init__(self, ops, case):
        self.ops, self.case = ops, case

    def __enter__(self):
        ops, c = self.ops, self.case
        self.keep = {n: getattr(ops, n) for n in ("PRECISION", "ACT_BF16", "WEIGHTS16", "PROFILER", *c.attrs)}
        self.opts = [ops.option(n, v) for n, v in c.options]
        ops.PRECISION = ops.PREC_F32 if c.mode == "f32" else ops.PREC_BF16
        ops.ACT_BF16 = c.mode == "act16"
        for n, v in c.attrs.items():
            setattr(ops, n, v)
        for o in self.opts:
            o.__enter__()
        return self

    def __exit__(self, *exc):
        for o in reversed(self.opts):
            o.__exit__()
        for n, v in self.keep.items():
            setattr(self.ops, n, v)
        return False


def _store(t, how):
    return t.bfloat16() if how == "bf16" else t


def run(case, dev="cuda", dry=False):
    """makes the call of `case` -> dict with the operands, the result, and the recorded route"""
    from vaehip import ops
    from vaehip.lib import lib
    c = case
    B, H, W, Ci, Co = c.shape
    Cs = c.Cs or Ci
    k = 1 if c.kind == "c1" else 3
    Ho, Wo = ops.out_hw(c.kind, H, W)
    gen = torch.Generator().manual_seed(_seed(c))
    r = {}

    def rnd(*shape, scale=1.0, shift=0.0):
        if dry:  # (values are never read)
            return torch.empty(*shape)
        return (torch.randn(*shape, generator=gen) * scale + shift).to(dev)

    with Mode(ops, c):
        x = rnd(B, H, W, Cs, scale=1.2, shift=0.1)
        w = rnd(Co, k, k, Ci, scale=1.0 / math.sqrt(Ci * k * k))  # OHWI memory
        wd = w.permute(0, 3, 1, 2)                                   # the logical OIHW view the ops take
        bias = rnd(Co) if c.bias else None
        if c.mode != "f32":  # a bf16 image of the weights, as the engine hands over
            img = torch.empty(w.numel(), device=dev, dtype=torch.bfloat16)
            rec0 = Recorder(ops, lib, dry)
            with rec0:
                ops.pack_bf16(w, img)
            ops.WEIGHTS16 = (w.data_ptr(), w.numel() * 4, img.data_ptr())
            r["w16"] = img
        st = None
        if c.xf:  # the conv reads scale / shift only
            z = torch.zeros(B, 32, device=dev)
            st = ops.Stats(z, z, rnd(B, Cs, scale=0.3, shift=1.0), rnd(B, Cs, scale=0.2))
        xs = _store(x, c.x)
        r.update(x=xs, w=w, bias=bias, st=st)
        with Recorder(ops, lib, dry) as rec0:
            if (c.xf or c.a16) and not c.raises:  # bf16 arithmetic reads the device's own transform, rounded (no one-ulp flips of a CPU one enter)
                r["act16"] = ops.gn_apply_bf16(xs, st, c.xf) if (c.xf and not dry and c.mode != "f32") else xs.bfloat16()
        a16 = r["act16"] if c.a16 else None
        dy = None
        if c.op != "fwd":
            dy = rnd(B, Ho, Wo, Co)
            if c.dy == "bf16":
                dy = dy.bfloat16()
            elif c.dy == "f32+img":  # an image that is NOT the rounded tensor: a kernel that reads it where it must not shows in the value
                dy._b16 = (dy * 0.5).bfloat16()
                r["dy_img"] = dy._b16
            r["dy"] = dy
        res = _store(rnd(B, Ho, Wo, Co), c.res) if c.res else None
        track = ops.conv_track_buffer(B * Ho * Wo, Co, dev) if c.track else None
        out_dtype = {None: None, "f32": torch.float32, "bf16": torch.bfloat16}[c.out]
        gnb = None
        if c.gnb:
            gshape = (B, H, W, Ci) if c.gnb == "match" else (B, H, 2 * W, Ci)
            gx = rnd(*gshape)
            gamma, beta = rnd(Ci, scale=0.3, shift=1.0), rnd(Ci, scale=0.2)
            if dry or Ci % 32:  # (102 channels have no 32 groups: that case is there for a gnb that is dropped)
                z = torch.zeros(B, 32, device=dev)
                gst = ops.Stats(z, z, z, z)
            else:
                gst = ops.gn_stats(gx, gamma, beta)
            gnb = ops.GnCtx(gx, gst, gamma, beta, True, 32)
            r["gnb"] = gnb
        if c.x_img:
            xs._b16 = xs.bfloat16()
        r.update(res=res, track=track)
        prof = None if dry else ops.LaunchProfiler()
        ops.PROFILER = prof
        rec = Recorder(ops, lib, dry)
        try:
            with rec:
                if c.op == "fwd":
                    r["out"] = ops.conv_fwd(xs, wd, bias, c.kind, xf=c.xf, stats=st, res=res, track=track, a16=a16,
                                            gstat_groups=32 if c.gstat else None, out_dtype=out_dtype)
                elif c.op == "dgrad":
                    r["out"] = ops.conv_dgrad(dy, wd, c.kind, (H, W), out_bf16=c.out_bf16, out_dtype=out_dtype, gnb=gnb)
                else:
                    gw = torch.full((Co, k, k, Ci), float("nan"), device=dev).permute(0, 3, 1, 2)
                    gb = torch.full((Co,), float("nan"), device=dev) if c.bias else None
                    ops.conv_wgrad(dy, xs, c.kind, gw, gb, xf=c.xf, stats=st, x16=a16)
                    r["out"], r["gb"] = gw.permute(0, 2, 3, 1), gb
        finally:
            ops.PROFILER = None
        if prof is not None:  # the profiler's names are the record; the argument blocks must tell the same story
            pn = [p[0] for p in prof.records if p[1] > 0]
            assert [n.split("<")[0] for n in pn] == [n.split("<")[0] for n in rec.names], (pn, rec.names)
            rec.names = pn
        r["route"] = rec
        if c.op == "fwd":  # the three image queries of the engine, for this layer in this mode
            r["image_ok"] = (ops.act_image_ok(c.kind, xs.shape, Co, Ci), ops.act_image32_ok(c.kind, xs.shape, Co, Ci),
                             ops.grad_image_ok(c.kind, xs.shape, Co, Ci))
        if not dry and c.op == "fwd" and c.gstat and hasattr(r["out"], "_gstat"):
            g1, b1 = torch.ones(Co, device=dev), torch.zeros(Co, device=dev)
            r["stats"] = (ops.gn_stats(r["out"], g1, b1), ops.gn_stats(r["out"].clone(), g1, b1))
        if not dry and c.op == "dgrad" and gnb is not None and hasattr(r["out"], "_gnb"):
            both = []
            for g in (r["out"], r["out"].clone()):
                dg, db = torch.empty(Ci, device=dev), torch.empty(Ci, device=dev)
                both.append((ops.gn_bwd(gnb.x, g, gnb.st, gnb.gamma, gnb.beta, True, None, dg, db).float(), dg, db))
            r["gnb_sums"] = both
    return r


def check_route(case, r):
    """the route part of a case: kernel names, helpers, recursion, storage and attributes of the result"""
    c, rec = case, r["route"]
    assert len(rec.names) == len(c.names) and all(n.startswith(p) for n, p in zip(rec.names, c.names)), (c.id, rec.names, c.names)
    assert tuple(rec.helpers) == tuple(c.helpers), (c.id, rec.helpers, c.helpers)
    assert rec.entries == c.entries, (c.id, rec.entries)
    out = r["out"]
    if c.op != "wgrad":
        assert out.dtype == (torch.bfloat16 if c.dtype == "bf16" else torch.float32), (c.id, out.dtype)
    if c.op == "fwd" and c.gstat:
        assert hasattr(out, "_gstat") == bool(c.attr), (c.id, hasattr(out, "_gstat"))
    if c.op == "dgrad" and c.gnb:
        assert hasattr(out, "_gnb") == bool(c.attr), (c.id, hasattr(out, "_gnb"))
    made = [n for n in ("x", "dy") if r.get(n) is not None and r[n].dtype == torch.float32 and getattr(r[n], "_b16", None) is not None
            and not (n == "x" and c.x_img) and not (n == "dy" and c.dy == "f32+img")]
    assert bool(made) == c.makes_b16, (c.id, made)
    if c.op == "fwd":
        assert r["image_ok"] == c.image_ok, (c.id, r["image_ok"])


# ------------------------------------------------------------------------------------------------ float64 reference
def _nchw(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def _conv(x, w, kind):
    if kind == "c1":
        return F.conv2d(x, w)
    if kind == "c3s2":
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, None, 2, 0)
    if kind == "c3up":
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return F.conv2d(x, w, None, 1, 1)


def _phase_conv(x, we):
    """conv3x3(nearest_upsample_2x(x)) as the four phase convolutions with the effective kernels `we` [4, Co, 3, 3, Ci]"""
    ys = [F.conv2d(x, we[p].permute(0, 3, 1, 2), None, 1, 1) for p in range(4)]
    B, Co, H, W = ys[0].shape
    y = torch.zeros(B, Co, 2 * H, 2 * W, dtype=x.dtype)
    for pa in (0, 1):
        for pb in (0, 1):
            y[:, :, pa::2, pb::2] = ys[pa * 2 + pb]
    return y


def reference(case, r):
    """float64 result of the call on the operands as the serving kernel reads them -> (reference NHWC / OHWI, bias-gradient
    reference or None, the part of the result it covers: None = all of it, else indices of the leading axis).  Which operands are rounded to bf16 follows from the recorded kernel name; a bf16 phase kernel reads
    effective kernels rounded AFTER the taps were summed in fp32 (the device's own sums, rounded)."""
    from vaehip import ops
    c, names = case, r["route"].names
    B, H, W, Ci, Co = c.shape
    k16 = "bf16" in names[-1] if c.op != "wgrad" else any("bf16" in n for n in names)
    phase = c.kind == "c3up" and len([n for n in names if "upwino" not in n]) == 4
    r16 = (lambda t: t.bfloat16()) if k16 else (lambda t: t)
    wv = r["w"]
    # the activation
    if c.a16:
        act = r["act16"]
    elif c.xf and k16:
        act = r["act16"]
    elif c.xf:  # fp32 arithmetic: the stored values through a float64 transform of the host's own
        act = r["x"].double().cpu() * r["st"].scale.double().cpu()[:, None, None, :] + r["st"].shift.double().cpu()[:, None, None, :]
        act = act * torch.sigmoid(act) if c.xf == 2 else act
    else:
        act = r16(r["x"])
    # the largest shapes are compared on a part of the result (float64 on the host costs seconds otherwise): the first, the
    # middle and the last image of a forward / dgrad, output channels at both ends of every 128-channel block of a wgrad
    sel = None
    if B >= 7:
        sel = [0, B // 2, B - 1] if c.op != "wgrad" else [ch for b0 in range(0, Co, 128) for ch in (*range(b0, b0 + 4), *range(b0 + 124, b0 + 128))]
    act = _nchw(act if (sel is None or c.op != "fwd") else act[sel])[:, :Ci]
    if phase and k16 and c.op != "wgrad":  # (fp32 phases: the plain upsample + convolution)
        we = r16(ops.upconv_phase_weights(wv)).double().cpu()
        conv = lambda a, _w: _phase_conv(a, we)  # noqa: E731
    else:
        conv = lambda a, w_: _conv(a, w_, c.kind)  # noqa: E731
    w64 = r16(wv).double().cpu().permute(0, 3, 1, 2)
    if c.op == "fwd":
        y = conv(act, w64)
        if r["bias"] is not None:
            y = y + r["bias"].double().cpu().view(1, -1, 1, 1)
        if r["res"] is not None:  # as stored: through the output's storage first
            res = r["res"].bfloat16() if c.dtype == "bf16" else r["res"]
            y = y + _nchw(res if sel is None else res[sel])
        return y.permute(0, 2, 3, 1), None, sel
    dy = r["dy_img"] if c.reads_img else r["dy"]
    if c.op == "dgrad":
        dy = dy if sel is None else dy[sel]
        a0 = torch.zeros(dy.shape[0], Ci, H, W, dtype=torch.float64, requires_grad=True)
        (gx,) = torch.autograd.grad(conv(a0, w64), a0, _nchw(r16(dy)))
        return gx.permute(0, 2, 3, 1), None, sel
    k = 1 if c.kind == "c1" else 3
    # the bias gradient: fp32 sums of dY as the kernel reads it -- the ROUNDED values where it reads a bf16 image (dY16), the
    # tensor as given on every other path (tests/test_kernels_gpu.py, test_bf16_gradient_images_conv)
    img = any(n.startswith("wgrad3_dma_bf16") or (n.startswith("wgrad3_tile_bf16") and n.endswith(",true>")) for n in names)
    gb = (dy.bfloat16() if img else dy).double().cpu().sum(dim=(0, 1, 2)) if c.bias else None
    if sel is not None:
        dy = dy[..., sel]
    w0 = torch.zeros(dy.shape[-1], Ci, k, k, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad(_conv(act, w0, c.kind), w0, _nchw(r16(dy)))
    return gw.permute(0, 2, 3, 1), gb, sel


def bar(case, names):
    c = case
    if c.op == "wgrad":
        return BAR_WGRAD_GN if (c.xf and c.mode == "f32") else BAR_WGRAD
    n = names[-1]
    return BAR_WINO4 if "wino4" in n else BAR_WINO if ("wino" in n and "upwino" not in n) else BAR_DIRECT


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def check_value(case, r):
    """-> {figure: (measured, bar)}; asserts after collecting"""
    c = case
    ref, gb, sel = reference(c, r)
    out = r["out"] if sel is None else r["out"][sel]
    fig = {}
    if out.dtype == torch.bfloat16:  # one rounding of the result: per element
        err = (out.double().cpu() - ref).abs()
        fig["elements_over_one_bf16_rounding"] = (float((err > 2.0 ** -7 * ref.abs() + 1e-6).sum()), 0.0)
        fig["rel16"] = (rel(out, ref), 6e-3)
    else:
        fig["rel"] = (rel(out, ref), bar(c, r["route"].names))
    if gb is not None:
        fig["bias_grad"] = (rel(r["gb"], gb), BAR_WGRAD)
    if r["track"] is not None:
        # the tracker epilogue holds mean |y| per channel of the tensor as stored (1e-5).  Where the result was re-stored as bf16
        # afterwards it describes the fp32 result BEFORE that rounding: held to the float64 reference, whose every element the
        # fp32 result meets within the forward bar of the reference's max -- so does a mean of magnitudes
        from vaehip import ops
        M = out.shape[0] * out.shape[1] * out.shape[2]
        got = ops.track_final(r["track"], M).double().cpu()
        if r["route"].entries == 1:
            fig["track"] = (rel(got, out.float().abs().mean(dim=(0, 1, 2))), BAR_STATS)
        else:
            fig["track_unrounded"] = (float((got - ref.abs().mean(dim=(0, 1, 2))).abs().max() / ref.abs().max()), bar(c, r["route"].names))
    if "stats" in r:
        sf, sp = r["stats"]
        fig["gstat_mean"] = (rel(sf.mean, sp.mean), BAR_STATS)
        fig["gstat_rstd"] = (rel(sf.rstd, sp.rstd), BAR_STATS)
    if "gnb_sums" in r:
        (d0, g0, b0), (d1, g1, b1) = r["gnb_sums"]
        fig["gnb_dx"], fig["gnb_dgamma"], fig["gnb_dbeta"] = (rel(d0, d1), BAR_STATS), (rel(g0, g1), BAR_STATS), (rel(b0, b1), BAR_STATS)
    return fig


# ------------------------------------------------------------------------------------------------ the cases
# --- table begin
CASES = [
    # --- main routes of the plain 3x3 layer, in fp32 mode, in bf16 mode with fp32 storage, and with bf16 storage
    _c('fwd-halo-f32', 'fwd', 'c3', HALO, 'f32', names=('conv3_wino_kernel',), attr=True, gstat=True, image_ok=(False, True, False),
       why='main route, halo tiles; statistics epilogue where the kernel has one'),
    _c('dgrad-halo-f32', 'dgrad', 'c3', HALO, 'f32', names=('conv3_wino_kernel',), attr=True, gnb='match',
       why='main route, halo tiles; GroupNorm-backward epilogue where the kernel has one (else nch = 0: gnb dropped)'),
    _c('wgrad-halo-f32', 'wgrad', 'c3', HALO, 'f32', names=('wgrad3_wino_kernel',), helpers=('vae_wgrad_wino_reduce',),
       why='main route, halo tiles'),
    _c('fwd-halo-bf16', 'fwd', 'c3', HALO, 'bf16', names=('conv3_tile_bf16_kernel',), attr=True, gstat=True, image_ok=(True, False, True),
       why='main route, halo tiles; statistics epilogue where the kernel has one'),
    _c('dgrad-halo-bf16', 'dgrad', 'c3', HALO, 'bf16', names=('conv3_tile_bf16_kernel',), attr=False, gnb='match',
       why='main route, halo tiles; GroupNorm-backward epilogue where the kernel has one (else nch = 0: gnb dropped)'),
    _c('wgrad-halo-bf16', 'wgrad', 'c3', HALO, 'bf16', names=('wgrad3_tile_bf16_kernel',), helpers=('vae_reduce_splits2',),
       why='main route, halo tiles'),
    _c('fwd-halo-act16', 'fwd', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), dtype='bf16', attr=True, x='bf16', gstat=True, image_ok=(True, False, True),
       why='main route, halo tiles; statistics epilogue where the kernel has one'),
    _c('dgrad-halo-act16', 'dgrad', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), dtype='bf16', attr=False, dy='bf16', gnb='match',
       why='main route, halo tiles; GroupNorm-backward epilogue where the kernel has one (else nch = 0: gnb dropped)'),
    _c('wgrad-halo-act16', 'wgrad', 'c3', HALO, 'act16', names=('wgrad3_dma_bf16_kernel',), helpers=('vae_reduce_splits2',), x='bf16', dy='bf16',
       why='main route, halo tiles'),
    _c('fwd-wino4-f32', 'fwd', 'c3', WINO4, 'f32', names=('conv3_wino4_kernel',), attr=True, gstat=True, image_ok=(False, True, False),
       why='main route, the F(4x4) shape; statistics epilogue where the kernel has one'),
    _c('dgrad-wino4-f32', 'dgrad', 'c3', WINO4, 'f32', names=('conv3_wino4_kernel',), attr=True, gnb='match',
       why='main route, the F(4x4) shape; GroupNorm-backward epilogue where the kernel has one (else nch = 0: gnb dropped)'),
    _c('wgrad-wino4-f32', 'wgrad', 'c3', WINO4, 'f32', names=('wgrad3_wino_kernel',), helpers=('vae_wgrad_wino_reduce',),
       why='main route, the F(4x4) shape'),
    _c('fwd-ragged-f32', 'fwd', 'c3', RAGGED, 'f32', names=('igemm_rows_kernel',), attr=False, gstat=True, image_ok=(False, False, False),
       why='main route, a ragged map: flat kernels; statistics epilogue where the kernel has one'),
    _c('dgrad-ragged-f32', 'dgrad', 'c3', RAGGED, 'f32', names=('igemm_rows_kernel',), attr=False, gnb='match',
       why='main route, a ragged map: flat kernels; GroupNorm-backward epilogue where the kernel has one (else nch = 0: gnb dropped)'),
    _c('wgrad-ragged-f32', 'wgrad', 'c3', RAGGED, 'f32', names=('wgrad_kernel',), helpers=('vae_reduce_splits',),
       why='main route, a ragged map: flat kernels'),
    _c('fwd-ragged-bf16', 'fwd', 'c3', RAGGED, 'bf16', names=('igemm_rows_bf16_kernel',), attr=False, gstat=True, image_ok=(False, False, False),
       why='main route, a ragged map: flat kernels; statistics epilogue where the kernel has one'),
    _c('dgrad-ragged-bf16', 'dgrad', 'c3', RAGGED, 'bf16', names=('igemm_rows_bf16_kernel',), attr=False, gnb='match',
       why='main route, a ragged map: flat kernels; GroupNorm-backward epilogue where the kernel has one (else nch = 0: gnb dropped)'),
    _c('wgrad-ragged-bf16', 'wgrad', 'c3', RAGGED, 'bf16', names=('wgrad_bf16_kernel',), helpers=('vae_reduce_splits',),
       why='main route, a ragged map: flat kernels'),
    _c('fwd-ragged-act16', 'fwd', 'c3', RAGGED, 'act16', names=('igemm_rows_bf16_kernel',), dtype='bf16', attr=False, x='bf16', gstat=True, image_ok=(False, False, False),
       why='main route, a ragged map: flat kernels; statistics epilogue where the kernel has one'),
    _c('dgrad-ragged-act16', 'dgrad', 'c3', RAGGED, 'act16', names=('igemm_rows_bf16_kernel',), dtype='bf16', attr=False, dy='bf16', gnb='match',
       why='main route, a ragged map: flat kernels; GroupNorm-backward epilogue where the kernel has one (else nch = 0: gnb dropped)'),
    _c('wgrad-ragged-act16', 'wgrad', 'c3', RAGGED, 'act16', names=('wgrad_bf16_kernel',), helpers=('vae_reduce_splits',), x='bf16', dy='bf16',
       why='main route, a ragged map: flat kernels'),
    # --- 1x1 and stride-2 layers (both dgrad forms)
    _c('fwd-c1-4-f32', 'fwd', 'c1', (2, 4, 4, 128, 256), 'f32', names=('igemm_rows_kernel',), image_ok=(False, False, False),
       why='1x1'),
    _c('dgrad-c1-4-f32', 'dgrad', 'c1', (2, 4, 4, 128, 256), 'f32', names=('igemm_rows_kernel',),
       why='1x1'),
    _c('wgrad-c1-4-f32', 'wgrad', 'c1', (2, 4, 4, 128, 256), 'f32', names=('wgrad_kernel',), bias=False,
       why='1x1; one split and no bias: nothing to reduce'),
    _c('fwd-c1-4-act16', 'fwd', 'c1', (2, 4, 4, 128, 256), 'act16', names=('igemm_rows_bf16_kernel',), dtype='bf16', x='bf16', image_ok=(False, False, False),
       why='1x1'),
    _c('dgrad-c1-4-act16', 'dgrad', 'c1', (2, 4, 4, 128, 256), 'act16', names=('igemm_rows_bf16_kernel',), dtype='bf16', dy='bf16',
       why='1x1'),
    _c('wgrad-c1-4-act16', 'wgrad', 'c1', (2, 4, 4, 128, 256), 'act16', names=('wgrad_bf16_kernel',), x='bf16', dy='bf16', bias=False,
       why='1x1; one split and no bias: nothing to reduce'),
    _c('fwd-c3s2-16-f32', 'fwd', 'c3s2', (2, 16, 16, 128, 128), 'f32', names=('igemm_rows_kernel',), image_ok=(False, False, False),
       why='stride 2, parity-class dgrad'),
    _c('dgrad-c3s2-16-f32', 'dgrad', 'c3s2', (2, 16, 16, 128, 128), 'f32', names=('igemm_rows_kernel',),
       why='stride 2, parity-class dgrad'),
    _c('wgrad-c3s2-16-f32', 'wgrad', 'c3s2', (2, 16, 16, 128, 128), 'f32', names=('wgrad_kernel',), bias=False,
       why='stride 2, parity-class dgrad; one split and no bias: nothing to reduce'),
    _c('fwd-c3s2-16-act16', 'fwd', 'c3s2', (2, 16, 16, 128, 128), 'act16', names=('igemm_rows_bf16_kernel',), dtype='bf16', x='bf16', image_ok=(False, False, False),
       why='stride 2, parity-class dgrad'),
    _c('dgrad-c3s2-16-act16', 'dgrad', 'c3s2', (2, 16, 16, 128, 128), 'act16', names=('igemm_rows_bf16_kernel',), dtype='bf16', dy='bf16',
       why='stride 2, parity-class dgrad'),
    _c('wgrad-c3s2-16-act16', 'wgrad', 'c3s2', (2, 16, 16, 128, 128), 'act16', names=('wgrad_bf16_kernel',), x='bf16', dy='bf16', bias=False,
       why='stride 2, parity-class dgrad; one split and no bias: nothing to reduce'),
    _c('fwd-c3s2-10-f32', 'fwd', 'c3s2', (1, 10, 14, 128, 128), 'f32', names=('igemm_rows_kernel',), image_ok=(False, False, False),
       why='stride 2, gather dgrad'),
    _c('dgrad-c3s2-10-f32', 'dgrad', 'c3s2', (1, 10, 14, 128, 128), 'f32', names=('igemm_rows_kernel',),
       why='stride 2, gather dgrad'),
    _c('wgrad-c3s2-10-f32', 'wgrad', 'c3s2', (1, 10, 14, 128, 128), 'f32', names=('wgrad_kernel',), bias=False,
       why='stride 2, gather dgrad; one split and no bias: nothing to reduce'),
    # --- conv_fwd: launches whose storage flags the serving kernel refuses (vae_conv_io16_ok = 0) are redone on fp32 copies
    _c('fwd-rec-track-gstat', 'fwd', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), helpers=('vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', attr=False, x='bf16', track=True, gstat=True, image_ok=(True, False, True),
       why='a tracked halo-tile output cannot be bf16; no statistics on the re-stored result'),
    _c('fwd-rec-track-res32', 'fwd', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), helpers=('vae_unpack_bf16', 'vae_pack_bf16', 'vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', attr=False, x='bf16', res='f32', track=True, gstat=True, image_ok=(True, False, True),
       why="a tracked halo-tile output cannot be bf16; an fp32 residual goes through the output's storage once"),
    _c('fwd-rec-track-res16', 'fwd', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), helpers=('vae_unpack_bf16', 'vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', x='bf16', res='bf16', track=True, image_ok=(True, False, True),
       why='a tracked halo-tile output cannot be bf16; a bf16 residual'),
    _c('fwd-rec-track-out32', 'fwd', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), helpers=('vae_unpack_bf16',), x='bf16', res='bf16', track=True, out='f32', image_ok=(True, False, True),
       why='a tracked halo-tile output cannot be bf16; fp32 output asked for, bf16 residual'),
    _c('fwd-rec-xf16-gstat', 'fwd', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), helpers=('vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', attr=False, x='bf16', xf=2, gstat=True, image_ok=(True, False, True),
       why='a bf16-stored x with a fused transform and no image on halo tiles; no statistics on the re-stored result'),
    _c('fwd-rec-xf16-res32', 'fwd', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), helpers=('vae_unpack_bf16', 'vae_pack_bf16', 'vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', attr=False, x='bf16', xf=2, res='f32', gstat=True, image_ok=(True, False, True),
       why="a bf16-stored x with a fused transform and no image on halo tiles; an fp32 residual goes through the output's storage once"),
    _c('fwd-rec-xf16-res16', 'fwd', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), helpers=('vae_unpack_bf16', 'vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', x='bf16', xf=2, res='bf16', image_ok=(True, False, True),
       why='a bf16-stored x with a fused transform and no image on halo tiles; a bf16 residual'),
    _c('fwd-rec-xf16-out32', 'fwd', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), helpers=('vae_unpack_bf16',) * 2, entries=2, x='bf16', xf=2, res='bf16', out='f32', image_ok=(True, False, True),
       why='a bf16-stored x with a fused transform and no image on halo tiles; fp32 output asked for, bf16 residual'),
    _c('fwd-rec-unvec-gstat', 'fwd', 'c3', UNVEC, 'act16', names=('igemm_rows_kernel',), helpers=('vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', attr=False, x='bf16', gstat=True, image_ok=(False, False, False),
       why='Ci = 102 has no vectorised form; no statistics on the re-stored result'),
    _c('fwd-rec-unvec-res32', 'fwd', 'c3', UNVEC, 'act16', names=('igemm_rows_kernel',), helpers=('vae_unpack_bf16', 'vae_pack_bf16', 'vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', attr=False, x='bf16', res='f32', gstat=True, image_ok=(False, False, False),
       why="Ci = 102 has no vectorised form; an fp32 residual goes through the output's storage once"),
    _c('fwd-rec-unvec-res16', 'fwd', 'c3', UNVEC, 'act16', names=('igemm_rows_kernel',), helpers=('vae_unpack_bf16', 'vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', x='bf16', res='bf16', image_ok=(False, False, False),
       why='Ci = 102 has no vectorised form; a bf16 residual'),
    _c('fwd-rec-unvec-out32', 'fwd', 'c3', UNVEC, 'act16', names=('igemm_rows_kernel',), helpers=('vae_unpack_bf16',) * 2, entries=2, x='bf16', res='bf16', out='f32', image_ok=(False, False, False),
       why='Ci = 102 has no vectorised form; fp32 output asked for, bf16 residual'),
    _c('fwd-rec-smallk-gstat', 'fwd', 'c3', SMALLK, 'act16', names=('conv_smallk_kernel',), helpers=('vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', attr=False, x='bf16', gstat=True, image_ok=(False, False, False),
       why='a <= 4-channel contraction reads fp32 only; no statistics on the re-stored result'),
    _c('fwd-smallk-res32', 'fwd', 'c3', SMALLK, 'act16', names=('igemm_rows_bf16_kernel',), helpers=('vae_pack_bf16',), dtype='bf16', attr=False, x='bf16', res='f32', gstat=True, image_ok=(False, False, False),
       why='a <= 4-channel contraction with a bf16 x and an fp32 residual: the bf16 flat kernel takes all of it, nothing recurses'),
    _c('fwd-smallk-res16', 'fwd', 'c3', SMALLK, 'act16', names=('igemm_rows_bf16_kernel',), dtype='bf16', x='bf16', res='bf16', image_ok=(False, False, False),
       why='a <= 4-channel contraction with a bf16 x and a bf16 residual: the bf16 flat kernel, nothing recurses'),
    _c('fwd-smallk-out32', 'fwd', 'c3', SMALLK, 'act16', names=('igemm_rows_bf16_kernel',), helpers=('vae_unpack_bf16',), x='bf16', res='bf16', out='f32', image_ok=(False, False, False),
       why='a <= 4-channel contraction with a bf16 x and an fp32 result: the bf16 flat kernel, nothing recurses'),
    _c('fwd-rec-track-a16', 'fwd', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), helpers=('vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', attr=False, xf=2, a16=True, track=True, gstat=True, image_ok=(True, False, True),
       why='the recursion reads the image (to_f32(a16)) and applies no transform again'),
    _c('fwd-a16-halo', 'fwd', 'c3', HALO, 'act16', names=('conv3_tile_bf16_kernel',), helpers=('vae_pack_bf16',), dtype='bf16', attr=True, xf=2, a16=True, res='f32', gstat=True, image_ok=(True, False, True),
       why='an image given: xf / stats are not applied again; fp32 residual re-stored as bf16'),
    _c('fwd-a16-halo-f32store', 'fwd', 'c3', HALO, 'bf16', names=('conv3_tile_bf16_kernel',), helpers=('vae_unpack_bf16',), xf=2, a16=True, res='bf16', image_ok=(True, False, True),
       why='an image given, fp32 output: a bf16 residual is unpacked'),
    _c('fwd-xf-halo-f32', 'fwd', 'c3', HALO, 'f32', names=('conv3_wino_kernel',), xf=2, res='f32', image_ok=(False, True, False),
       why='fused transform on the Winograd kernel'),
    _c('fwd-xf-halo-bf16', 'fwd', 'c3', HALO, 'bf16', names=('conv3_tile_bf16_kernel',), xf=1, image_ok=(True, False, True),
       why='fused affine transform on the bf16 halo-tile kernel'),
    # --- a transform the kernel cannot fuse (vae_xf_fusable_rows = 0 / vae_wgrad_plan fusable = 0) is materialised by gn_apply, once
    _c('fwd-unfus-4x4-f32', 'fwd', 'c3', UNFUS, 'f32', names=('igemm_rows_kernel',), helpers=('vae_gn_apply',), xf=2, image_ok=(False, False, False),
       why='unfusable transform, forward'),
    _c('wgrad-unfus-4x4-f32', 'wgrad', 'c3', UNFUS, 'f32', names=('wgrad_kernel',), helpers=('vae_reduce_splits',), xf=2,
       why='unfusable transform, weight gradient'),
    _c('fwd-unfus-4x4-bf16', 'fwd', 'c3', UNFUS, 'bf16', names=('igemm_rows_bf16_kernel',), helpers=('vae_gn_apply',), xf=2, image_ok=(False, False, False),
       why='unfusable transform, forward'),
    _c('wgrad-unfus-4x4-bf16', 'wgrad', 'c3', UNFUS, 'bf16', names=('wgrad_bf16_kernel',), helpers=('vae_reduce_splits',), xf=2,
       why='unfusable transform, weight gradient'),
    _c('fwd-unfus-4x4-act16', 'fwd', 'c3', UNFUS, 'act16', names=('igemm_rows_bf16_kernel',), helpers=('vae_gn_apply',), dtype='bf16', x='bf16', xf=2, image_ok=(False, False, False),
       why='unfusable transform, forward'),
    _c('wgrad-unfus-4x4-act16', 'wgrad', 'c3', UNFUS, 'act16', names=('wgrad_bf16_kernel',), helpers=('vae_reduce_splits',), x='bf16', xf=2, dy='bf16',
       why='unfusable transform, weight gradient'),
    _c('fwd-unfus-6x10-f32', 'fwd', 'c3', (2, 6, 10, 512, 128), 'f32', names=('igemm_rows_kernel',), helpers=('vae_gn_apply',), xf=2, image_ok=(False, False, False),
       why='unfusable transform, forward'),
    _c('wgrad-unfus-6x10-f32', 'wgrad', 'c3', (2, 6, 10, 512, 128), 'f32', names=('wgrad_kernel',), helpers=('vae_reduce_splits',), xf=2,
       why='unfusable transform, weight gradient'),
    _c('fwd-unfus-unvec-f32', 'fwd', 'c3', UNVEC, 'f32', names=('igemm_rows_kernel',), helpers=('vae_gn_apply',), Cs=104, xf=2, image_ok=(False, False, False),
       why='unfusable transform, forward'),
    _c('wgrad-unfus-unvec-f32', 'wgrad', 'c3', UNVEC, 'f32', names=('wgrad_kernel',), helpers=('vae_gn_apply', 'vae_reduce_splits'), Cs=104, xf=2,
       why='unfusable transform, weight gradient'),
    _c('fwd-unfus-unvec-bf16', 'fwd', 'c3', UNVEC, 'bf16', names=('igemm_rows_kernel',), helpers=('vae_gn_apply',), Cs=104, xf=2, image_ok=(False, False, False),
       why='unfusable transform, forward'),
    _c('wgrad-unfus-unvec-bf16', 'wgrad', 'c3', UNVEC, 'bf16', names=('wgrad_kernel',), helpers=('vae_gn_apply', 'vae_reduce_splits'), Cs=104, xf=2,
       why='unfusable transform, weight gradient'),
    _c('fwd-unfus-unvec-act16', 'fwd', 'c3', UNVEC, 'act16', names=('igemm_rows_kernel',), helpers=('vae_gn_apply', 'vae_pack_bf16'), entries=2, dtype='bf16', x='bf16', Cs=104, xf=2, image_ok=(False, False, False),
       why='unfusable transform, forward'),
    _c('wgrad-unfus-unvec-act16', 'wgrad', 'c3', UNVEC, 'act16', names=('wgrad_kernel',), helpers=('vae_gn_apply', 'vae_unpack_bf16', 'vae_reduce_splits'), entries=2, x='bf16', Cs=104, xf=2, dy='bf16',
       why='unfusable transform, weight gradient'),
    # --- conv_wgrad: operand storage
    _c('wgrad-fixedbug', 'wgrad', 'c3', UNVEC, 'act16', names=('wgrad_kernel',), helpers=('vae_gn_apply', 'vae_unpack_bf16', 'vae_reduce_splits'), entries=2, Cs=104, xf=2, dy='bf16',
       why='unfusable AND vae_wgrad_io16_ok = 0: materialised, then redone on fp32 copies with NO transform left'),
    _c('wgrad-io16-xf', 'wgrad', 'c3', HALO, 'act16', names=('wgrad3_tile_bf16_kernel',), helpers=('vae_unpack_bf16', 'vae_unpack_bf16', 'vae_reduce_splits2'), entries=2, x='bf16', xf=2, dy='bf16',
       why='vae_wgrad_io16_ok = 0 only: a bf16 x with a fused transform and no image; the transform is applied once, by the kernel'),
    _c('wgrad-x16', 'wgrad', 'c3', HALO, 'act16', names=('wgrad3_dma_bf16_kernel',), helpers=('vae_reduce_splits2',), x='bf16', xf=2, a16=True, dy='bf16',
       why='an image given: no transform'),
    _c('wgrad-x16-rec', 'wgrad', 'c3', UNVEC, 'act16', names=('wgrad_kernel',), helpers=('vae_unpack_bf16', 'vae_unpack_bf16', 'vae_reduce_splits'), entries=2, x='bf16', Cs=104, xf=2, a16=True, dy='bf16',
       why='an image given to an fp32-only kernel: to_f32(x16), no transform'),
    _c('wgrad-halo-bf16-nobias', 'wgrad', 'c3', HALO, 'bf16', names=('wgrad3_tile_bf16_kernel',), helpers=('vae_reduce_splits',), bias=False,
       why='several splits, no bias gradient: the slab reduction alone'),
    _c('wgrad-halo-nowino', 'wgrad', 'c3', HALO, 'f32', names=('wgrad3_tile_kernel',), helpers=('vae_reduce_splits',), options=(('no_wino', 1),),
       why='fp32 halo-tile weight gradient: one split, the bias slab alone is reduced'),
    # --- conv_dgrad: storage and operand forms
    _c('dgrad-dy16-f32only', 'dgrad', 'c3', UNVEC, 'act16', names=('igemm_rows_kernel',), helpers=('vae_unpack_bf16', 'vae_pack_bf16'), entries=2, dtype='bf16', dy='bf16',
       why='a bf16-only gradient into an fp32-only kernel: to_f32(dy16), result re-stored as bf16'),
    _c('dgrad-dy16-f32only-out32', 'dgrad', 'c3', UNVEC, 'act16', names=('igemm_rows_kernel',), helpers=('vae_unpack_bf16',), entries=2, out='f32', dy='bf16',
       why='the same with an fp32 result asked for'),
    _c('dgrad-out16-kept', 'dgrad', 'c3', HALO, 'bf16', names=('conv3_tile_bf16_kernel',), dtype='bf16', attr=False, out_bf16=True, gnb='match',
       why='out_bf16 asked for in fp32-storage mode and kept (halo-tile kernel)'),
    _c('dgrad-out16-away', 'dgrad', 'c3', UNVEC, 'bf16', names=('igemm_rows_kernel',), out_bf16=True,
       why='out_bf16 asked for and negotiated away (fp32-only kernel)'),
    _c('dgrad-gnb-shape', 'dgrad', 'c3', HALO, 'f32', names=('conv3_wino_kernel',), attr=False, gnb='shape',
       why='gnb of a GroupNorm with another input shape: dropped'),
    _c('dgrad-gnb-restored', 'dgrad', 'c3', UNVEC, 'act16', names=('igemm_rows_kernel',), helpers=('vae_pack_bf16',), dtype='bf16', attr=False, gnb='match',
       why='gnb on a result that is re-stored as bf16: dropped'),
    _c('dgrad-img-unused', 'dgrad', 'c3', RAGGED, 'bf16', names=('igemm_rows_bf16_kernel',), dy='f32+img',
       why='an fp32 gradient carrying an image where grad_image_ok is false: the fp32 tensor is read'),
    _c('dgrad-img-used', 'dgrad', 'c3', HALO, 'bf16', names=('conv3_tile_bf16_kernel',), dy='f32+img', reads_img=True,
       why='... and where it is true: the image is read'),
    _c('dgrad-img-f32mode', 'dgrad', 'c3', HALO, 'f32', names=('conv3_wino_kernel',), dy='f32+img',
       why='fp32 mode never reads an image'),
    # --- the upsampler's forward
    _c('fwd-up-upwino', 'fwd', 'c3up', UPS, 'f32', names=('conv3_upwino_kernel',), image_ok=(False, False, False),
       why='upwino'),
    _c('fwd-up-cs-upwino', 'fwd', 'c3up', UPS, 'f32', names=('conv3_upwino_kernel',), Cs=136, image_ok=(False, False, False),
       why='upwino on a padded x (Cs != Ci)'),
    _c('fwd-up-phase-f32', 'fwd', 'c3up', UPS, 'f32', names=('conv3_tile_kernel',) * 4, options=(('no_wino', 1),), image_ok=(False, False, False),
       why='four phases on the fp32 halo-tile kernel'),
    _c('fwd-up-cs', 'fwd', 'c3up', UPS, 'f32', names=('conv3_tile_kernel',), options=(('no_wino', 1),), Cs=136, image_ok=(False, False, False),
       why='Cs != Ci: no phases, the virtual-upsample kernel'),
    _c('fwd-up-phase-wide16', 'fwd', 'c3up', WIDE, 'act16', names=('conv3_wide_bf16_kernel',) * 4, helpers=('vae_pack_bf16',), dtype='bf16', x='bf16', image_ok=(False, False, False),
       why='phases with the bf16 x as the image on the wide kernel, bf16 output'),
    _c('fwd-up-phase-wide-made', 'fwd', 'c3up', WIDE, 'bf16', names=('conv3_wide_bf16_kernel',) * 4, helpers=('vae_pack_bf16',) * 2, makes_b16=True, image_ok=(False, False, False),
       why='phases with an image made of the fp32 x (left as x._b16 for the weight gradient)'),
    _c('fwd-up-phase-tile', 'fwd', 'c3up', UPS, 'bf16', names=('conv3_tile_bf16_kernel',) * 4, helpers=('vae_pack_bf16',), image_ok=(False, False, False),
       why='phases without an image on the bf16 halo-tile kernel'),
    _c('fwd-up-phase-tile-act16', 'fwd', 'c3up', UPS, 'act16', names=('conv3_tile_bf16_kernel',) * 4, helpers=('vae_pack_bf16',) * 2, dtype='bf16', image_ok=(False, False, False),
       why='... whose fp32 result is re-stored as bf16'),
    _c('fwd-up-below16', 'fwd', 'c3up', UPS, 'act16', names=('conv3_tile_bf16_kernel',), dtype='bf16', x='bf16', image_ok=(False, False, False),
       why='a bf16 x below the wide threshold: no phases, the virtual-upsample kernel on taps rounded one by one'),
    _c('fwd-up-below16-out32', 'fwd', 'c3up', UPS, 'act16', names=('conv3_tile_bf16_kernel',), x='bf16', out='f32', image_ok=(False, False, False),
       why='the same with an fp32 result: held to 2e-5 against taps rounded one by one'),
    _c('fwd-up-below16-7', 'fwd', 'c3up', UP7, 'act16', names=('conv3_tile_bf16_kernel',), dtype='bf16', x='bf16', image_ok=(False, False, False),
       why='the same just below 192 wide tiles'),
    _c('fwd-up-ragged-f32', 'fwd', 'c3up', UPR, 'f32', names=('igemm_rows_kernel',), image_ok=(False, False, False),
       why='a ragged map: the flat kernel over the virtual upsample'),
    _c('fwd-up-ragged-act16', 'fwd', 'c3up', UPR, 'act16', names=('igemm_rows_bf16_kernel',), dtype='bf16', x='bf16', image_ok=(False, False, False),
       why='a ragged map, bf16 storage'),
    _c('fwd-up-virtual', 'fwd', 'c3up', UPS, 'f32', names=('conv3_tile_kernel',), options=(('no_wino', 1),), attrs={'PHASE_UPCONV': False}, image_ok=(False, False, False),
       why='phases switched off'),
    # --- the upsampler's dgrad
    _c('dgrad-up-upwino', 'dgrad', 'c3up', UPS, 'f32', names=('conv3_upwino_kernel',),
       why='upwino (dgrad and 2x2 sum-pool in one pass)'),
    _c('dgrad-up-upwino-img', 'dgrad', 'c3up', UPS, 'f32', names=('conv3_upwino_kernel',), dy='f32+img',
       why='upwino ignores an attached image'),
    _c('dgrad-up-phase-f32', 'dgrad', 'c3up', UPS, 'f32', names=('conv3_tile_kernel',) * 4, options=(('no_wino', 1),),
       why='four phases on the fp32 halo-tile kernel'),
    _c('dgrad-up-phase-wide16', 'dgrad', 'c3up', WIDE_D, 'act16', names=('conv3_wide_bf16_kernel',) * 4, helpers=('vae_pack_bf16',) * 2, dtype='bf16', dy='bf16',
       why='phases with the bf16 dy as the image on the wide kernel; the fp32 sum re-stored as bf16'),
    _c('dgrad-up-phase-wide-made', 'dgrad', 'c3up', WIDE_D, 'bf16', names=('conv3_wide_bf16_kernel',) * 4, helpers=('vae_pack_bf16',) * 2,
       why='phases with an image made of the fp32 dy'),
    _c('dgrad-up-phase-tile', 'dgrad', 'c3up', UPS, 'bf16', names=('conv3_tile_bf16_kernel',) * 4, helpers=('vae_pack_bf16',),
       why='phases without an image on the bf16 halo-tile kernel'),
    _c('dgrad-up-below16', 'dgrad', 'c3up', UPS, 'act16', names=('conv3_tile_bf16_kernel',), helpers=('vae_sumpool2x2', 'vae_pack_bf16'), dtype='bf16', dy='bf16',
       why='a bf16 dy below the wide threshold: the virtual-upsample kernel, pooled, re-stored as bf16'),
    _c('dgrad-up-ragged-f32', 'dgrad', 'c3up', UPR, 'f32', names=('igemm_rows_kernel',), helpers=('vae_sumpool2x2',),
       why='the pooled fall-back'),
    _c('dgrad-up-ragged-act16', 'dgrad', 'c3up', UPR, 'act16', names=('igemm_rows_bf16_kernel',), helpers=('vae_sumpool2x2', 'vae_pack_bf16'), dtype='bf16', dy='bf16',
       why='the pooled fall-back, bf16 storage (want16 re-store after the pool)'),
    _c('dgrad-up-virtual', 'dgrad', 'c3up', UPS, 'f32', names=('conv3_tile_kernel',), helpers=('vae_sumpool2x2',), options=(('no_wino', 1),), attrs={'PHASE_UPCONV': False},
       why='phases switched off: halo-tile kernel, pooled'),
    # --- the upsampler's weight gradient
    _c('wgrad-up-upwino', 'wgrad', 'c3up', UPS, 'f32', names=('wgrad3_upwino_kernel',), helpers=('vae_wgrad_wino_reduce',),
       why='the 9-position scheme'),
    _c('wgrad-up-phase-f32', 'wgrad', 'c3up', UPS, 'f32', names=('wgrad3_tile_kernel',) * 4, helpers=('vae_reduce_splits', 'vae_reduce_splits', 'vae_reduce_splits', 'vae_reduce_splits', 'vae_upconv_fold_wgrad'), options=(('no_wino', 1),),
       why='four phase gradients on the fp32 halo-tile kernel, folded'),
    _c('wgrad-up-phase-nobias', 'wgrad', 'c3up', UPS, 'f32', names=('wgrad3_tile_kernel',) * 4, helpers=('vae_upconv_fold_wgrad',), options=(('no_wino', 1),), bias=False,
       why='... one split and no bias: nothing to reduce'),
    _c('wgrad-up-cs', 'wgrad', 'c3up', UPS, 'f32', names=('wgrad3_tile_kernel',), helpers=('vae_reduce_splits2',), options=(('no_wino', 1),), Cs=136,
       why='Cs != Ci: no phases'),
    _c('wgrad-up-phase-both16', 'wgrad', 'c3up', WIDE, 'act16', names=('wgrad3_dma_bf16_kernel',) * 4, helpers=('vae_reduce_splits2', 'vae_reduce_splits2', 'vae_reduce_splits2', 'vae_reduce_splits2', 'vae_upconv_fold_wgrad'), x='bf16', dy='bf16',
       why='both images exist (bf16 tensors); several splits'),
    _c('wgrad-up-phase-made', 'wgrad', 'c3up', UPS, 'bf16', names=('wgrad3_dma_bf16_kernel',) * 4, helpers=('vae_pack_bf16', 'vae_pack_bf16', 'vae_reduce_splits', 'vae_reduce_splits', 'vae_reduce_splits', 'vae_reduce_splits', 'vae_upconv_fold_wgrad'), makes_b16=True,
       why="both images made (dy's left as dy._b16 for the dgrad)"),
    _c('wgrad-up-phase-ximg', 'wgrad', 'c3up', WIDE, 'bf16', names=('wgrad3_dma_bf16_kernel',) * 4, helpers=('vae_pack_bf16', 'vae_reduce_splits2', 'vae_reduce_splits2', 'vae_reduce_splits2', 'vae_reduce_splits2', 'vae_upconv_fold_wgrad'), makes_b16=True, x_img=True,
       why="x's image exists (left by the forward), dy's is made"),
    _c('wgrad-up-phase-x16-dy32', 'wgrad', 'c3up', UPS, 'act16', names=('wgrad3_dma_bf16_kernel',) * 4, helpers=('vae_pack_bf16', 'vae_upconv_fold_wgrad'), makes_b16=True, x='bf16', bias=False,
       why="x is its own image, dy's is made; one split, no bias"),
    _c('wgrad-up-co132', 'wgrad', 'c3up', (2, 4, 32, 128, 132), 'act16', names=('wgrad3_tile_bf16_kernel',) * 4, helpers=('vae_unpack_bf16', 'vae_unpack_bf16', 'vae_reduce_splits', 'vae_reduce_splits', 'vae_reduce_splits', 'vae_reduce_splits', 'vae_upconv_fold_wgrad'), entries=2, x='bf16', dy='bf16',
       why="Co % 8 != 0: bf16 tensors are no images, so the phases leave them to the general path ('the fp32 halo-tile kernel needs fp32 operands'), which redoes the call on fp32 copies: phases without images"),
    _c('wgrad-up-below16', 'wgrad', 'c3up', UPS, 'act16', names=('wgrad3_dma_bf16_kernel',) * 4, helpers=('vae_reduce_splits', 'vae_reduce_splits', 'vae_reduce_splits', 'vae_reduce_splits', 'vae_upconv_fold_wgrad'), x='bf16', dy='bf16',
       why='both images exist, one split with the bias'),
    _c('wgrad-up-ragged-f32', 'wgrad', 'c3up', UPR, 'f32', names=('wgrad_kernel',), helpers=('vae_reduce_splits',),
       why='not served by the phases: the flat kernel'),
    _c('wgrad-up-ragged-act16', 'wgrad', 'c3up', UPR, 'act16', names=('wgrad_bf16_kernel',), helpers=('vae_reduce_splits',), x='bf16', dy='bf16',
       why='not served by the phases, bf16 storage'),
    _c('wgrad-up-virtual', 'wgrad', 'c3up', UPS, 'f32', names=('wgrad3_tile_kernel',), helpers=('vae_reduce_splits2',), options=(('no_wino', 1),), attrs={'PHASE_UPCONV': False},
       why='phases switched off'),
    # --- fp32 mode has fp32 storage: a bf16 operand on a non-Winograd kernel is refused by the launch check, before anything runs
    _c('fwd-unfus-c102-refuse', 'fwd', 'c3', UNVEC, 'f32', names=('igemm_rows_kernel',), helpers=('vae_gn_apply',), raises=True, xf=2, image_ok=(False, False, False),
       why='an unfusable transform on a tensor of 102 channels: gn_apply takes multiples of 4 and refuses'),
    _c('fwd-refuse', 'fwd', 'c3', RAGGED, 'f32', names=('igemm_rows_kernel',), raises=True, x='bf16', image_ok=(False, False, False),
       why='A16 in fp32 mode'),
    _c('dgrad-refuse', 'dgrad', 'c3', RAGGED, 'f32', names=('igemm_rows_kernel',), raises=True, dy='bf16',
       why='A16 (the gradient) in fp32 mode'),
    _c('wgrad-refuse', 'wgrad', 'c3', RAGGED, 'f32', names=('wgrad_kernel',), helpers=('vae_reduce_splits',), raises=True, dy='bf16',
       why='dY16 in fp32 mode'),
    _c('wgrad-up-refuse', 'wgrad', 'c3up', UPS, 'f32', names=('wgrad3_tile_kernel',), helpers=('vae_reduce_splits2',), raises=True, options=(('no_wino', 1),), x='bf16',
       why="the phases leave a bf16 x to the general path ('the fp32 halo-tile kernel needs fp32 operands'), whose launch refuses X16 in fp32 mode"),
]
# --- table end


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vae-channel-dynamics_amd", "src"))
    for case in CASES:
        res = run(case, dev="cpu", dry=True)
        try:
            check_route(case, res)
        except AssertionError:
            rt = res["route"]
            print(f"{case.id}: names={tuple(n.split('<')[0] for n in rt.names)} helpers={tuple(rt.helpers)} entries={rt.entries} "
                  f"dtype={res['out'].dtype} image_ok={res.get('image_ok')}")
