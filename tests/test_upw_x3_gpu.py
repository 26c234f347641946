"""The fp32 upsampler convolution on split-bf16 products (csrc/conv3_upwino.hip): a step takes 16 channels (the K of
v_mfma_f32_32x32x16_bf16), U arrives as three bf16 planes written by vae_wino_weights with K padded to 16 by zero planes, V is
split once by the staging threads, and the octet behind channel K of a K % 16 == 8 layer is zero in both.  ops.conv_fwd /
ops.conv_dgrad with kind "c3up" are called at the smallest shapes at which the loop can go wrong, the kernel names are taken
from the profiler records, and the results are compared with float64 on the host.

Bars: forward and dgrad within 1e-5 of max |ref| (tests/test_kernels_gpu.py).  Every launch is made twice (bit-identical).  The
crafted case compares with float64 on the scale sum |U| |V| carried through |A'| / |s| under the bar tests/test_upw_x3_host.py
derives (tests/upw_x3_refs.py): between the emulated correct form's error and the smallest single mistake's.  It runs at
(1, 8, 16, 64, 64): the kernel's tiles are 4 x 8 low-resolution pixels, so a map of 6 rows is not served (asserted below).

Shapes (B, H, W, Ci, Co): (1,4,8,64,32) one tile, minimum K, four steps, an empty second channel block; (1,4,8,80,64) five steps:
the odd double-buffer parity; (1,4,8,72,36) K % 16 == 8 and a ragged second block; (1,4,8,36,72) its mirror, the dgrad's K = Co
with the tail; (2,8,16,128,160) several tiles both ways, three channel tiles, even and odd workgroups: both seats of the ninth
position."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import upw_x3_refs as R
from guarded import GuardedPool, guarded
from vaehip import ops
from vaehip.lib import lib

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 8, 64, 32), (1, 4, 8, 80, 64), (1, 4, 8, 72, 36), (1, 4, 8, 36, 72), (2, 8, 16, 128, 160)]
# what vae_wino_ok refuses (K = Ci forward, Co dgrad: a multiple of 8, at least 64)
REFUSED = {("fwd", (1, 4, 8, 36, 72)), ("dgrad", (1, 4, 8, 64, 32)), ("dgrad", (1, 4, 8, 72, 36))}
SERVED = [(op, s) for s in SHAPES for op in ("fwd", "dgrad") if (op, s) not in REFUSED]
NAME = {"fwd": "conv3_upwino_kernel<false>", "dgrad": "conv3_upwino_kernel<true>"}
BAR = 1e-5


@functools.lru_cache(maxsize=None)
def _operands(shape, seed=7):
    """host operands of a shape, made once: x, dy, w (OHWI), bias and the float64 forward / dgrad"""
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(seed)
    x, dy = torch.randn(B, H, W, Ci, generator=g), torch.randn(B, 2 * H, 2 * W, Co, generator=g)
    w, bias = torch.randn(Co, 3, 3, Ci, generator=g) / (3.0 * Ci ** 0.5), torch.randn(Co, generator=g)
    return dict(x=x, dy=dy, w=w, bias=bias, fwd=_ref_fwd(x, w, bias), dgrad=_ref_dgrad(dy, w, H, W))


def _ref_fwd(x, w, bias):
    y = F.conv2d(F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest"), w.double().permute(0, 3, 1, 2),
                 None if bias is None else bias.double(), 1, 1)
    return y.permute(0, 2, 3, 1).contiguous()


def _ref_dgrad(dy, w, H, W):
    hi = F.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None, 1, 1)  # gradient wrt the upsampled image
    return F.avg_pool2d(hi, 2, divisor_override=1).permute(0, 2, 3, 1).contiguous()


def _w(w_ohwi, dev):
    """the layer's weight as ops takes it: logical OIHW over OHWI memory"""
    return w_ohwi.to(dev).contiguous().permute(0, 3, 1, 2)


def _run(op, src, w, bias, hw):
    """one call under the profiler -> (result, kernel names)"""
    ops.PROFILER = ops.LaunchProfiler()
    try:
        out = ops.conv_fwd(src, w, bias, "c3up") if op == "fwd" else ops.conv_dgrad(src, w, "c3up", hw)
        names = [r[0] for r in ops.PROFILER.records]
    finally:
        ops.PROFILER = None
    return out, names


def _twice(op, src, w, bias, hw):
    one, names = _run(op, src, w, bias, hw)
    two, _ = _run(op, src, w, bias, hw)
    assert names == [NAME[op]], names
    assert torch.equal(one, two), "two launches differ"
    return one


def _args(op, shape, dev, Cs=None):
    """the launch ops builds for (op, shape), with operands that only stand for their alignment"""
    B, H, W, Ci, Co = shape
    a = ops.fwd_args("c3up", B, H, W, Cs or Ci, Co, Ci) if op == "fwd" else ops.up2x_dgrad_args(B, H, W, Co, Ci)
    keep = torch.zeros(64, device=dev)
    a.A, a.W, a.C = ops._p(keep), ops._p(keep), ops._p(keep)
    return a, keep


def test_which_shapes_are_served(cuda):
    got = {(op, s) for s in SHAPES for op in ("fwd", "dgrad") if not lib.query("vae_wino_ok", C.byref(_args(op, s, cuda)[0]))}
    assert got == REFUSED
    for op in ("fwd", "dgrad"):  # the tiles are 4 x 8 low-resolution pixels: the crafted case cannot have 6 rows
        assert not lib.query("vae_wino_ok", C.byref(_args(op, (1, 6, 16, 64, 64), cuda)[0]))
        assert lib.query("vae_wino_ok", C.byref(_args(op, (1, 8, 16, 64, 64), cuda)[0]))


@pytest.mark.parametrize("op,shape", SERVED)
def test_against_float64(cuda, op, shape):
    r = _operands(shape)
    B, H, W, Ci, Co = shape
    if op == "fwd":
        out = _twice(op, r["x"].to(cuda), _w(r["w"], cuda), r["bias"].to(cuda), None)
    else:
        out = _twice(op, r["dy"].to(cuda), _w(r["w"], cuda), None, (H, W))
    ref = r[op]
    e = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"{op} {shape}: {e:.3e} of max |ref|")
    assert out.shape == ref.shape and e < BAR


def test_tail_with_poison(cuda):
    """Ci = 72 in a tensor of 80 channels whose channels 72..79 hold NaN: the last step's second octet is that memory"""
    shape = (1, 4, 8, 72, 36)
    r = _operands(shape)
    x = torch.full((1, 4, 8, 80), float("nan"))
    x[..., :72] = r["x"]
    out = _twice("fwd", x.to(cuda), _w(r["w"], cuda), r["bias"].to(cuda), None)
    assert bool(torch.isfinite(out).all())
    ref = r["fwd"]
    assert float((out.double().cpu() - ref).abs().max() / ref.abs().max()) < BAR
    # (the dgrad takes no padded dY: ops.conv_dgrad asserts dy's channel count is Co)


@pytest.mark.parametrize("op", ["fwd", "dgrad"])
def test_crafted_operands(cuda, op):
    B, H, W, Ci, Co = 1, 8, 16, 64, 64
    dg = op == "dgrad"
    src, w, ref, scale, e_ok, e_bad, _ = R.crafted_sides(B, H, W, Ci, Co, 24, dg)
    bar = R.bar_between(e_ok, e_bad)
    out = _twice(op, src.to(cuda), _w(w, cuda), None, (H, W))
    ref, scale = R.image(ref, B, H, W, dg), R.image(scale, B, H, W, dg)
    e = R.rel_err(out.cpu(), ref, scale)
    print(f"{op}: device {e:.3e}, emulated {e_ok:.3e}, smallest single mistake {e_bad:.3e}, bar {bar:.3e} of sum|U||V|")
    assert e < bar


@pytest.mark.parametrize("op", ["fwd", "dgrad"])
def test_plane_image(cuda, op):
    """vae_wino_weights at N = 36, K = 72 (forward: Co = 36, Ci = 72; dgrad: the mirror, its K is Co): every plane bitwise the
    CPU's fp32 transform + split, the K padding exactly zero"""
    dg = op == "dgrad"
    shape = (1, 4, 8, 36, 72) if dg else (1, 4, 8, 72, 36)
    Ci, Co = shape[3:]
    w = _operands(shape)["w"]
    a, keep = _args(op, shape, cuda)
    wd = w.to(cuda).contiguous()
    a.W = ops._p(wd)
    assert lib.query("vae_wino_ok", C.byref(a))
    N, K = (Ci, Co) if dg else (Co, Ci)
    nbytes = int(lib.query("vae_wino_weight_bytes", C.byref(a)))
    assert nbytes == 6 * 9 * N * 80 and int(lib.query("vae_wino_weight_floats", C.byref(a))) == 9 * N * K
    wu = torch.full((nbytes // 2,), -1, device=cuda, dtype=torch.int16)
    lib.call("vae_wino_weights", C.byref(a), ops._p(wu), ops._stream())
    got = wu.cpu().reshape(5, 9, 3, N, 16)
    planes = R.split(R.pad16(R.transform_u(w, dg)))                              # 3 x [9, N, 80]
    want = torch.stack([p.bfloat16().view(torch.int16).reshape(9, N, 5, 16) for p in planes])  # [3, 9, N, 5, 16]
    assert torch.equal(got, want.permute(3, 1, 0, 2, 4))
    assert not bool(got[4, :, :, :, 8:].any()), "the K padding is not zero"


@pytest.mark.parametrize("op", ["fwd", "dgrad"])
def test_in_guarded_memory(cuda, op):
    """operands, Wu (sized by vae_wino_weight_bytes) and the output between poisoned guards: every element written, nothing
    outside touched, no operand changed"""
    shape = (1, 4, 8, 72, 36) if op == "fwd" else (1, 4, 8, 36, 72)
    B, H, W, Ci, Co = shape
    r = _operands(shape)
    pool = GuardedPool(cuda)
    src = pool.put((r["x"] if op == "fwd" else r["dy"]).to(cuda), "src")
    w = pool.put(r["w"].to(cuda), "w").permute(0, 3, 1, 2)
    bias = pool.put(r["bias"].to(cuda), "bias") if op == "fwd" else None
    pool.snapshot()
    with guarded(pool, ops):
        out, names = _run(op, src, w, bias, (H, W))
    torch.cuda.synchronize()
    assert names == [NAME[op]]
    assert pool.violations() == [] and pool.changed() == [] and pool.unwritten_report() == []
    ref = r[op]
    assert float((out.double().cpu() - ref).abs().max() / ref.abs().max()) < BAR


def test_one_inf_reaches_its_windows_only(cuda):
    """one Inf in x: exactly the outputs whose 3x3 window over the upsampled image contains it are non-finite"""
    shape = (1, 4, 8, 80, 64)
    r = _operands(shape)
    x = r["x"].clone()
    i, j = 2, 5
    x[0, i, j, 77] = float("inf")
    out, names = _run("fwd", x.to(cuda), _w(r["w"], cuda), r["bias"].to(cuda), None)
    assert names == [NAME["fwd"]]
    want = torch.zeros(1, 8, 16, 64, dtype=torch.bool)
    want[0, max(2 * i - 1, 0):2 * i + 3, max(2 * j - 1, 0):2 * j + 3] = True
    assert torch.equal(~torch.isfinite(out.cpu()), want)
