"""The fp32 upsampler convolution with 128 output channels per workgroup (csrc/conv3_upwino.hip, VAE_UPW_NB_FWD / VAE_UPW_NB_DG = 4):
a wave multiplies its A planes against four 32-channel blocks of U, the ninth position's four blocks sit on waves 4..7, a block
that lies wholly at or beyond N is skipped (no MFMAs, no epilogue pass) and the ragged block is masked lane by lane.  The scheme
of tests/test_upw_x3_gpu.py: ops.conv_fwd / ops.conv_dgrad with kind "c3up", the kernel names from the profiler records, every
launch made twice (bit-identical), the results compared with float64 on the host within 1e-5 of max |ref|.  The tests hold under
either width (a direction built with two blocks runs the same shapes through two channel tiles where four blocks have one).

Shapes (B, H, W, Ci, Co), the forward's N = Co: (1,4,8,64,128) one tile, exactly one full channel tile, four steps; (1,4,8,80,96)
N < 128: the fourth block skipped, five steps (the odd double-buffer parity); (1,4,8,72,132) K % 16 == 8 and a second channel tile
whose only live block is ragged (4 columns); (1,4,8,64,160) a second channel tile with one whole live block; (2,8,16,128,256)
several tiles, two channel tiles, even and odd workgroup ids, B = 2.  The dgrad's K = Co and N = Ci, so the mirrors (1,4,8,128,64),
(1,4,8,96,80), (2,8,16,256,128) put it at N = 128, 96 and 256.  Both directions run on every shape vae_wino_ok serves.

The crafted case (tests/upw_x3_refs.py) runs at (1,8,16,64,128) in both directions and, for the dgrad's four blocks, at the mirror
(1,8,16,128,64); its bar lies between the emulated correct form's error and the smallest single mistake's, and every 32-channel
block is held to it on its own."""
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

SHAPES = [(1, 4, 8, 64, 128), (1, 4, 8, 80, 96), (1, 4, 8, 72, 132), (1, 4, 8, 64, 160), (2, 8, 16, 128, 256),
          (1, 4, 8, 128, 64), (1, 4, 8, 96, 80), (2, 8, 16, 256, 128)]
# what vae_wino_ok refuses (K = Ci forward, Co dgrad: a multiple of 8, at least 64)
REFUSED = {("dgrad", (1, 4, 8, 72, 132))}
SERVED = [(op, s) for s in SHAPES for op in ("fwd", "dgrad") if (op, s) not in REFUSED]
NAME = {"fwd": "conv3_upwino_kernel<false>", "dgrad": "conv3_upwino_kernel<true>"}
BAR = 1e-5


@functools.lru_cache(maxsize=None)
def _operands(shape, seed=11):
    """host operands of a shape, made once: x, dy, w (OHWI), bias and the float64 forward / dgrad"""
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(seed)
    x, dy = torch.randn(B, H, W, Ci, generator=g), torch.randn(B, 2 * H, 2 * W, Co, generator=g)
    w, bias = torch.randn(Co, 3, 3, Ci, generator=g) / (3.0 * Ci ** 0.5), torch.randn(Co, generator=g)
    y = F.conv2d(F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest"), w.double().permute(0, 3, 1, 2), bias.double(), 1, 1)
    hi = F.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None, 1, 1)  # gradient wrt the upsampled image
    dx = F.avg_pool2d(hi, 2, divisor_override=1)
    return dict(x=x, dy=dy, w=w, bias=bias, fwd=y.permute(0, 2, 3, 1).contiguous(), dgrad=dx.permute(0, 2, 3, 1).contiguous())


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


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max() / ref.abs().max())


def test_which_shapes_are_served(cuda):
    got = set()
    keep = torch.zeros(64, device=cuda)
    for s in SHAPES:
        B, H, W, Ci, Co = s
        for op in ("fwd", "dgrad"):
            a = ops.fwd_args("c3up", B, H, W, Ci, Co, Ci) if op == "fwd" else ops.up2x_dgrad_args(B, H, W, Co, Ci)
            a.A, a.W, a.C = ops._p(keep), ops._p(keep), ops._p(keep)
            if not lib.query("vae_wino_ok", C.byref(a)):
                got.add((op, s))
    assert got == REFUSED


@pytest.mark.parametrize("op,shape", SERVED)
def test_against_float64(cuda, op, shape):
    r = _operands(shape)
    B, H, W, Ci, Co = shape
    if op == "fwd":
        out = _twice(op, r["x"].to(cuda), _w(r["w"], cuda), r["bias"].to(cuda), None)
    else:
        out = _twice(op, r["dy"].to(cuda), _w(r["w"], cuda), None, (H, W))
    ref = r[op]
    e = _err(out, ref)
    print(f"{op} {shape}: {e:.3e} of max |ref|")
    assert out.shape == ref.shape and e < BAR


def test_tail_with_poison(cuda):
    """Ci = 72 in a tensor of 80 channels whose channels 72..79 hold NaN (Cs > K): the last step's second octet is that memory,
    and all five live blocks of the two channel tiles must stay finite"""
    shape = (1, 4, 8, 72, 132)
    r = _operands(shape)
    x = torch.full((1, 4, 8, 80), float("nan"))
    x[..., :72] = r["x"]
    out = _twice("fwd", x.to(cuda), _w(r["w"], cuda), r["bias"].to(cuda), None)
    assert bool(torch.isfinite(out).all())
    assert _err(out, r["fwd"]) < BAR


@pytest.mark.parametrize("op,shape", [("fwd", (1, 8, 16, 64, 128)), ("dgrad", (1, 8, 16, 64, 128)), ("dgrad", (1, 8, 16, 128, 64))])
def test_crafted_operands(cuda, op, shape):
    """no plane missing, doubled or swapped in any 32-channel block (forward and the mirrored dgrad: N = 128, blocks 0..3 and the
    ninth position's four blocks on waves 4..7)"""
    B, H, W, Ci, Co = shape
    dg = op == "dgrad"
    src, w, ref, scale, e_ok, e_bad, _ = R.crafted_sides(B, H, W, Ci, Co, 24, dg)
    bar = R.bar_between(e_ok, e_bad)
    out = _twice(op, src.to(cuda), _w(w, cuda), None, (H, W)).cpu()
    ref, scale = R.image(ref, B, H, W, dg), R.image(scale, B, H, W, dg)
    N = out.shape[-1]
    errs = [R.rel_err(out[..., q:q + 32], ref[..., q:q + 32], scale[..., q:q + 32]) for q in range(0, N, 32)]
    print(f"{op} {shape}: device per block {['%.3e' % e for e in errs]}, emulated {e_ok:.3e}, smallest single mistake {e_bad:.3e}, bar {bar:.3e} of sum|U||V|")
    assert max(errs) < bar


@pytest.mark.parametrize("op,shape", [("fwd", (1, 4, 8, 72, 132)), ("dgrad", (1, 4, 8, 132, 72))])
def test_in_guarded_memory(cuda, op, shape):
    """operands, Wu and the output between poisoned guards at N = 132 (a second channel tile with 4 live columns: three skipped
    blocks and a ragged one): every element written, nothing outside touched, no operand changed"""
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
    assert _err(out, r[op]) < BAR
