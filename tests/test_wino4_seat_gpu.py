"""The main loop of the fp32 Winograd F(4x4,3x3) convolution (csrc/conv3_wino4.hip) at the step counts and borders the other
F(4x4) cases do not reach: they all contract over 128, 256 or 512 channels (even step counts), so the loop's odd tail and the
smallest contraction never ran.  A halo DMA issued at the wrong place, or a wait that retires the wrong operations, shows
exactly there -- as a wrong border pixel or as a difference between two launches, not as a hang.

Every case is held to a float64 convolution of the same operands (computed once per shape on the host and shared) and must
have been served by conv3_wino4_kernel<0> (ops.LaunchProfiler).  Bars: those of
test_kernels_gpu.py::test_winograd_forward_and_dgrad, 4e-5 of the tensor's max for forward and dgrad (2x the worst element
measured for F(4x4) against float64 at 128..512 channels; a shorter contraction rounds less); the epilogue's GroupNorm moments
against a separate gn_stats pass at 1e-5 and the GroupNorm-backward epilogue against the three-pass form at 2e-6, as there.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from guarded import GuardedPool, guarded

pytestmark = pytest.mark.gpu

BAR = 4e-5
KERNEL = "conv3_wino4_kernel<0>"
# contraction lengths with 8, 9, 10 and 17 steps of 8 channels
KS = [64, 72, 80, 136]
FWD_MAPS = [(1, 16, 32, 64), (2, 32, 64, 128)]  # B, H, W, Cout
DGRAD_MAPS = [(1, 16, 32), (2, 32, 64)]         # B, H, W (Cin = 64, contraction over Cout = K)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _dev(t):  # NCHW host -> NHWC device
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _w_dev(w):  # OIHW host -> logical OIHW view of OHWI device memory
    return w.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)


_REF = {}


def _case(B, H, W, Ci, Co, offset=0.2, scale=1.3):
    """seeded operands of a layer and their float64 forward / input gradient, once per shape (never modified)"""
    key = (B, H, W, Ci, Co, offset, scale)
    if key not in _REF:
        gen = torch.Generator().manual_seed(101 + 3 * Ci + 5 * Co + 7 * H + B)
        x = torch.randn(B, Ci, H, W, generator=gen) * scale + offset
        w = torch.randn(Co, Ci, 3, 3, generator=gen) / math.sqrt(9 * Ci)
        bias = torch.randn(Co, generator=gen)
        dy = torch.randn(B, Co, H, W, generator=gen) * scale + offset
        res = torch.randn(B, Co, H, W, generator=gen)
        y64 = F.conv2d(x.double(), w.double(), bias.double(), 1, 1)
        dx64 = F.conv_transpose2d(dy.double(), w.double(), None, 1, 1)
        _REF[key] = dict(x=x, w=w, bias=bias, dy=dy, res=res, y64=y64, dx64=dx64,
                         xd=_dev(x), wd=_w_dev(w), bd=bias.cuda(), dyd=_dev(dy), resd=_dev(res))
    return _REF[key]


def _profiled(fn):
    """fn() with a launch profiler installed -> (result, kernel names)"""
    from vaehip import ops
    prof = ops.PROFILER = ops.LaunchProfiler()
    try:
        out = fn()
    finally:
        ops.PROFILER = None
    return out, [r[0] for r in prof.records]


def _fwd(r, **kw):
    from vaehip import ops
    return _profiled(lambda: ops.conv_fwd(r["xd"], r["wd"], r["bd"], "c3", **kw))


def _dgrad(r, H, W, **kw):
    from vaehip import ops
    return _profiled(lambda: ops.conv_dgrad(r["dyd"], r["wd"], "c3", (H, W), **kw))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("B,H,W,Co", FWD_MAPS)
@pytest.mark.parametrize("K", KS)
def test_forward_step_counts(cuda, K, B, H, W, Co):
    """8, 9, 10 and 17 steps: the two-step loop ends on either side, the odd tail runs, one tile and sixteen"""
    r = _case(B, H, W, K, Co)
    y, names = _fwd(r)
    err = _rel(_nchw(y), r["y64"])
    print(f"forward B {B} {H}x{W} {K}->{Co}: {err:.2e} of max")
    assert names == [KERNEL], names
    assert err < BAR


@pytest.mark.parametrize("B,H,W", DGRAD_MAPS)
@pytest.mark.parametrize("K", KS)
def test_dgrad_step_counts(cuda, K, B, H, W):
    """the dgrad contracts over Cout = K"""
    r = _case(B, H, W, 64, K)
    dx, names = _dgrad(r, H, W)
    err = _rel(_nchw(dx), r["dx64"])
    print(f"dgrad B {B} {H}x{W} 64<-{K}: {err:.2e} of max")
    assert names == [KERNEL], names
    assert err < BAR


@pytest.mark.parametrize("H,W", [(16, 32), (48, 96)])
def test_halo_and_seams(cuda, H, W):
    """one tile with all four borders padded, and 3 x 3 tiles whose centre tile has real neighbours on every side; 9 steps.  The
    maps are a constant plus noise: a halo pixel that is stale (another chunk's), missing or not zero where the padding is moves
    a border output by the size of a weight times the constant, thousands of times the bar."""
    rf, rd = _case(1, H, W, 72, 64, offset=1.0, scale=1.0), _case(1, H, W, 64, 72, offset=1.0, scale=1.0)
    y, nf = _fwd(rf)
    dx, nd = _dgrad(rd, H, W)
    assert nf == [KERNEL] and nd == [KERNEL], (nf, nd)
    ef, ed = (_nchw(y).double().cpu() - rf["y64"]).abs() / rf["y64"].abs().max(), (_nchw(dx).double().cpu() - rd["dx64"]).abs() / rd["dx64"].abs().max()
    print(f"halo {H}x{W}: forward {float(ef.max()):.2e} dgrad {float(ed.max()):.2e} of max")
    for e in (ef, ed):
        border = torch.cat([e[..., 0, :].flatten(), e[..., -1, :].flatten(), e[..., :, 0].flatten(), e[..., :, -1].flatten()])
        seams = torch.cat([e[..., 15:17, :].flatten(), e[..., :, 31:33].flatten()]) if H > 16 else border
        assert float(border.max()) < BAR and float(seams.max()) < BAR and float(e.max()) < BAR


def test_forward_epilogue_residual_and_statistics(cuda):
    """bias + residual + the GroupNorm moments of the output, as the step's resnet convolutions run"""
    from vaehip import ops
    B, H, W, C = 2, 32, 64, 128
    r = _case(B, H, W, C, C)
    y, names = _fwd(r, res=r["resd"], gstat_groups=32)
    assert names == [KERNEL], names
    err = _rel(_nchw(y), r["y64"] + r["res"].double())
    print(f"forward + residual: {err:.2e} of max")
    assert err < BAR
    assert hasattr(y, "_gstat") and y._gstat[2] == (H // 16) * (W // 32)
    g, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    st_f, st_p = ops.gn_stats(y, g, b), ops.gn_stats(y.clone(), g, b)  # from the epilogue's moments / from a pass over the tensor
    assert _rel(st_f.mean, st_p.mean) < 1e-5 and _rel(st_f.rstd, st_p.rstd) < 1e-5


def test_dgrad_epilogue_groupnorm_backward(cuda):
    """the dgrad that leaves the first pass of the GroupNorm(+SiLU) backward, against the three-pass form"""
    from vaehip import ops
    B, H, W, Ci, Co = 2, 16, 32, 128, 64
    r = _case(B, H, W, Ci, Co)
    gen = torch.Generator().manual_seed(5)
    gd, bd = (1 + 0.3 * torch.randn(Ci, generator=gen)).cuda(), (0.2 * torch.randn(Ci, generator=gen)).cuda()
    st = ops.gn_stats(r["xd"], gd, bd)
    ctx = ops.GnCtx(r["xd"], st, gd, bd, True, 32)
    dA_f, names = _dgrad(r, H, W, gnb=ctx)
    dA_p, _ = _dgrad(r, H, W)
    assert names == [KERNEL], names
    assert hasattr(dA_f, "_gnb") and dA_f._gnb[1] == (H // 16) * (W // 32) and not hasattr(dA_p, "_gnb")
    assert torch.equal(dA_f, dA_p)
    assert _rel(_nchw(dA_f), r["dx64"]) < BAR

    def bwd(dA):
        dg, db = torch.full((Ci,), float("nan"), device="cuda"), torch.full((Ci,), float("nan"), device="cuda")
        return ops.gn_bwd(r["xd"], dA, st, gd, bd, True, None, dg, db), dg, db

    for a, b, nm in zip(bwd(dA_f), bwd(dA_p), ("dx", "dgamma", "dbeta")):
        e = _rel(a, b)
        print(f"GroupNorm backward from the epilogue's sums, {nm}: {e:.2e}")
        assert e < 2e-6, nm


def test_fifty_launches_are_bitwise_equal(cuda):
    """a DMA that lands after its barrier, or a transform that reads a halo before it has landed, differs from launch to launch"""
    rf, rd, re = _case(2, 32, 64, 72, 128), _case(2, 32, 64, 64, 72), _case(2, 32, 64, 128, 128)
    (y0, _), (d0, _), (e0, _) = _fwd(rf), _dgrad(rd, 32, 64), _fwd(re, res=re["resd"], gstat_groups=32)
    for i in range(1, 50):
        (y, nf), (d, nd), (e, ne) = _fwd(rf), _dgrad(rd, 32, 64), _fwd(re, res=re["resd"], gstat_groups=32)
        assert nf == nd == ne == [KERNEL]
        assert torch.equal(y, y0), f"launch {i}: forward differs"
        assert torch.equal(d, d0), f"launch {i}: dgrad differs"
        assert torch.equal(e, e0) and torch.equal(e._gstat[0], e0._gstat[0]), f"launch {i}: forward with statistics differs"


def _guarded_run(cuda, rf, rd, H, W, off_maps, off_w, off_bias):
    from vaehip import ops
    pool = GuardedPool(cuda)
    x, dy = pool.put(rf["xd"], "x", offset_bytes=off_maps), pool.put(rd["dyd"], "dy", offset_bytes=off_maps)
    wf = pool.put(rf["wd"].permute(0, 2, 3, 1), "w forward", offset_bytes=off_w).permute(0, 3, 1, 2)
    wd = pool.put(rd["wd"].permute(0, 2, 3, 1), "w dgrad", offset_bytes=off_w).permute(0, 3, 1, 2)
    bias = pool.put(rf["bd"], "bias", offset_bytes=off_bias)
    pool.snapshot()
    with guarded(pool, ops):
        y, nf = _profiled(lambda: ops.conv_fwd(x, wf, bias, "c3"))
        d, nd = _profiled(lambda: ops.conv_dgrad(dy, wd, "c3", (H, W)))
    torch.cuda.synchronize()
    assert pool.violations() == [] and pool.changed() == [] and pool.unwritten_report() == []
    return y, d, nf, nd


@pytest.mark.parametrize("off", [0, 4])
def test_in_guarded_memory(cuda, off):
    """the 9-step forward and dgrad between poisoned guards: no guard byte changed, every output element written, no operand
    changed, the result bitwise that of the ordinary run.  off = 4 twice: with the bias 4 bytes past a 256-byte boundary -- the
    one operand F(4x4) takes at any alignment -- the kernel still serves both launches; with every operand 4 bytes off the
    dispatcher must NOT hand the launch to it (its halo DMA and fragment loads move 16 bytes at a time; csrc/dispatch.cpp
    rows_vec, conv3_wino4_eligible), the guards stay intact under the kernel that serves instead and the result is the float64
    convolution's within the same bar."""
    B, H, W = 2, 32, 64
    rf, rd = _case(B, H, W, 72, 128), _case(B, H, W, 64, 72)
    (y0, _), (d0, _) = _fwd(rf), _dgrad(rd, H, W)
    y, d, nf, nd = _guarded_run(cuda, rf, rd, H, W, 0, 0, off)
    assert nf == [KERNEL] and nd == [KERNEL], (nf, nd)
    assert torch.equal(y, y0) and torch.equal(d, d0)
    if off:
        y, d, nf, nd = _guarded_run(cuda, rf, rd, H, W, off, off, off)
        assert len(nf) == 1 and len(nd) == 1 and "wino" not in nf[0] and "wino" not in nd[0], (nf, nd)
        assert _rel(_nchw(y), rf["y64"]) < BAR and _rel(_nchw(d), rd["dx64"]) < BAR
