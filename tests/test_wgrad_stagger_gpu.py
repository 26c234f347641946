"""The control flow of the fp32 Winograd weight gradient (csrc/wgrad3_wino.hip) whose waves 4..7 issue the MFMAs of a step's last
channel blocks at the top of the NEXT step and drain them once after the loop: vae_wgrad_wino + vae_wgrad_wino_reduce called
through vaehip.lib with an explicit split count, at the smallest shapes at which that flow can go wrong (0..5 units per split,
a unit range across an image boundary, several tiles under all three workgroup-id mappings, bias gradient on and off, the
GroupNorm(+SiLU) instantiations), against torch's conv2d weight gradient in float64 on the host.

Bars: dW within 3e-5 of max |dW| (the bar of the wgrad3_wino_kernel<0> cases of tests/conv_routes.py; measured worst on these
shapes: 3.3e-7, profiles/wgrad_stagger_measured.json).  db is a sum of n = B*H*W fp32 values per channel in some order:
|db - ref| <= n * 2^-24 * sum |dy|.  A split without units writes a slab and a bias partial of zeros.  Every launch is made
twice: bit-identical slabs.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from guarded import GuardedPool
from vaehip import ops
from vaehip.lib import lib

pytestmark = pytest.mark.gpu

BAR = 3e-5
U = 2.0 ** -24


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_REF = {}


def _operands(dev, B, H, W, Ci, Co, xf):
    """seeded operands and their float64 weight / bias gradient, computed once per shape and shared (never modified)"""
    key = (B, H, W, Ci, Co, xf)
    if key not in _REF:
        g = torch.Generator(device="cpu").manual_seed(1 + sum(p * v for p, v in zip((3, 5, 7, 11, 13, 17), key)))
        x = torch.randn((B, H, W, Ci), generator=g)
        dy = torch.randn((B, H, W, Co), generator=g)
        scale = torch.rand((B, Ci), generator=g) + 0.5
        shift = torch.randn((B, Ci), generator=g) * 0.5
        act = x.double()
        if xf != ops.XF_NONE:
            act = act * scale.double()[:, None, None, :] + shift.double()[:, None, None, :]
            if xf == ops.XF_AFFINE_SILU:
                act = act * torch.sigmoid(act)
        w0 = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
        (gw,) = torch.autograd.grad(F.conv2d(act.permute(0, 3, 1, 2), w0, None, 1, 1), w0, dy.double().permute(0, 3, 1, 2))
        _REF[key] = dict(x=x.to(dev), dy=dy.to(dev), scale=scale.to(dev), shift=shift.to(dev), gw=gw.permute(0, 2, 3, 1).contiguous(),
                         gb=dy.double().sum(dim=(0, 1, 2)), gb_abs=dy.double().abs().sum(dim=(0, 1, 2)))
    return _REF[key]


def _launch(r, B, H, W, Ci, Co, ns, xf, bias, alloc, x=None, dy=None):
    """slab, bias partials, dW, db of one vae_wgrad_wino + vae_wgrad_wino_reduce; outputs start as NaN"""
    a = ops.wgrad_args("c3", B, H, W, Ci, Co, Ci, xf=xf, prec=ops.PREC_F32)
    slab = alloc((ns, 16 * Ci * Co), "slab")
    bpart = alloc((ns, Co), "bias slab") if bias else None
    dW = alloc((Co, 3, 3, Ci), "dW")
    db = alloc((Co,), "db") if bias else None
    a.dY, a.X = _p(r["dy"] if dy is None else dy), _p(r["x"] if x is None else x)
    a.nsplit, a.partial, a.bias_partial = ns, _p(slab), _p(bpart)
    if xf != ops.XF_NONE:
        a.scale, a.shift = _p(r["scale"]), _p(r["shift"])
    lib.call("vae_wgrad_wino", C.byref(a), _stream())
    lib.call("vae_wgrad_wino_reduce", _p(slab), ns, 16, Ci, Co, None, _p(dW), _p(bpart), _p(db), _stream())
    return slab, bpart, dW, db


def _nan(dev):
    return lambda shape, label: torch.full(shape, float("nan"), device=dev)


def _check(r, dW, db, what):
    ref = r["gw"]
    err = float((dW.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"{what}: dW max err / max |dW| = {err:.3e}")
    assert err <= BAR, f"{what}: dW off by {err:.3e} of max |dW| (bar {BAR})"  # (a NaN fails the comparison too)
    if db is not None:
        n = r["x"].shape[0] * r["x"].shape[1] * r["x"].shape[2]
        e = (db.double().cpu() - r["gb"]).abs()
        worst = float((e / (n * U * r["gb_abs"])).max())
        print(f"{what}: db max err / bound = {worst:.3f}")
        assert worst <= 1.0, f"{what}: db beyond n * 2^-24 * sum |dy| by a factor {worst:.3f}"


def _case(dev, B, H, W, Ci, Co, ns, xf=ops.XF_NONE):
    r = _operands(dev, B, H, W, Ci, Co, xf)
    units = B * (H // 2) * (W // 16)
    per = -(-units // ns)
    for bias in (False, True):
        what = f"B {B} {H}x{W} Cin {Ci} Cout {Co} nsplit {ns} xf {xf} bias {bias}"
        one = _launch(r, B, H, W, Ci, Co, ns, xf, bias, _nan(dev))
        two = _launch(r, B, H, W, Ci, Co, ns, xf, bias, _nan(dev))
        _check(r, one[2], one[3], what)
        for a, b, nm in zip(one, two, ("slab", "bias partials", "dW", "db")):
            assert a is None or torch.equal(a, b), f"{what}: two launches differ in {nm}"
        for s in range(ns):
            if s * per >= units:  # a split without units: nothing held back, and still its slab of zeros
                assert not one[0][s].any(), f"{what}: empty split {s} left a slab that is not zero"
                assert not bias or not one[1][s].any(), f"{what}: empty split {s} left bias partials that are not zero"


# B, H (W = 16): 1, 2, 3, 4, 5 units; (2, 2) and (2, 4) put an image boundary inside a unit range
@pytest.mark.parametrize("ns", [1, 2, 4])
@pytest.mark.parametrize("B,H", [(1, 2), (2, 2), (1, 6), (2, 4), (1, 10)])
def test_units_per_split(cuda, B, H, ns):
    """0..5 units per split: 3 units in 4 splits leave the last split empty, 1 unit drains right after the prologue, odd and
    even counts end the two-step loop on either side"""
    _case(cuda, B, H, 16, 32, 128, ns)


@pytest.mark.parametrize("ns", [2, 3, 8])
def test_several_tiles(cuda, ns):
    """4 tiles (Cin 64, Cout 256) of 8 units: the workgroup-id mapping for nsplit % 8 == 0, for 2 | 4 splits and the plain one"""
    _case(cuda, 1, 8, 32, 64, 256, ns)


@pytest.mark.parametrize("xf,B,H,W,Ci,ns", [(ops.XF_AFFINE_SILU, 2, 4, 16, 64, 1), (ops.XF_AFFINE, 3, 2, 32, 32, 2)])
def test_groupnorm_instantiations(cuda, xf, B, H, W, Ci, ns):
    """wgrad3_wino_kernel<2> and <1>: a unit range that crosses an image re-reads the GroupNorm rows"""
    _case(cuda, B, H, W, Ci, 128, ns, xf)


def test_in_guarded_memory(cuda):
    """operands, slab, bias partials, dW and db between poisoned guards (3 units in 4 splits: the empty split's zeros included):
    every element written, nothing outside touched, no operand changed"""
    B, H, W, Ci, Co, ns = 1, 6, 16, 32, 128, 4
    r = _operands(cuda, B, H, W, Ci, Co, ops.XF_NONE)
    pool = GuardedPool(cuda)
    x, dy = pool.put(r["x"], "x"), pool.put(r["dy"], "dy")
    pool.snapshot()
    _, _, dW, db = _launch(r, B, H, W, Ci, Co, ns, ops.XF_NONE, True, lambda shape, label: pool.alloc(shape, label=label), x=x, dy=dy)
    torch.cuda.synchronize()
    assert pool.violations() == [] and pool.changed() == [] and pool.unwritten_report() == []
    _check(r, dW, db, "guarded")
