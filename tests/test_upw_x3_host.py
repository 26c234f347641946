"""The split-bf16 arithmetic of the fp32 upsampler convolution (csrc/conv3_upwino.hip) on the CPU (tests/upw_x3_refs.py), and the
size query of its plane image of U.

* The emulated correct form and every single mistake (a dropped or doubled term, swapped planes, a stale double-buffer side, a
  missing K-tail mask) lie on opposite sides of the bar the GPU test holds the device to, on the scale sum |U| |V| carried
  through |A'| (forward) / |s| (dgrad).
* The emulation itself is the convolution: against torch's float64 conv3x3(nearest_upsample_2x(x)) and its input gradient.
* vae_wino_weight_bytes: 6 * 9 * N * roundup16(K) where the upsampler kernel serves, 4 x vae_wino_weight_floats elsewhere, 0 for a
  null argument."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import upw_x3_refs as R


@pytest.mark.parametrize("dgrad", [False, True])
@pytest.mark.parametrize("shape", [(1, 8, 16, 64, 64), (1, 4, 8, 72, 72)])
def test_correct_form_and_single_mistakes_lie_apart(shape, dgrad):
    """(1, 8, 16, 64, 64) is the GPU test's crafted case; 72 channels add the K tail (K % 16 == 8) and the odd step count"""
    _, _, _, _, e_ok, e_bad, errs = R.crafted_sides(*shape, 24, dgrad)
    bar = R.bar_between(e_ok, e_bad)
    print(f"{shape} dgrad {dgrad}: emulated {e_ok:.3e}, bar {bar:.3e}, smallest single mistake {e_bad:.3e}")
    assert e_ok < bar
    for name, e in errs.items():
        assert e > bar, (name, e, bar)
    assert len(errs) == (17 if shape[3] == 72 else 16)
    if shape[3] == 72:
        assert "K tail not masked" in errs


@pytest.mark.parametrize("dgrad", [False, True])
def test_emulation_is_the_convolution(dgrad):
    B, H, W, Ci, Co = 1, 4, 8, 40, 24
    g = torch.Generator().manual_seed(3)
    w = torch.randn(Co, 3, 3, Ci, generator=g)
    src = torch.randn((B, 2 * H, 2 * W, Co) if dgrad else (B, H, W, Ci), generator=g)
    w64 = w.double().permute(0, 3, 1, 2)
    if dgrad:
        hi = F.conv_transpose2d(src.double().permute(0, 3, 1, 2), w64, None, 1, 1)
        ref = F.avg_pool2d(hi, 2, divisor_override=1).permute(0, 2, 3, 1)
    else:
        ref = F.conv2d(F.interpolate(src.double().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest"), w64, None, 1, 1).permute(0, 2, 3, 1)
    M64, _ = R.reference(R.transform_v(src, dgrad, torch.float64), R.transform_u(w, dgrad, torch.float64))
    assert float((R.image(R.output(M64, dgrad), B, H, W, dgrad) - ref).abs().max()) < 1e-11 * float(ref.abs().max())
    got = R.image(R.output(R.emulate(R.transform_v(src, dgrad), R.transform_u(w, dgrad)), dgrad), B, H, W, dgrad)
    assert float((got.double() - ref).abs().max()) < 1e-5 * float(ref.abs().max())


def test_split_planes_sum_to_the_value():
    a = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 2.0 ** torch.arange(-20, 21).repeat(100)[:4096]
    hi, mid, lo = R.split(a)
    assert float(((hi.double() + mid.double() + lo.double() - a.double()).abs() / a.abs().double()).max()) <= 2.0 ** -24
    for p in (hi, mid, lo):
        assert torch.equal(p, p.bfloat16().float())


def _args(ops, mode_dgrad, B, H, W, Ci, Co, kind="c3up"):
    keep = torch.zeros(64)
    base = (keep.data_ptr() + 15) // 16 * 16  # a 16-byte aligned address that only stands for the operands' alignment
    if kind == "c3up":
        a = ops.up2x_dgrad_args(B, H, W, Co, Ci, prec=ops.PREC_F32) if mode_dgrad else ops.fwd_args("c3up", B, H, W, Ci, Co, Ci, prec=ops.PREC_F32)
    else:
        a = ops.dgrad_args(kind, B, H, W, Co, Ci, prec=ops.PREC_F32) if mode_dgrad else ops.fwd_args(kind, B, H, W, Ci, Co, Ci, prec=ops.PREC_F32)
    a.A, a.W, a.C = C.c_void_p(base), C.c_void_p(base), C.c_void_p(base)
    return a, keep


def test_weight_bytes_query():
    from vaehip import ops
    from vaehip.lib import lib
    dll = lib.load()
    assert dll.vae_wino_weight_bytes(None) == 0
    up16 = lambda k: (k + 15) // 16 * 16  # noqa: E731
    served = 0
    for dg in (False, True):
        for Ci, Co in ((64, 32), (72, 36), (36, 72), (80, 64), (128, 160), (512, 512), (32, 32), (60, 64)):
            for H, W in ((4, 8), (8, 16), (6, 16)):
                a, keep = _args(ops, dg, 2, H, W, Ci, Co)
                N, K = (Ci, Co) if dg else (Co, Ci)
                nbytes, floats = int(lib.query("vae_wino_weight_bytes", C.byref(a))), int(lib.query("vae_wino_weight_floats", C.byref(a)))
                assert floats == 9 * N * K
                if lib.query("vae_wino_ok", C.byref(a)):
                    served += 1
                    assert K % 8 == 0 and K >= 64 and H % 4 == 0
                    assert nbytes == 6 * 9 * N * up16(K), (dg, Ci, Co, H, W, nbytes)
                else:
                    assert nbytes == 4 * floats
    assert served >= 12
    # elsewhere: the plain 3x3 layers (F(4x4) with 36 positions, F(2x2) with 16) read fp32 U
    seen = set()
    for dg in (False, True):
        for (H, W, Ci, Co) in ((16, 32, 64, 64), (8, 8, 64, 64), (16, 32, 64, 96), (6, 10, 32, 48)):
            a, keep = _args(ops, dg, 1, H, W, Ci, Co, kind="c3")
            floats = int(lib.query("vae_wino_weight_floats", C.byref(a)))
            seen.add(floats // (Ci * Co))
            assert int(lib.query("vae_wino_weight_bytes", C.byref(a))) == 4 * floats
    assert seen == {16, 36}
