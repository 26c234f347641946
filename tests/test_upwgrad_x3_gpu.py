"""The fp32 upsampler weight gradient on split-bf16 products (csrc/wgrad3_upwino.hip): a step takes TWO units of 8 low-resolution
pixels (the K = 16 of v_mfma_f32_32x32x16_bf16), each in an LDS stage of its own; an odd last unit of a split is paired with a
unit of zeros, and the two units of a pair may lie in two rows or two images.  vae_wgrad_wino + vae_wgrad_wino_reduce are called
through vaehip.lib with an explicit split count at the smallest shapes at which the pairing can go wrong, against torch's conv2d
weight gradient of the upsampled input in float64 on the host.

Bars: dW within 3e-5 of max |dW| (the split bar of tests/test_wgrad_x3_gpu.py).  The bias partials are the exact loop's bit for
bit: compared with the `make -C csrc upwgrad_x3_off` library where it lies beside the loaded one (its dW error is printed beside
the split loop's), and always with a float32 replay of the kernel's order of sums (tests/upwgrad_x3_refs.py).  Every launch is made
twice (bit-identical slabs); a split without units leaves zeros.  The crafted case compares the slab itself with float64 on the
scale sum |V| |D| under the bar tests/test_upwgrad_x3_host.py derives: between the emulated correct form's error and the smallest
single mistake's (a dropped or doubled term, swapped planes, a stale partner unit).

Shapes (B, Hs, Ws, Ci, Co): Ws = 8 with Hs = 1..5 and B = 2 gives 2, 4, 6, 8, 10 units, one per row: pairs cross rows everywhere and
images where Hs is odd; in 2 and 4 splits the ranges hold 0, 1, 2, 3 and 5 units (2 units in 4 splits: two empty splits; 10 in 4:
3 + 3 + 3 + 1).  (2, 3, 16, 64, 256): two units per row, four tiles of Cin x Cout.  (1, 3, 8, 32, 128) in a tensor of 40 channels
whose last 8 hold NaN: Cs > N."""
import ctypes as C
import functools
import os

import pytest
import torch

import upwgrad_x3_refs as R
from guarded import GuardedPool
from vaehip import ops
from vaehip.lib import LIB_PATH, WgradArgs, lib

pytestmark = pytest.mark.gpu

BAR = 3e-5
OFF_LIB = os.path.join(os.path.dirname(LIB_PATH), "libvaehip_upwgrad_x3off.so")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(dev):
    return lambda shape, label: torch.full(shape, float("nan"), device=dev)


@functools.lru_cache(maxsize=None)
def _operands(shape, seed=11):
    """host operands of a shape and their float64 gradients, made once and shared (never modified)"""
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(seed + sum(p * v for p, v in zip((3, 5, 7, 11, 13), shape)))
    x, dy = torch.randn(B, H, W, Ci, generator=g), torch.randn(B, 2 * H, 2 * W, Co, generator=g)
    gw, gb = R.dw_f64(x, dy)
    return dict(x=x, dy=dy, gw=gw, gb=gb)


@functools.lru_cache(maxsize=None)
def _off_dll():
    """the exact-products build, if it was made (make -C csrc upwgrad_x3_off); loaded beside the default library"""
    if not os.path.exists(OFF_LIB):
        return None
    lib.load()
    dll = C.CDLL(OFF_LIB)
    dll.vae_wgrad_wino.restype, dll.vae_wgrad_wino.argtypes = C.c_int, [C.POINTER(WgradArgs), C.c_void_p]
    return dll


def _launch(x, dy, shape, ns, bias, alloc, dll=None, Cs=None):
    """slab, bias partials, dW, db of one vae_wgrad_wino (of `dll`, default: the loaded library) + vae_wgrad_wino_reduce"""
    B, H, W, Ci, Co = shape
    a = ops.wgrad_args("c3up", B, H, W, Cs or Ci, Co, Ci, prec=ops.PREC_F32)
    slab = alloc((ns, 9 * Ci * Co), "slab")
    bpart = alloc((ns, Co), "bias slab") if bias else None
    dW = alloc((Co, 3, 3, Ci), "dW")
    db = alloc((Co,), "db") if bias else None
    a.dY, a.X = _p(dy), _p(x)
    a.nsplit, a.partial, a.bias_partial = ns, _p(slab), _p(bpart)
    assert int(lib.query("vae_wgrad_wino_positions", C.byref(a))) == 9, "not the upsampler kernel's launch"
    if dll is None:
        lib.call("vae_wgrad_wino", C.byref(a), _stream())
    else:
        assert dll.vae_wgrad_wino(C.byref(a), _stream()) == 0
    lib.call("vae_wgrad_wino_reduce", _p(slab), ns, 9, Ci, Co, None, _p(dW), _p(bpart), _p(db), _stream())
    return slab, bpart, dW, db


def _err(dW, ref):
    return float((dW.double().cpu() - ref).abs().max() / ref.abs().max())


def _case(dev, shape, ns, x=None, Cs=None):
    B, H, W, Ci, Co = shape
    r = _operands(shape)
    xd, dyd = (r["x"] if x is None else x).to(dev), r["dy"].to(dev)
    for bias in (False, True):
        what = f"{shape} nsplit {ns} bias {bias}"
        one = _launch(xd, dyd, shape, ns, bias, _nan(dev), Cs=Cs)
        two = _launch(xd, dyd, shape, ns, bias, _nan(dev), Cs=Cs)
        for a, b, nm in zip(one, two, ("slab", "bias partials", "dW", "db")):
            assert a is None or torch.equal(a, b), f"{what}: two launches differ in {nm}"
        e = _err(one[2], r["gw"])
        off = _off_dll()
        e_off = None
        if off is not None:
            ex = _launch(xd, dyd, shape, ns, bias, _nan(dev), dll=off, Cs=Cs)
            e_off = _err(ex[2], r["gw"])
            if bias:
                assert torch.equal(one[1].view(torch.int32), ex[1].view(torch.int32)), f"{what}: bias partials differ from the exact build's"
        print(f"{what}: dW max err / max |dW| = {e:.3e}" + ("" if e_off is None else f" (exact build {e_off:.3e})"))
        assert e <= BAR, f"{what}: dW off by {e:.3e} of max |dW| (bar {BAR})"  # (a NaN fails the comparison too)
        if bias:
            want = R.bias_partials_f32(r["dy"], W, ns)
            assert torch.equal(one[1].cpu().view(torch.int32), want.view(torch.int32)), f"{what}: bias partials differ from the float32 replay"
        for s, (_, nu) in enumerate(R.unit_ranges(B * H * (W // 8), ns)):
            if nu == 0:  # a split without units still writes its slab of zeros
                assert not one[0][s].any(), f"{what}: empty split {s} left a slab that is not zero"
                assert not bias or not one[1][s].any(), f"{what}: empty split {s} left bias partials that are not zero"


@pytest.mark.parametrize("ns", [1, 2, 4])
@pytest.mark.parametrize("H", [1, 2, 3, 4, 5])
def test_units_per_split(cuda, H, ns):
    _case(cuda, (2, H, 8, 32, 128), ns)


@pytest.mark.parametrize("ns", [1, 2, 4])
def test_several_tiles(cuda, ns):
    """Ws = 16, Cin 64, Cout 256: 12 units, four tiles; only the tiles of the first Cin block write bias partials"""
    _case(cuda, (2, 3, 16, 64, 256), ns)


def test_padded_x_with_poison(cuda):
    """Cin = 32 in a tensor of 40 channels whose channels 32..39 hold NaN"""
    shape = (1, 3, 8, 32, 128)
    x = torch.full((1, 3, 8, 40), float("nan"))
    x[..., :32] = _operands(shape)["x"]
    _case(cuda, shape, 2, x=x, Cs=40)


@pytest.mark.parametrize("ns", [1, 2])
def test_crafted_operands(cuda, ns):
    """3 units (one image of 3 x 8) of operands every term has a known share of: the slab, summed over the splits, against float64;
    one split pairs (0, 1) and (2, zeros), two splits (0, 1) and (2, zeros) in ranges of their own"""
    shape = B, H, W, Ci, Co = 1, 3, 8, 32, 128
    x, dy = R.crafted_xy(B, H, W, Ci, Co, 24)
    V, D = R.transforms(x, dy)
    ref, S = R.reference(V, D)
    e_ok = R.rel_err(R.emulate(V, D, ns).sum(dim=0), ref, S)
    e_bad = min(R.rel_err(M, ref, S) for M in R.mistakes(V, D, ns).values())
    bar = R.bar_between(e_ok, e_bad)
    one = _launch(x.to(cuda), dy.to(cuda), shape, ns, False, _nan(cuda))
    two = _launch(x.to(cuda), dy.to(cuda), shape, ns, False, _nan(cuda))
    assert torch.equal(one[0], two[0]), "two launches differ in the slab"
    M = one[0].double().sum(dim=0).reshape(9, Ci, Co).cpu()
    live = S > 0
    assert not bool(M[~live].any()), "an element without products is not exactly zero"
    e = float(((M - ref).abs()[live] / S[live]).max())
    print(f"nsplit {ns}: device {e:.3e}, emulated {e_ok:.3e}, smallest single mistake {e_bad:.3e}, bar {bar:.3e} of sum|V||D|")
    assert e < bar


def test_in_guarded_memory(cuda):
    """5 units in 2 splits (3 + 2), operands and outputs between poisoned guards: every element written, nothing outside touched,
    no operand changed"""
    shape = (1, 5, 8, 32, 128)
    r = _operands(shape)
    pool = GuardedPool(cuda)
    x, dy = pool.put(r["x"].to(cuda), "x"), pool.put(r["dy"].to(cuda), "dy")
    pool.snapshot()
    _, _, dW, db = _launch(x, dy, shape, 2, True, lambda s, label: pool.alloc(s, label=label))
    torch.cuda.synchronize()
    assert pool.violations() == [] and pool.changed() == [] and pool.unwritten_report() == []
    assert _err(dW, r["gw"]) <= BAR
    n = r["dy"].shape[0] * r["dy"].shape[1] * r["dy"].shape[2]  # db: a sum of n fp32 values per channel in some order
    assert bool(((db.double().cpu() - r["gb"]).abs() <= n * 2.0 ** -24 * r["dy"].double().abs().sum(dim=(0, 1, 2))).all())
