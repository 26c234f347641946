"""The six kernels of the <= 4-channel convolutions (csrc/skinny.hip, conv_thin_bf16.hip, wgrad_thin_bf16.hip) at the smallest
shapes that run the control flow no other test below full model size reaches: several tiles per split of the weight gradient
(prefetch under the MFMAs, the barrier pair around the restaging, the scale / shift reload when a range enters the next image, an
empty trailing split), two tiles per workgroup of conv_thin_bf16_kernel, every XF instantiation, 1..4 channels on the narrow
side, a channel-block tail, ragged last tiles, tiles that straddle images, the stride-2 / upsampled / 1x1 geometries.  Launches go
through the C ABI with explicit argument blocks (vae_igemm_rows, vae_wgrad with nsplit set by hand, vae_reduce_splits[2]); cases,
float64 references and criteria are in tests/thin_refs.py, proved on the CPU by tests/test_thin_edges_host.py.

Every case asserts the kernel instantiation its block selects and the storage-flag query; outputs, slabs, bias partials and
tracker buffers start as NaN; a storage wider than the contraction holds 1e4 in the unused channels; every launch is made twice
and must give the same bits; a split without tiles writes zeros.

Bars: forward / dgrad 2e-5, weight gradient 3e-5, with a fused GroupNorm 5e-5 of max |v| (a bf16 result: ulp / 2 per element on
top); db within n * 2^-24 * sum |dy|; tracker partials within the summed element allowances + 128 * 2^-24 * sum |v|; a matrix-pipe
kernel with a transform: max(4 x fp32-CPU, the bar above).  Measured worst per kernel (profiles/thin_edges_measured.json):
  conv_smallk_kernel: out 2.7e-07 of 2.0e-05 [smallk-n96]; track 2.4e-03 of 1.0e+00 [smallk-n96]
  conv_smalln_kernel: out 1.4e-06 of 2.0e-05 [smalln-5-k128of128-n4-xf1]
  conv_thin_bf16_kernel: out 3.7e-08 of 2.0e-05 [thin-large]; track 4.9e-02 of 1.0e+00 [thin-straddle]
  conv_thinn_bf16_kernel: out 2.2e-04 of 9.0e-04 (fp32 CPU 2.2e-04) [thinn-1-k32of32-n3-xf2]
  wgrad_smallk_kernel: dW 8.8e-07 of 3.0e-05 [smallk-k1-3of4-m128-ns1]; db 3.0e-02 of 1.0e+00 [smallk-c3s2-k1-3of4-m128-ns1]
  wgrad_thin_bf16_kernel: dW 3.7e-05 of 1.5e-04 (fp32 CPU 3.7e-05) [thin-k2-m3-n128-xf2-ns12]; db 1.6e-04 of 1.0e+00 [thin-k2-m3-n128-xf1-ns5]
"""
import ctypes as C

import pytest
import torch

import streaming_refs as sr
import thin_refs as T
from guarded import GuardedPool
from vaehip import ops
from vaehip.lib import lib

pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Plain:
    """operands copied to the device, results that start as NaN"""

    def __init__(self, dev):
        self.dev = dev

    def put(self, t, label):
        return t.to(self.dev)

    def alloc(self, shape, dtype, label):
        return torch.full(shape, float("nan"), dtype=dtype, device=self.dev)


class Guarded:
    """the same between poisoned guards (an all-ones word is a NaN as fp32 and as bf16)"""

    def __init__(self, pool):
        self.pool = pool

    def put(self, t, label):
        return self.pool.put(t, label)

    def alloc(self, shape, dtype, label):
        return self.pool.alloc(shape, dtype, label=label)


def launch_rows(c, mem, ready=None):
    """-> out [M,N], tracker partials [tiles,N] or None"""
    o = T.rows_operands(c)
    a = T.rows_block(c, ops)
    M, N, _, _ = T.rows_dims(c)
    src, w = mem.put(o.src, "src"), mem.put(o.w, "w")
    bias = mem.put(o.bias, "bias") if c.bias else None
    scale = mem.put(o.scale, "scale") if c.xf != T.XF_NONE else None
    shift = mem.put(o.shift, "shift") if c.xf != T.XF_NONE else None
    if ready is not None:
        ready()
    out = mem.alloc((M, N), torch.bfloat16 if c.out16 else torch.float32, "out")
    trk = mem.alloc(((M + T.TP - 1) // T.TP, N), torch.float32, "track") if c.track else None
    a.A, a.W, a.C, a.bias, a.track, a.scale, a.shift = _p(src), _p(w), _p(out), _p(bias), _p(trk), _p(scale), _p(shift)
    with ops.option("no_thin_mfma", int(c.no_thin)):
        assert T.kernel_name(lib, "vae_igemm_kernel_name", a) == c.kernel
        assert lib.query("vae_conv_io16_ok", C.byref(a)) == 1
        lib.call("vae_igemm_rows", C.byref(a), _stream())
    return out, trk


def launch_wgrad(c, mem, ready=None):
    """-> slab [ns, Co*taps*Ci] (None with one split), bias partials [ns,Co] or None, dW [Co,taps,Ci], db or None"""
    o = T.wg_operands(c)
    a = T.wg_block(c, ops)
    taps = T.taps_of(c.kind)
    n = c.Co * taps * c.Ci
    x, dy = mem.put(o.x, "x"), mem.put(o.dy, "dy")
    scale = mem.put(o.scale, "scale") if c.xf != T.XF_NONE else None
    shift = mem.put(o.shift, "shift") if c.xf != T.XF_NONE else None
    if ready is not None:
        ready()
    dW = mem.alloc((c.Co, taps, c.Ci), torch.float32, "dW")
    slab = mem.alloc((c.ns, n), torch.float32, "slab") if c.ns > 1 else None
    bpart = mem.alloc((c.ns, c.Co), torch.float32, "bias partials") if c.bias else None
    db = mem.alloc((c.Co,), torch.float32, "db") if c.bias else None
    a.dY, a.X, a.scale, a.shift = _p(dy), _p(x), _p(scale), _p(shift)
    a.out, a.partial, a.bias_partial = (_p(dW) if c.ns == 1 else None), _p(slab), _p(bpart)
    with ops.option("no_thin_mfma", int(c.no_thin)):
        assert T.kernel_name(lib, "vae_wgrad_kernel_name", a) == c.kernel
        assert lib.query("vae_wgrad_io16_ok", C.byref(a)) == 1
        lib.call("vae_wgrad", C.byref(a), _stream())
    if slab is not None and bpart is not None:
        lib.call("vae_reduce_splits2", _p(slab), c.ns, n, _p(dW), _p(bpart), c.Co, _p(db), _stream())
    elif slab is not None:
        lib.call("vae_reduce_splits", _p(slab), c.ns, n, _p(dW), _stream())
    elif bpart is not None:
        lib.call("vae_reduce_splits", _p(bpart), c.ns, c.Co, _p(db), _stream())
    return slab, bpart, dW, db


def _sync(what):
    """a device fault ends the session: nothing more is launched after it"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: the device reported {e}", returncode=3)


def _check(c, figs):
    for what, (measured, limit, fp) in figs.items():
        sr.check("thin_edges/" + T.family(c.kernel), f"{c.id} {what}", measured, limit, fp, strict=False)


def _same_bits(a, b) -> bool:
    """(a NaN left behind is the same bits too: the value check is what refuses it)"""
    it = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.view(it), b.view(it))


def _rows(c, dev):
    one, two = launch_rows(c, Plain(dev)), launch_rows(c, Plain(dev))
    _sync(c.id)
    for a, b, nm in zip(one, two, ("out", "tracker partials")):
        assert a is None or _same_bits(a, b), f"{c.id}: two launches differ in {nm}"
    out, trk = one
    _check(c, T.rows_figures(c, out.cpu(), None if trk is None else trk.cpu()))


def _empty_splits_are_zero(c, slab, bpart):
    for s, (t0, t1) in enumerate(T.wg_ranges(c)):
        if t0 == t1:
            assert slab is not None and not slab[s].any(), f"{c.id}: empty split {s} left a slab that is not zero"
            assert bpart is None or not bpart[s].any(), f"{c.id}: empty split {s} left bias partials that are not zero"


def _wgrad(c, dev):
    one, two = launch_wgrad(c, Plain(dev)), launch_wgrad(c, Plain(dev))
    _sync(c.id)
    for a, b, nm in zip(one, two, ("slab", "bias partials", "dW", "db")):
        assert a is None or _same_bits(a, b), f"{c.id}: two launches differ in {nm}"
    slab, bpart, dW, db = one
    _check(c, T.wg_figures(c, dW.cpu(), None if db is None else db.cpu()))
    _empty_splits_are_zero(c, slab, bpart)


# ---------------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("c", [c for c in T.WG_CASES if T.family(c.kernel) == "wgrad_smallk_kernel"], ids=lambda c: c.id)
def test_wgrad_smallk(cuda, c):
    """the tile loop of the VALU kernel: 12, 3 and 1 tiles per split, ranges across image boundaries (the scale / shift reload),
    an empty last split, a ragged last tile with image boundaries inside tiles, a 160-channel wide side, the stride-2, upsampled
    and 1x1 geometries, the wide side stored as bf16"""
    _wgrad(c, cuda)


@pytest.mark.parametrize("c", [c for c in T.WG_CASES if T.family(c.kernel) == "wgrad_thin_bf16_kernel"], ids=lambda c: c.id)
def test_wgrad_thin_bf16(cuda, c):
    """the tile loop of the matrix-pipe kernel: the prefetch of tile t + 1 under the MFMAs of tile t, the barrier pair around the
    restaging, the scale / shift reload at an image boundary, an empty last split; <true,0>, <false,0>, <false,1>, <false,2>"""
    _wgrad(c, cuda)


# ---------------------------------------------------------------------------------------------------- rows form
@pytest.mark.parametrize("c", T.SMALLK_CASES, ids=lambda c: c.id)
def test_conv_smallk(cuda, c):
    _rows(c, cuda)


@pytest.mark.parametrize("c", T.THIN_CASES, ids=lambda c: c.id)
def test_conv_thin_bf16(cuda, c):
    _rows(c, cuda)


def test_conv_thin_bf16_two_tiles_per_workgroup(cuda):
    """2055 tiles: 2 per workgroup, the register prefetch across them and the reuse of the output / tracker tiles in LDS; the
    last of the 1028 workgroups gets one tile"""
    _rows(T.THIN_LARGE, cuda)


@pytest.mark.parametrize("c", T.SMALLN_CASES, ids=lambda c: c.id)
def test_conv_smalln(cuda, c):
    _rows(c, cuda)


@pytest.mark.parametrize("c", T.THINN_CASES, ids=lambda c: c.id)
def test_conv_thinn_bf16(cuda, c):
    _rows(c, cuda)


# ---------------------------------------------------------------------------------------------------- guarded memory
GUARDED = ("smallk-c3-ragged", "thin-straddle", "smalln-4-k128of128-n3-xf2", "thinn-4-k128of128-n3-xf2",
           "smallk-k1-3of4-m128-ns5", "smallk-k2-m3-n128-xf2-ns5", "thin-k1-3of4-m128-ns5", "thin-k2-m3-n128-xf2-ns5")


@pytest.mark.parametrize("cid", GUARDED)
def test_in_guarded_memory(cuda, cid):
    """one launch of each kernel on its multi-tile case between poisoned guards (the weight gradients with 5 splits, the empty
    one included): nothing outside a tensor touched, no operand changed, every element of every result written"""
    pool = GuardedPool(cuda)
    mem = Guarded(pool)
    if cid in {c.id for c in T.WG_CASES}:
        c = T.wg_case(cid)
        slab, bpart, dW, db = launch_wgrad(c, mem, ready=pool.snapshot)
        figs = lambda: T.wg_figures(c, dW.cpu(), None if db is None else db.cpu())   # noqa: E731
    else:
        c = T.rows_case(cid)
        out, trk = launch_rows(c, mem, ready=pool.snapshot)
        figs = lambda: T.rows_figures(c, out.cpu(), None if trk is None else trk.cpu())   # noqa: E731
    _sync(cid)
    assert pool.violations() == [] and pool.changed() == [] and pool.unwritten_report() == []
    assert T.passes(figs()), (cid, figs())
    if cid in {c.id for c in T.WG_CASES}:
        _empty_splits_are_zero(c, slab, bpart)
