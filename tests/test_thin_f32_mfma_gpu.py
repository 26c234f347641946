"""wgrad_smallk_kernel<SMALL_X,XF> (csrc/skinny.hip) with its matrix-pipe body: the 3x3 weight gradient with a <= 4-channel side
and a wide side of >= 64 channels runs as v_mfma_f32_16x16x4_f32 over 128-pixel tiles; 1x1 layers, a wide operand that is odd or
not 8-byte (bf16: 4-byte) aligned, and a fused GroupNorm over tiles that straddle images keep the VALU loop behind a
grid-uniform branch of the same kernel.  The cases are the smallest that reach every loop end of both bodies:

  map 3 x 10 x 10    300 pixels: three tiles, the last with 44 rows, image boundaries inside tiles (a fused GroupNorm: VALU loop)
  map 2 x 16 x 16    four whole tiles, two per image: a fused GroupNorm on the matrix pipe, the scale / shift reload between images
  wide channels      128, and 136 (a second channel block of 8: its waves 1..3 and lanes 4..15 of wave 0 own no channel)
  narrow channels    1, 3, 4 of a 4-channel storage that holds 1e4 in the unused channels (side 1), 1, 3, 4 rows of dY (side 2)
  xf                 0, 1, 2
  wide storage       fp32 and bf16
  taps               9 and 1
  splits             1, 5 (the last empty: zeros) and the planned count (vae_wgrad_plan, asserted)
  operands           the wide and the narrow tensor 4 bytes off their alignment (fp32 wide: VALU loop; bf16 wide: matrix pipe)

Every case launches through vae_wgrad (+ vae_reduce_splits[2]) between poisoned guards with NaN-prefilled results: no guard byte
touched, no operand changed, every element of every result written, the reported kernel name the case's, dW within 3e-5 of max
|dW| (5e-5 with a fused GroupNorm) of the float64 reference of tests/thin_refs.py, db within n * 2^-24 * sum |dy|.  Rows 37 .. 47 of
the padded product, the narrow channels past the contraction and the columns past the wide side must contribute nothing: the
unused storage channels hold 1e4 and the guards behind the last pixel hold NaN bit patterns.  Twenty launches of the multi-tile
cases give the same bits.

Measured worst on MI355X (profiles/thin_f32_measured.json): dW 6.2e-07 of 3.0e-05 [k2-m3-n128-xf0-ns1], with a fused GroupNorm
6.8e-07 of 5.0e-05 [w-k2-m3-n128-xf1-ns1]; db 5.7e-03 of 1.0 [k1-1of4-m128-ns1].  26 tests in 2.9 s.

conv_smallk_kernel and conv_smalln_kernel<XF> keep their VALU bodies; their cases stay in tests/test_thin_edges_gpu.py.
"""
import ctypes as C

import pytest
import torch

import test_thin_edges_gpu as E
import thin_refs as T
from guarded import GuardedPool
from vaehip import ops
from vaehip.lib import lib

pytestmark = pytest.mark.gpu

MAP_B = T.MAP_B            # (3, 10, 10)
MAP_W = (2, 16, 16)


def _c(tag, side, narrow, wide, ns, **k):
    return T._wg("f32m-" + tag, side, narrow, 4 if side == 1 else None, wide, ns, **k)


def _w16(**k):
    return dict(wide16=True, no_thin=True, bf16=True, **k)


# (case, planned: ns is what vae_wgrad_plan answers, {operand label: bytes off its alignment})
CASES = (
    # side 1: the narrow side is X
    (_c("k1-1of4-m128", 1, 1, 128, 1, shape=MAP_B), False, {}),
    (_c("k1-3of4-m128", 1, 3, 128, 5, shape=MAP_B), False, {}),
    (_c("k1-4of4-m136", 1, 4, 136, 3, shape=MAP_B), True, {}),
    (_c("k1-3of4-m136-nobias", 1, 3, 136, 5, shape=MAP_B, bias=False), False, {}),
    # side 2: the narrow side is dY; XF 0 on the ragged map, XF 1 / 2 on both maps
    (_c("k2-m3-n128-xf0", 2, 3, 128, 1, shape=MAP_B), False, {}),
    (_c("k2-m1-n136-xf0", 2, 1, 136, 5, shape=MAP_B), False, {}),
    (_c("k2-m4-n128-xf0", 2, 4, 128, 3, shape=MAP_B), True, {}),
    (_c("k2-m3-n128-xf1", 2, 3, 128, 3, shape=MAP_B, xf=1), True, {}),
    (_c("k2-m3-n136-xf2", 2, 3, 136, 5, shape=MAP_B, xf=2), False, {}),
    (_c("w-k2-m3-n128-xf1", 2, 3, 128, 1, shape=MAP_W, xf=1), False, {}),
    (_c("w-k2-m4-n136-xf2", 2, 4, 136, 5, shape=MAP_W, xf=2), False, {}),
    (_c("w-k2-m3-n128-xf2", 2, 3, 128, 4, shape=MAP_W, xf=2), True, {}),
    # the wide side stored as bf16
    (_c("w16-k1-3of4-m128", 1, 3, 128, 5, shape=MAP_B, **_w16()), False, {}),
    (_c("w16-k2-m3-n128-xf0", 2, 3, 128, 1, shape=MAP_B, **_w16()), False, {}),
    (_c("w16-w-k2-m3-n136-xf2", 2, 3, 136, 4, shape=MAP_W, **_w16(xf=2)), True, {}),
    # 1x1 layers
    (_c("c1-k1-4of4-m128", 1, 4, 128, 3, shape=MAP_B, kind="c1"), True, {}),
    (_c("c1-k2-m3-n128", 2, 3, 128, 1, shape=MAP_B, kind="c1"), False, {}),
    # operands 4 bytes off their alignment
    (_c("mis-k1-3of4-m128", 1, 3, 128, 5, shape=MAP_B), False, {"dy": 4, "x": 4}),
    (_c("mis-k2-m3-n136-xf0", 2, 3, 136, 3, shape=MAP_B), True, {"x": 4, "dy": 4}),
    (_c("mis-w-k2-m3-n128-xf2", 2, 3, 128, 1, shape=MAP_W, xf=2), False, {"x": 4}),
    (_c("mis-w16-k1-3of4-m136", 1, 3, 136, 5, shape=MAP_B, **_w16()), False, {"dy": 4}),
    (_c("mis-w16-w-k2-m3-n128-xf2", 2, 3, 128, 4, shape=MAP_W, **_w16(xf=2)), True, {"x": 4, "dy": 4}),
)
TWENTY = ("smallk-f32m-k1-3of4-m128-ns5", "smallk-f32m-k2-m1-n136-xf0-ns5", "smallk-f32m-w-k2-m4-n136-xf2-ns5", "smallk-f32m-w16-k1-3of4-m128-ns5")


class Offset(E.Guarded):
    """guarded operands, some of them placed a few bytes off their alignment"""

    def __init__(self, pool, off):
        super().__init__(pool)
        self.off = off

    def put(self, t, label):
        return self.pool.put(t, label, offset_bytes=self.off.get(label, 0))


def _planned(c) -> int:
    a = T.wg_block(c, ops)
    ns, fus = C.c_int32(0), C.c_int32(0)
    with ops.option("no_thin_mfma", int(c.no_thin)):
        lib.call("vae_wgrad_plan", C.byref(a), C.byref(ns), C.byref(fus))
    return ns.value


@pytest.mark.parametrize("c,planned,off", CASES, ids=lambda v: v.id if isinstance(v, T.Wg) else None)
def test_wgrad_smallk_in_guarded_memory(cuda, c, planned, off):
    assert c.kernel.startswith("wgrad_smallk_kernel<")
    if planned:
        assert _planned(c) == c.ns
    pool = GuardedPool(cuda)
    slab, bpart, dW, db = E.launch_wgrad(c, Offset(pool, off), ready=pool.snapshot)   # (asserts the kernel name the block selects)
    E._sync(c.id)
    assert pool.violations() == [] and pool.changed() == [] and pool.unwritten_report() == []
    figs = T.wg_figures(c, dW.cpu(), None if db is None else db.cpu())
    for what, (measured, limit, _) in figs.items():
        print(f"{c.id} {what}: {measured:.3e} of {limit:.1e}")
    assert T.passes(figs), (c.id, figs)
    E._empty_splits_are_zero(c, slab, bpart)


@pytest.mark.parametrize("cid", TWENTY)
def test_twenty_launches_same_bits(cuda, cid):
    c = {k.id: k for k, _, _ in CASES}[cid]
    runs = [E.launch_wgrad(c, E.Plain(cuda)) for _ in range(20)]
    E._sync(cid)
    for r in runs[1:]:
        for a, b, nm in zip(runs[0], r, ("slab", "bias partials", "dW", "db")):
            assert a is None or E._same_bits(a, b), f"{cid}: two of twenty launches differ in {nm}"
    assert T.passes(T.wg_figures(c, runs[0][2].cpu(), None if runs[0][3] is None else runs[0][3].cpu()))
