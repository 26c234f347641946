"""The bf16 halo-tile, wide-tile and resident-weight 1x1 kernels at the ends of their loops (a helper module, not a test).

Three things, shared by tests/test_bf16_tile_edges_host.py (no GPU) and tests/test_bf16_tile_edges_gpu.py:

  plan(case)       a Python restatement of what each launch does with its shape, from the constants of csrc/bf16_tile_common.h and
                   the launchers of csrc/conv3_tile_bf16.hip, conv3_wide_bf16.hip and conv1_bf16.hip: tiles, grid, the persistent
                   schedule (first_tile, tiles per workgroup), channel chunks, conv1's blocks per wave.  The host test holds it to
                   the library's own answers and holds every regime a case claims to the plan of that case.
  CASES            one line per launch: family, direction, form, shape, storage, epilogues, the instantiation the library must
                   name, the regimes the case is there for, and the line of the kernel that regime exercises.
  reference(...)   F.conv2d / conv_transpose2d in float64 on the operands AS THE KERNEL READS THEM (bf16 images as they are, fp32
                   operands r16()-rounded, r16() of the weights), bias and residual added in float64; computed once per case.

Criterion: bf16_refs.ratio(stage) <= 1 with the project's bars (bf16_refs.BAR_DIRECT, BAR_STATS, BAR_GN_APPLY; the tracker's 1e-5
of tests/test_kernels_gpu.py::test_conv_track_epilogue) -- none chosen here.

Every launch goes through the library entry with a block from ops.fwd_args / dgrad_args / phase_args (ops._launch_igemm, as
tests/test_act16_gpu.py does): the output is then allocated HERE, NaN-prefilled and with any row stride, and shapes ops.conv_fwd
will not route still reach their kernel -- an A16 forward with Cin % 64 != 0 (vae_bf16_act_image_ok also wants the weight gradient
on the halo-tile kernel), a gradient image likewise (vae_bf16_grad_image_ok), a bias or an output stride on a dgrad.  The cases
marked OPS are also run through ops.conv_fwd / ops.conv_dgrad and must give the same bits.

Maps are a constant plus noise (tests/test_wino4_seat_gpu.py::test_halo_and_seams): a halo pixel that is stale, missing or not zero
where the padding is moves a border output by a weight times the constant.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

import bf16_refs as br
from bf16_refs import BAR_DIRECT, BAR_GN_APPLY, BAR_STATS, Stage, r16, ratio  # noqa: F401  (re-exported: the tests take them here)

BAR_TRACK = 1e-5   # tests/test_kernels_gpu.py::test_conv_track_epilogue

# ---------------------------------------------------------------------------------------------------- constants of the kernels
BK, BN, TW = 32, 128, 32                       # bf16_tile_common.h, namespace conv
TH = {"tile": 4, "wide": 8}                    # conv3_tile_bf16.hip / conv3_wide_bf16.hip
GRID_CAP = {"tile": 512, "wide": 256}          # launch_conv3_tile_bf16 / launch_wide (minus the option wide_reserved_cus)
WIDE_MIN_TILES = 192                           # conv3_wide_bf16_eligible
C1_BN, C1_MIN_M, C1_LDS = 128, 32768, 150 * 1024   # conv1_bf16.hip

# ---------------------------------------------------------------------------------------------------- regimes
KCH1_K8 = "tile: kchunks == 1, K = 8 (every chunk first and last; c < p.K cuts inside the chunk)"
KCH1_K32 = "tile: kchunks == 1, K = 32 (a whole chunk)"
KCH1_CROSS = "tile: kchunks == 1 AND a next tile: the cross-tile prefetch (last, vn, n0n, c0n) starts in the first step"
KCH2_PART = "tile: kchunks == 2, last chunk partial (K = 40)"
KCH3_PART = "tile: kchunks == 3, last chunk partial (K = 72)"
T_N40, T_N136, T_N264 = "tile: N = 40 (one partial channel tile)", "tile: N = 136", "tile: N = 264 (tilesN = 3, last tile 8 channels)"
T_OUT32 = "tile: N tail with fp32 output"
T_OUT16_RES_BIAS = "tile: N tail with bf16 output + bf16 residual + bias (pack_pair)"
T_TRACK_TAIL = "tile: tracker epilogue on an N tail (cur.n0 + tid < p.N)"
T_G_NOT8 = "tile: G % 8 != 0 with ntiles > 8 (first_tile is the identity)"
T_ABOVE_GRID_TN3 = "tile: ntiles just above 512 with tilesN = 3 (a workgroup's tiles differ in n0, some cross an image)"
T_TAIL_NEXT = "tile: a tail tile as the prefetched next tile, bf16 stores"
T_THREE = "tile: ntiles > 1024, some workgroups run three tiles"
T_XF = "tile: fused transform (XF = 1 and 2, A16 = false), K tail, B >= 2, a second tile in another image"
T_UP = "tile: the UP instantiation (virtual nearest-2x upsample)"
T_PHASE_TAIL = "tile: phase set (tapmask, a_step / c_step) with an N tail"
T_DGRAD = "tile: dgrad (contracts over Cout, transposing weight reads)"
T_STATS = "tile: statistics epilogue"
W_NCH2, W_NCH6 = "wide: nch == 2 (K = 64)", "wide: nch == 6 (K = 192)"
W_N40, W_N136, W_N264 = "wide: N = 40", "wide: N = 136", "wide: N = 264"
W_192 = "wide: ntiles == 192, the smallest launch"
W_195 = "wide: 192 < ntiles < 256 with G % 8 != 0"
W_260 = "wide: ntiles slightly above 256 (a few workgroups take a second tile)"
W_513_TN3 = "wide: ntiles >= 513 with tilesN = 3 (tilesN does not divide the grid: consecutive tiles change n0; three tiles)"
W_OUT32, W_OUT16 = "wide: fp32 output", "wide: bf16 output"
W_RES_K192 = "wide: residual with K > 128"
W_DGRAD_TAIL = "wide: dgrad from a gradient image, the tail in Cin"
W_PHASE_TAIL = "wide: phase case (KS = 2) with an N tail"
W_STATS = "wide: statistics epilogue"
C1_KN = "conv1: K in {128, 256, 512} x N in {128, 512}"
C1_MIN = "conv1: M = 32768"
C1_PLUS32 = "conv1: M = 32768 + 32"
C1_2_AND_3 = "conv1: waves with 2 and with 3 blocks (both exits of the while loop in one launch)"



class Case(NamedTuple):
    name: str
    fam: str            # tile | wide | conv1
    dgrad: bool
    form: str           # plain | up (MODE_UP2X) | phase (the four tap masks of an upsampler, sub-sampled view)
    bhw: Tuple[int, int, int]   # the layer's forward input map (phase: the low-resolution map)
    Ci: int
    Co: int
    a: str              # operand: f32 (fp32, rounded while staged) | a16 (bf16 image) | xf1 | xf2 (fp32, transformed + rounded while staged)
    out16: bool
    epi: str            # letters: r residual (stored like the output)  b bias  s statistics  t tracker
    kernel: str         # the instantiation vae_igemm_kernel_name must give
    regimes: tuple
    why: str            # the line(s) of the kernel the case is there for

    @property
    def N(self):
        return self.Ci if self.dgrad else self.Co

    @property
    def K(self):
        return self.Co if self.dgrad else self.Ci


_T, _W, _C = "conv3_tile_bf16_kernel", "conv3_wide_bf16_kernel", "conv1_bf16_kernel"
CASES = [
    # ---- conv3_tile_bf16_kernel<DG,UP,XF,A16> (csrc/conv3_tile_bf16.hip)
    Case("t_k8_n40", "tile", False, "plain", (1, 4, 32), 8, 40, "f32", False, "", _T + "<false,false,0,false>",
         (KCH1_K8, T_N40, T_OUT32), "load_halo / load_w `c < p.K` at K = 8; one tile, no next tile (vn false at the only chunk)"),
    Case("t_k32_n136_o16", "tile", False, "plain", (2, 8, 64), 32, 136, "f32", True, "rb", _T + "<false,false,0,false>",
         (KCH1_K32, T_N136, T_OUT16_RES_BIAS), "epilogue `col < p.N` with pack_pair stores and rsR16 loads; first_tile remap at G = 16"),
    Case("t_k40_n264", "tile", False, "plain", (1, 12, 32), 40, 264, "a16", False, "", _T + "<false,false,0,true>",
         (KCH2_PART, T_N264, T_G_NOT8, T_OUT32), "A16 load_halo `c8 < p.K` at c8 = 40; load_w rows n >= 264; G = 9"),
    Case("t_dg_k72_n40_o16", "tile", True, "plain", (2, 8, 32), 40, 72, "a16", True, "", _T + "<true,false,0,true>",
         (KCH3_PART, T_DGRAD, T_N40), "dgrad load_w `k < p.K && n < Nv` (rows 72.. of chunk 2, columns 40..), frag_tr reads"),
    Case("t_k72_n40_o16", "tile", False, "plain", (1, 8, 64), 72, 40, "f32", True, "rb", _T + "<false,false,0,false>",
         (KCH3_PART, T_N40, T_OUT16_RES_BIAS), "pbias `col < p.N`, o16[] BUF_OOB for 88 of 128 columns"),
    Case("t_k40_n264_o16", "tile", False, "plain", (1, 12, 32), 40, 264, "a16", True, "rb", _T + "<false,false,0,true>",
         (T_N264, T_OUT16_RES_BIAS), "pack_pair on the 8-channel last tile"),
    Case("t_track_n136", "tile", False, "plain", (2, 8, 64), 8, 136, "f32", False, "bt", _T + "<false,false,0,false>",
         (T_TRACK_TAIL, T_N136, T_OUT32), "`tid < BN && cur.n0 + tid < p.N` and tsum of BUF_OOB columns"),
    Case("t_576_k32_o16", "tile", False, "plain", (3, 32, 256), 32, 264, "f32", True, "rb", _T + "<false,false,0,false>",
         (T_ABOVE_GRID_TN3, KCH1_CROSS, T_TAIL_NEXT), "main loop at kchunks == 1: load_halo(nxt, 0, has_next), load_w(n0n = nxt.n0); 576 tiles on 512 workgroups"),
    Case("t_dg_1280", "tile", True, "plain", (5, 64, 256), 136, 8, "a16", False, "", _T + "<true,false,0,true>",
         (T_THREE, KCH1_CROSS), "`t = tnext` twice: 1280 tiles on 512 workgroups (3 and 2 tiles)"),
    Case("t_xf2_576", "tile", False, "plain", (3, 32, 256), 40, 264, "xf2", False, "", _T + "<false,false,2,false>",
         (T_XF, T_ABOVE_GRID_TN3), "`min(c, p.K - 4)` on rsc / rsh of image nxt.b; padding zero AFTER the transform"),
    Case("t_xf1_528", "tile", False, "plain", (2, 44, 256), 8, 264, "xf1", True, "", _T + "<false,false,1,false>",
         (T_XF, KCH1_CROSS), "the same at K = 8: every second tile lies in image 1"),
    Case("t_up", "tile", False, "up", (1, 4, 32), 40, 40, "f32", False, "b", _T + "<false,true,0,false>",
         (T_UP, KCH2_PART, T_N40), "load_halo `sy = hy >> 1` with Hb = 2 Hs (what ops runs with PHASE_UPCONV off)"),
    Case("t_phase_fwd", "tile", False, "phase", (1, 8, 32), 40, 136, "f32", False, "b", _T + "<false,false,0,false>",
         (T_PHASE_TAIL, T_N136), "rmask / cmask / ngrp and the c_step offsets of off[] with BUF_OOB columns"),
    Case("t_phase_dg", "tile", True, "phase", (1, 8, 32), 40, 72, "f32", False, "r", _T + "<true,false,0,false>",
         (T_PHASE_TAIL, T_N40, T_DGRAD), "a_step reads of the high-resolution gradient; the phases add up through the fp32 residual"),
    Case("t_stats", "tile", False, "plain", (2, 8, 32), 40, 128, "a16", True, "bs", _T + "<false,false,0,true>",
         (T_STATS, KCH2_PART), "gstat_write of rounded pairs behind a partial chunk"),
    # ---- conv3_wide_bf16_kernel<DG,KS> (csrc/conv3_wide_bf16.hip)
    Case("w_k64_n40_192", "wide", False, "plain", (3, 64, 256), 64, 40, "a16", False, "", _W + "<false,3>",
         (W_NCH2, W_N40, W_192, W_OUT32), "`for (c = 0; c < nch; c += 2)` runs once; w_load_piece `n < p.N`; G = ntiles = 192"),
    Case("w_k192_n264_195", "wide", False, "plain", (5, 104, 32), 192, 264, "a16", True, "rb", _W + "<false,3>",
         (W_NCH6, W_N264, W_195, W_RES_K192, W_OUT16), "epi16(RES) with b2[] = 0x80000000 columns; first_tile identity at G = 195"),
    Case("w_k64_n136_260", "wide", False, "plain", (5, 104, 64), 64, 136, "a16", False, "b", _W + "<false,3>",
         (W_N136, W_260, W_OUT32), "w_advance / h_advance into a second tile on 4 workgroups, w_ok false on the other 252"),
    Case("w_576_tn3", "wide", False, "plain", (3, 64, 256), 64, 264, "a16", True, "", _W + "<false,3>",
         (W_513_TN3, W_N264, W_OUT16), "w_n0 = decode(w_t).n0 changes between a workgroup's tiles; 16-byte stores (wide_st) on the tail tile"),
    Case("w_dg_n136", "wide", True, "plain", (3, 64, 256), 136, 64, "a16", True, "", _W + "<true,3>",
         (W_DGRAD_TAIL, W_N136), "dgrad w_load_piece `k < p.K && n < p.N` with n in steps of 8; frag_tr on zero columns"),
    Case("w_dg_k192_n40", "wide", True, "plain", (3, 64, 256), 40, 192, "a16", False, "", _W + "<true,3>",
         (W_NCH6, W_N40, W_DGRAD_TAIL, W_OUT32), "three rounds of the 6-stage loop in dgrad, fp32 epilogue `col < p.N`"),
    Case("w_phase_fwd", "wide", False, "phase", (3, 64, 128), 64, 136, "a16", True, "b", _W + "<false,2>",
         (W_PHASE_TAIL, W_N136), "KS = 2: 2-stage chunks (fragments wait for the barrier), pstep = cs * ldc * 2 in the store offsets"),
    Case("w_phase_dg", "wide", True, "phase", (3, 64, 256), 40, 64, "a16", False, "r", _W + "<true,2>",
         (W_PHASE_TAIL, W_N40), "h_load_piece a_step offsets; roff / dxb of the dgrad tap block; fp32 residual adds the phases"),
    Case("w_stats", "wide", False, "plain", (3, 64, 256), 64, 128, "a16", True, "bs", _W + "<false,3>",
         (W_STATS, W_NCH2, W_192), "shifted_add_pair_fma / gstat_write behind the shortest main loop"),
    # ---- conv1_bf16_kernel<DG,KG> (csrc/conv1_bf16.hip); M = B H W
    Case("c_k128_n128", "conv1", False, "plain", (2, 128, 128), 128, 128, "a16", True, "b", _C + "<false,8>",
         (C1_KN, C1_MIN), "wpn = 256, stride 1024 = nblocks: one block per wave, exit after a0"),
    Case("c_k128_n512", "conv1", False, "plain", (1, 100, 328), 128, 512, "a16", True, "b", _C + "<false,8>",
         (C1_KN, C1_PLUS32, C1_2_AND_3), "stride 512, 1025 blocks: one wave runs 3 (exit after a0), the others 2 (exit at the while)"),
    Case("c_k256_n128", "conv1", False, "plain", (1, 100, 328), 256, 128, "a16", True, "b", _C + "<false,16>",
         (C1_KN, C1_PLUS32), "wpn = ceil(1025 / 4) = 257, stride 1028 > nblocks: three waves find no block (the while loop is not entered)"),
    Case("c_k256_n512", "conv1", False, "plain", (2, 128, 128), 256, 512, "a16", True, "b", _C + "<false,16>",
         (C1_KN, C1_MIN), "four slices: slice = blockIdx.x / wpn"),
    Case("c_k512_n128", "conv1", False, "plain", (2, 128, 128), 512, 128, "a16", True, "", _C + "<false,32>",
         (C1_KN, C1_MIN), "KG = 32: 32 x 16-byte A loads per block in flight"),
    Case("c_k512_n512", "conv1", False, "plain", (1, 100, 328), 512, 512, "a16", True, "b", _C + "<false,32>",
         (C1_KN, C1_PLUS32), "stride 256, 1025 blocks: waves with 4 and 5"),
    Case("c_dg_k128_n128", "conv1", True, "plain", (2, 128, 128), 128, 128, "a16", True, "", _C + "<true,8>",
         (C1_KN, C1_MIN), "dgrad slice [k][n] through frag_tr"),
    Case("c_dg_k128_n512", "conv1", True, "plain", (1, 100, 328), 512, 128, "a16", True, "", _C + "<true,8>",
         (C1_KN, C1_PLUS32, C1_2_AND_3), "dgrad: `Wh[k * p.sk + n0 + c]` for n0 = 0 .. 384; 2 and 3 blocks"),
    Case("c_dg_k256_n128", "conv1", True, "plain", (2, 128, 128), 128, 256, "a16", True, "", _C + "<true,16>",
         (C1_KN, C1_MIN), "dgrad KG = 16: 80 KB slice, one workgroup per CU, one block per wave"),
    Case("c_dg_k256_n512", "conv1", True, "plain", (1, 100, 328), 512, 256, "a16", True, "", _C + "<true,16>",
         (C1_KN, C1_PLUS32), "dgrad, 4 slices, waves with 4 and 5 blocks"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# what the GPU module runs beyond the plain comparison (names of CASES)
OPS = ("t_k8_n40", "w_k64_n40_192", "w_k64_n136_260", "w_576_tn3", "w_dg_n136", "c_k128_n512", "c_dg_k128_n512")  # also through ops: same bits
LDC_PAD = ("t_k40_n264", "t_dg_k72_n40_o16", "w_k64_n136_260", "w_576_tn3")  # ldc = N + 8 (conv1 takes ldc == N only)
GUARDED = ("t_576_k32_o16", "w_k64_n136_260", "c_k128_n512")                # N tail + ntiles above the grid (conv1: blocks above the stride)
REPEAT = ("t_576_k32_o16", "w_576_tn3", "c_k128_n512")                      # twenty launches, bitwise
OPTIONS = ("w_k64_n136_260", "w_576_tn3")                                    # no_wide (BAR_DIRECT) / wide_reserved_cus = 24 (bitwise)



def route(c: Case) -> str:
    """which way the case reaches its kernel, and why not through ops where it does not"""
    if c.name in OPS:
        return "direct launch, and ops.%s to the same bits" % ("conv_dgrad" if c.dgrad else "conv_fwd")
    if c.form == "phase":
        why = "one tap mask per launch with these weights (ops sums an upsampler's taps into effective kernels first)"
    elif c.form == "up":
        why = "ops takes the phase form while PHASE_UPCONV is on"
    elif set(c.epi) & set("st") or c.a in ("xf1", "xf2"):
        why = "the workspace and the scale / shift rows are this module's own, NaN-prefilled"
    elif "r" in c.epi or "b" in c.epi:
        why = "the output must be NaN-prefilled (ops allocates its own)"
    elif c.a == "a16" and not c.dgrad and c.Ci % 64:
        why = "vae_bf16_act_image_ok also wants the weight gradient on the halo-tile kernel (Cin % 64 == 0)"
    elif c.a == "a16" and c.dgrad and c.fam != "conv1":
        why = "vae_bf16_grad_image_ok also wants the weight gradient on the halo-tile kernel"
    else:
        why = "the output must be NaN-prefilled (ops allocates its own)"
    return "direct launch: " + why


PHASES = ((0, 0), (0, 1), (1, 0), (1, 1))
_PHASE_ROWS = {0: (0, 1), 1: (1, 2)}   # ops._PHASE_MASK


def tapmask(pa, pb):
    return sum(1 << (kh * 3 + kw) for kh in _PHASE_ROWS[pa] for kw in _PHASE_ROWS[pb])


# ---------------------------------------------------------------------------------------------------- the plan of a launch
def first_tile(G, w):
    """bf16_tile_common.h: consecutive ids on one XCD when the grid is a multiple of 8"""
    return (w % 8) * (G // 8) + w // 8 if G % 8 == 0 else w


def row_grid(c: Case):
    B, H, W = c.bhw
    return (B, 2 * H, 2 * W) if c.form == "up" else (B, H, W)


def decode(c: Case, t, p):
    """conv::decode: tile id -> (image, y0, x0, n0)"""
    lin, tn = divmod(t, p["tilesN"])
    r, tx = divmod(lin, p["tiles_x"])
    b, ty = divmod(r, p["tiles_y"])
    return b, ty * TH[c.fam], tx * TW, tn * BN


def plan(c: Case, reserved_cus: int = 0) -> dict:
    B, H, W = row_grid(c)
    N, K = c.N, c.K
    if c.fam == "conv1":
        dg = c.dgrad
        lds = K * (C1_BN + 32) * 2 if dg else C1_BN * (K + 8) * 2
        slices, nblocks = N // C1_BN, (B * H * W) // 32
        per_cu = 2 if (K // 16 <= 16 and 2 * lds <= C1_LDS) else 1
        wpn = max(1, min((256 * per_cu) // slices, (nblocks + 3) // 4))
        stride = 4 * wpn
        counts = sorted({len(range(v, nblocks, stride)) for v in range(stride)})
        return dict(M=B * H * W, slices=slices, nblocks=nblocks, lds=lds, per_cu=per_cu, wpn=wpn, stride=stride, grid=slices * wpn,
                    blocks_per_wave=counts, eligible=(K in (128, 256, 512) and N % C1_BN == 0 and (B * H * W) % 32 == 0 and
                                                       B * H * W >= C1_MIN_M and lds <= C1_LDS))
    th = TH[c.fam]
    tilesN, tiles_x, tiles_y = -(-N // BN), W // TW, H // th
    ntiles = tilesN * tiles_x * tiles_y * B
    G = min(ntiles, GRID_CAP[c.fam] - (reserved_cus if c.fam == "wide" else 0))
    kch = -(-K // BK)
    p = dict(tilesN=tilesN, tiles_x=tiles_x, tiles_y=tiles_y, ntiles=ntiles, grid=G, remap=G % 8 == 0, max_tiles=-(-ntiles // G),
             min_tiles=ntiles // G, kchunks=kch, last_partial=K % BK != 0, whole_tiles=(W % TW == 0 and H % th == 0))
    if c.fam == "tile":
        p["gstat_chunks"] = tiles_x * (H // 2) if (N % BN == 0 and not c.dgrad and c.form != "phase") else 0
    else:
        p["gstat_chunks"] = tiles_x * (H // 4) if (N % BN == 0 and not c.dgrad and c.form != "phase") else 0
        # conv3_wide_bf16_eligible, for the blocks this module builds (3x3 stride 1, both operands images, alpha 1)
        p["eligible"] = (c.a == "a16" and "t" not in c.epi and not ("r" in c.epi and K <= 128 and c.form != "phase") and c.form != "up"
                         and p["whole_tiles"] and K % (2 * BK) == 0 and N % 8 == 0 and N > 32 and ntiles >= WIDE_MIN_TILES
                         and not (c.form == "phase" and "s" in c.epi))
    return p


def tiles_of(c: Case, p: dict, w: int):
    """the tile ids workgroup w runs, in order"""
    return list(range(first_tile(p["grid"], w), p["ntiles"], p["grid"]))


# what it means for a plan to HAVE a regime (tests/test_bf16_tile_edges_host.py asserts it for every case that claims one)
def _wg_n0_changes(c, p):
    return any(decode(c, ts[i], p)[3] != decode(c, ts[i + 1], p)[3] for w in range(p["grid"]) for ts in [tiles_of(c, p, w)] for i in range(len(ts) - 1))


def _wg_crosses_image(c, p):
    return any(decode(c, ts[i], p)[0] != decode(c, ts[i + 1], p)[0] for w in range(p["grid"]) for ts in [tiles_of(c, p, w)] for i in range(len(ts) - 1))


def _tail_is_next(c, p):
    return any(decode(c, t, p)[3] + BN > c.N for w in range(p["grid"]) for t in tiles_of(c, p, w)[1:])


HOLDS = {
    KCH1_K8: lambda c, p: c.fam == "tile" and c.K == 8 and p["kchunks"] == 1 and p["last_partial"],
    KCH1_K32: lambda c, p: c.fam == "tile" and c.K == 32 and p["kchunks"] == 1 and not p["last_partial"],
    KCH1_CROSS: lambda c, p: c.fam == "tile" and p["kchunks"] == 1 and p["max_tiles"] >= 2,
    KCH2_PART: lambda c, p: c.fam == "tile" and c.K == 40 and p["kchunks"] == 2 and p["last_partial"],
    KCH3_PART: lambda c, p: c.fam == "tile" and c.K == 72 and p["kchunks"] == 3 and p["last_partial"],
    T_N40: lambda c, p: c.fam == "tile" and c.N == 40 and p["tilesN"] == 1,
    T_N136: lambda c, p: c.fam == "tile" and c.N == 136 and p["tilesN"] == 2,
    T_N264: lambda c, p: c.fam == "tile" and c.N == 264 and p["tilesN"] == 3,
    T_OUT32: lambda c, p: c.fam == "tile" and c.N % BN != 0 and not c.out16,
    T_OUT16_RES_BIAS: lambda c, p: c.fam == "tile" and c.N % BN != 0 and c.out16 and "r" in c.epi and "b" in c.epi,
    T_TRACK_TAIL: lambda c, p: c.fam == "tile" and c.N % BN != 0 and "t" in c.epi and not c.out16,
    T_G_NOT8: lambda c, p: c.fam == "tile" and p["grid"] % 8 != 0 and p["ntiles"] > 8 and not p["remap"],
    T_ABOVE_GRID_TN3: lambda c, p: (c.fam == "tile" and p["tilesN"] == 3 and 512 < p["ntiles"] <= 640 and (p["max_tiles"], p["min_tiles"]) == (2, 1)
                                    and _wg_n0_changes(c, p) and _wg_crosses_image(c, p)),
    T_TAIL_NEXT: lambda c, p: c.fam == "tile" and c.out16 and _tail_is_next(c, p),
    T_THREE: lambda c, p: c.fam == "tile" and p["ntiles"] > 1024 and p["max_tiles"] == 3,
    T_XF: lambda c, p: (c.fam == "tile" and c.a in ("xf1", "xf2") and p["last_partial"] and c.bhw[0] >= 2 and _wg_crosses_image(c, p)),
    T_UP: lambda c, p: c.fam == "tile" and c.form == "up",
    T_PHASE_TAIL: lambda c, p: c.fam == "tile" and c.form == "phase" and c.N % BN != 0,
    T_DGRAD: lambda c, p: c.fam == "tile" and c.dgrad,
    T_STATS: lambda c, p: c.fam == "tile" and "s" in c.epi and p["gstat_chunks"] > 0,
    W_NCH2: lambda c, p: c.fam == "wide" and p["kchunks"] == 2,
    W_NCH6: lambda c, p: c.fam == "wide" and p["kchunks"] == 6,
    W_N40: lambda c, p: c.fam == "wide" and c.N == 40,
    W_N136: lambda c, p: c.fam == "wide" and c.N == 136,
    W_N264: lambda c, p: c.fam == "wide" and c.N == 264,
    W_192: lambda c, p: c.fam == "wide" and p["ntiles"] == 192 == p["grid"],
    W_195: lambda c, p: c.fam == "wide" and 192 < p["ntiles"] < 256 and p["grid"] % 8 != 0,
    W_260: lambda c, p: c.fam == "wide" and 256 < p["ntiles"] <= 272 and (p["max_tiles"], p["min_tiles"]) == (2, 1),
    W_513_TN3: lambda c, p: (c.fam == "wide" and p["ntiles"] >= 513 and p["tilesN"] == 3 and p["grid"] % 3 != 0 and _wg_n0_changes(c, p)
                             and p["max_tiles"] == 3),
    W_OUT32: lambda c, p: c.fam == "wide" and not c.out16,
    W_OUT16: lambda c, p: c.fam == "wide" and c.out16,
    W_RES_K192: lambda c, p: c.fam == "wide" and "r" in c.epi and c.K > 128 and c.form == "plain",
    W_DGRAD_TAIL: lambda c, p: c.fam == "wide" and c.dgrad and c.a == "a16" and c.Ci % BN != 0,
    W_PHASE_TAIL: lambda c, p: c.fam == "wide" and c.form == "phase" and c.N % BN != 0,
    W_STATS: lambda c, p: c.fam == "wide" and "s" in c.epi and p["gstat_chunks"] > 0,
    C1_KN: lambda c, p: c.fam == "conv1" and c.K in (128, 256, 512) and c.N in (128, 512),
    C1_MIN: lambda c, p: c.fam == "conv1" and p["M"] == 32768,
    C1_PLUS32: lambda c, p: c.fam == "conv1" and p["M"] == 32768 + 32,
    C1_2_AND_3: lambda c, p: c.fam == "conv1" and p["blocks_per_wave"] == [2, 3],
}
REGIMES = tuple(HOLDS)


# ---------------------------------------------------------------------------------------------------- argument blocks
def args(c: Case, ops, ldc: int = 0):
    """the launch's block from integers alone (ops.fwd_args / dgrad_args / phase_args) with the case's storage flags; pointers are
    set by the caller.  A phase case: the block of phase (0, 0); the caller sets tapmask and the view offsets per phase."""
    B, H, W = c.bhw
    xf = {"xf1": ops.XF_AFFINE, "xf2": ops.XF_AFFINE_SILU}.get(c.a, ops.XF_NONE)
    kind = "c1" if c.fam == "conv1" else ("c3up" if c.form == "up" else "c3")
    if c.form == "phase":
        a = ops.phase_args(B, H, W, c.Co, c.Ci, c.dgrad, prec=ops.PREC_BF16)
    elif c.dgrad:
        a = ops.dgrad_args(kind, B, H, W, c.Co, c.Ci, prec=ops.PREC_BF16)
    else:
        a = ops.fwd_args(kind, B, H, W, c.Ci, c.Co, c.Ci, xf=xf, prec=ops.PREC_BF16)
    a.out_bf16 = int(c.out16)
    if c.fam == "conv1":
        a.a_bf16 = 1          # after rows_canon: the operand is a bf16 TENSOR
    if "r" in c.epi:
        a.res_bf16 = int(c.out16)
    if "s" in c.epi:
        a.gstat_groups = 32
    if ldc:
        a.ldc = ldc
    return a


def pointer_fields(c: Case):
    """the pointer fields the case's launch sets (besides A, W, C, Wh)"""
    f = ["A", "W", "C", "Wh"]
    if c.a == "a16" and c.fam != "conv1":
        f.append("A16")
    if c.a in ("xf1", "xf2"):
        f += ["scale", "shift"]
    f += [{"r": "res", "b": "bias", "s": "gstat", "t": "track"}[e] for e in c.epi]
    return f


# ---------------------------------------------------------------------------------------------------- inputs and the reference
def _gen(c: Case):
    return torch.Generator().manual_seed(zlib.crc32(c.name.encode()) & 0x7fffffff)


def out_shape(c: Case):
    B, H, W = c.bhw
    if c.form == "up" or (c.form == "phase" and not c.dgrad):
        return (B, 2 * H, 2 * W, c.N)
    return (B, H, W, c.N)


def operand_shape(c: Case):
    B, H, W = c.bhw
    if c.form == "phase" and c.dgrad:
        return (B, 2 * H, 2 * W, c.Co)   # the high-resolution gradient, read at every second pixel
    return (B, H, W, c.K)


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """NHWC CPU tensors as the launch stores them.  x: the operand (fp32, or bf16 for an image); w: logical OIHW fp32"""
    c, g = BY_NAME[name], _gen(BY_NAME[name])
    k = 1 if c.fam == "conv1" else 3
    x = 1.0 + torch.randn(operand_shape(c), generator=g)
    d = dict(x=x.bfloat16() if c.a == "a16" else x, w=torch.randn(c.Co, c.Ci, k, k, generator=g) / (k * k * c.K) ** 0.5)
    if c.a in ("xf1", "xf2"):
        d["scale"] = 1.0 + 0.3 * torch.randn(c.bhw[0], c.Ci, generator=g)
        d["shift"] = 0.2 * torch.randn(c.bhw[0], c.Ci, generator=g)
    if "b" in c.epi:
        d["bias"] = 0.5 * torch.randn(c.N, generator=g)
    if "r" in c.epi and c.form != "phase":   # (a phase dgrad's residual is the output itself: the phases add up)
        r = torch.randn(out_shape(c), generator=g)
        d["res"] = r.bfloat16() if c.out16 else r
    return d


def transform64(c: Case, inp):
    """float64 value of the fused transform on the stored fp32 x (bf16_refs.Ev._xf)"""
    y = inp["x"].double() * inp["scale"].double()[:, None, None, :] + inp["shift"].double()[:, None, None, :]
    return y * torch.sigmoid(y) if c.a == "xf2" else y


def operand_read(c: Case, inp, device_act=None) -> torch.Tensor:
    """float64 NHWC operand as the kernel multiplies it.  device_act: the device's own gn_apply_bf16 for a fused transform (its
    rounding is what the kernel reads: bf16_refs.Ev.fused_act); None = the host's r16 of the float64 transform"""
    if c.a == "a16":
        return inp["x"].double()
    if c.a == "f32":
        return r16(inp["x"]).double()
    return (device_act if device_act is not None else r16(transform64(c, inp).float())).double()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _masked(w, pa, pb):
    m = torch.zeros(3, 3, dtype=w.dtype)
    for kh in _PHASE_ROWS[pa]:
        for kw in _PHASE_ROWS[pb]:
            m[kh, kw] = 1
    return w * m


def contraction(c: Case, act: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """the bare convolution of the case in the dtype of its arguments: act NHWC (as read), w OIHW (as read) -> NHWC"""
    a = _nchw(act)
    pad = 0 if c.fam == "conv1" else 1
    if c.form == "phase":
        if not c.dgrad:
            B, _, H, W = a.shape
            y = torch.zeros(B, c.Co, 2 * H, 2 * W, dtype=a.dtype)
            for pa, pb in PHASES:
                y[:, :, pa::2, pb::2] = F.conv2d(a, _masked(w, pa, pb), None, 1, 1)
            return _nhwc(y)
        return _nhwc(sum(F.conv_transpose2d(a[:, :, pa::2, pb::2], _masked(w, pa, pb), None, 1, 1) for pa, pb in PHASES))
    if c.dgrad:
        return _nhwc(F.conv_transpose2d(a, w, None, 1, pad))
    if c.form == "up":
        a = F.interpolate(a, scale_factor=2.0, mode="nearest")
    return _nhwc(F.conv2d(a, w, None, 1, pad))


def epilogue64(c: Case, inp, y: torch.Tensor) -> torch.Tensor:
    if "bias" in inp:
        y = y + inp["bias"].to(y.dtype)
    if "res" in inp:
        y = y + inp["res"].to(y.dtype)
    return y


_REF = {}


def reference(c: Case, device_act=None) -> torch.Tensor:
    """float64 NHWC value of the launch before storage rounding; once per case (with the device's transform for xf cases)"""
    key = (c.name, device_act is not None)
    if key not in _REF:
        inp = inputs(c.name)
        _REF[key] = epilogue64(c, inp, contraction(c, operand_read(c, inp, device_act), r16(inp["w"]).double()))
    return _REF[key]


def stage(c: Case, got: torch.Tensor, v: torch.Tensor = None, name: str = "") -> Stage:
    """the criterion's stage for a stored result `got` of the case (bf16_refs.ratio)"""
    v = reference(c) if v is None else v
    return Stage(c.name + name, "dgrad" if c.dgrad else "fwd", v, got.cpu(), "bf16" if got.dtype == torch.bfloat16 else "f32", BAR_DIRECT, None)


def store(c: Case, v: torch.Tensor) -> torch.Tensor:
    """a float64 value as a correct kernel stores it"""
    return r16(v.float()) if c.out16 else v.float()
