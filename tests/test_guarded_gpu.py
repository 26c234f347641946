"""Every kernel once more, in guarded and poisoned memory (tests/guarded.py).

The value suite hands a kernel tensors that are exactly as large as they must be, lets vaehip/ops.py allocate the result with
torch.empty and compares the values inside it.  That cannot see (1) a store outside the result, (2) an element the kernel
never wrote (the caching allocator hands the previous, correct answer back to the next launch of the same shape), (3) a load
outside an operand whose value is multiplied away (finite allocator garbage times zero).  Here every case runs twice from the
same seeded CPU operands: the ordinary way (PLAIN run), and with every operand copied into pool tensors and `torch` inside
vaehip.ops swapped for the pool's proxy (GUARDED run: NaN bytes before and behind every operand, result and workspace).  Then

  (a) no guard byte of any block changed;
  (b) every operand is bytewise what it was, except the ones an op is documented to update in place (INPLACE below);
  (c) no tensor the pool handed out during the op still holds a poisoned element -- results, tensors attached to results
      (_gstat, _gnb, _b16) and workspaces alike, without exception: vaehip/ops.py asks the library before it allocates, so every
      tensor it allocates is written by a launch;
  (d) every result of the guarded run is torch.equal to the plain run's.  The plain run's values are what the parity tests
      (test_kernels_gpu.py, test_act16_gpu.py, ...) hold against their references, so no tolerance is introduced here;
  (e) both runs recorded the same kernel names: the guarded run exercised the instantiations production allocation does.

What this cannot see: a load outside an operand whose value never reaches a result.

The misaligned cases at the end (a pointer 4 bytes off 16-byte alignment: the unvectorised igemm_rows_kernel<...,false,N> /
wgrad_kernel<...,false,N> of tests/golden/dispatch_table.json) have no plain twin with the same kernel; they are held against
the CPU references of test_conv_fwd_dgrad_wgrad / test_gn_fused_conv_and_backward at those tests' bars (2e-5 / 3e-5 / 5e-5:
the unvectorised kernel is the same exact-product fp32 chain).
"""
import contextlib
import ctypes
import math
import re

import pytest
import torch
import torch.nn.functional as F

from guarded import GuardedPool, guarded
from norm_refs import SHAPES
from test_act16_gpu import FWD_CASES as ACT16_FWD_CASES
from test_dispatch_table import FAMILIES, _family
from test_kernels_gpu import (BF16_CONV_CASES, BF16_FLAT_CASES, BF16_UPCONV_PHASE_CASES, CONV_CASES, GEMM_CASES, GN_FUSED_CASES,
                              GN_RAGGED_CASES, UPCONV_PHASE_CASE, UPWINO_CASES, WIDE_CASES, WINO_CASES, WINO_WGRAD_CASES, _ref_conv,
                              _rel)

pytestmark = pytest.mark.gpu

NAN = float("nan")

# (b): operands an op updates in place, by op and operand name of the case
INPLACE = {
    "softmax_rows_": ("S",),
    "softmax_bwd_rows_": ("dP",),
    "adamw": ("p", "m", "v"),
    "sqnorm": ("out", "ws"),
    "conv_wgrad": ("gw", "gb"),          # wgrad_out / bgrad_out
    "gn_bwd": ("dgamma", "dbeta"),       # (outputs the caller allocates)
    "pack_bf16": ("dst",),
    "sumpool": ("out",),
}

SEEN = set()     # kernel families recorded over the guarded runs (test_every_kernel_family_ran_guarded)
EXTRA_FAMILIES = ["wgrad3_wino", "wgrad3_upwino", "wgrad_wino_reduce"]


def _fam(name):
    if re.match(r"(\w+?)_kernel(<.*>)?$", name):
        return _family(name)
    return re.split(r"[ <(]", name)[0].replace("_kernels", "").replace("_kernel", "")


@contextlib.contextmanager
def _mode(mode, options):
    """f32 | bf16 (bf16 arithmetic, fp32 storage: the bf16_mode fixture's setting) | bf16p (+ packed weight image) |
    act16 (bf16 storage, as tests/test_act16_gpu.py sets it up); every module-level switch is restored"""
    from vaehip import ops
    keep = (ops.PRECISION, ops.ACT_BF16, ops.WEIGHTS16, ops.PROFILER)
    with contextlib.ExitStack() as stack:
        try:
            ops.PRECISION = ops.PREC_F32 if mode == "f32" else ops.PREC_BF16
            ops.ACT_BF16 = mode == "act16" if mode != "f32" else keep[1]
            ops.WEIGHTS16 = None
            for name, value in (options or {}).items():
                stack.enter_context(ops.option(name, value))
            yield
        finally:
            ops.PRECISION, ops.ACT_BF16, ops.WEIGHTS16, ops.PROFILER = keep


def _flatten(res):
    """results, and the tensors attached to them"""
    out = []
    for r in res:
        if r is None:
            continue
        out.append(r)
        for attr, pick in (("_gstat", 0), ("_gnb", 0), ("_b16", None)):
            v = getattr(r, attr, None)
            if v is not None:
                out.append(v if pick is None else v[pick])
    return out


def _once(pool, operands, outputs, fn, mode, options, offsets, modules):
    from vaehip import ops
    dev = torch.device("cuda")
    with _mode(mode, options):
        if pool is None:
            t = {k: v.to(dev) for k, v in operands.items()}
            for k, (shape, dtype) in outputs.items():
                t[k] = torch.full(shape, NAN, dtype=dtype, device=dev)
        else:
            t = {k: pool.put(v, k, offset_bytes=offsets.get(k, 0)) for k, v in operands.items()}
            pool.snapshot()
            for k, (shape, dtype) in outputs.items():
                t[k] = pool.alloc(shape, dtype, label=k, offset_bytes=offsets.get(k, 0))
        if mode in ("bf16p", "act16") and "w" in t:  # the bf16 image of the weight, as the engine hands it over
            n = t["w"].numel()
            img = torch.empty(n, device=dev, dtype=torch.bfloat16) if pool is None else pool.alloc((n,), torch.bfloat16, label="w16")
            ops.pack_bf16(t["w"], img)
            ops.WEIGHTS16 = (t["w"].data_ptr(), n * 4, img.data_ptr())
            t["_w16"] = img
        prof = ops.PROFILER = ops.LaunchProfiler()
        if pool is None:
            res = fn(ops, t)
        else:
            with guarded(pool, ops, *modules):
                res = fn(ops, t)
        torch.cuda.synchronize()
        return t, _flatten(res), [r[0] for r in prof.records]


def _check(cid, operands, fn, *, outputs=None, mode="f32", options=None, inplace=(), offsets=None, plain=True, modules=()):
    """the plain run, the guarded run, and (a)-(e); -> (results of the guarded run, kernel names, its tensors)"""
    outputs, offsets = outputs or {}, offsets or {}
    rp = names_p = None
    if plain:
        _, rp, names_p = _once(None, operands, outputs, fn, mode, options, offsets, modules)
    pool = GuardedPool("cuda")
    tg, rg, names = _once(pool, operands, outputs, fn, mode, options, offsets, modules)
    SEEN.update(_fam(n) for n in names)
    viol = pool.violations()
    changed = pool.changed()
    unwritten = pool.unwritten_report()
    print(f"{cid} [{mode}{' ' + str(options) if options else ''}]: {len(pool.blocks)} blocks, kernels {names}; "
          f"violations {viol}; changed {changed}; unwritten {unwritten}")
    assert viol == [], (cid, viol)                                                                   # (a)
    allowed = {pool.block_of(tg[k]).label for k in inplace if k in tg}
    assert set(changed) <= allowed, (cid, changed)                                                   # (b)
    assert unwritten == [], (cid, unwritten)                                                         # (c)
    if plain:
        assert names == names_p, (cid, names, names_p)                                               # (e)
        assert len(rg) == len(rp), (cid, len(rg), len(rp))
        for i, (g, p) in enumerate(zip(rg, rp)):                                                     # (d)
            assert g.dtype == p.dtype and g.shape == p.shape, (cid, i, g.dtype, p.dtype, g.shape, p.shape)
            assert torch.equal(g, p), (cid, f"result {i} of {len(rg)}", _rel(g.float(), p.float()))
    return rg, names, tg


# ------------------------------------------------------------------------------------------------- convolutions
def _conv_operands(kind, B, H, W, Ci, Co, seed, *, res=False, gn=False, gstat=False, add=False, store16=False, dy16=False):
    from vaehip import ops
    gen = torch.Generator().manual_seed(seed)
    k = 1 if kind == "c1" else 3
    cpad = 4 if Ci == 3 else Ci
    Ho, Wo = ops.out_hw(kind, H, W)
    x = torch.zeros(B, H, W, cpad)
    x[..., :Ci] = torch.randn(B, H, W, Ci, generator=gen) * 1.3 + 0.2
    t = dict(x=x, w=torch.randn(Co, k, k, Ci, generator=gen) / math.sqrt(Ci * k * k), b=torch.randn(Co, generator=gen),
             dy=torch.randn(B, Ho, Wo, Co, generator=gen))
    if res:
        t["res"] = torch.randn(B, Ho, Wo, Co, generator=gen)
    if gn:
        t["gamma"], t["beta"] = 1 + 0.3 * torch.randn(cpad, generator=gen), 0.2 * torch.randn(cpad, generator=gen)
    if gstat:
        t["go"], t["bo"] = 1 + 0.3 * torch.randn(Co, generator=gen), 0.2 * torch.randn(Co, generator=gen)
    if add:
        t["add"] = torch.randn(B, H, W, cpad, generator=gen)
    if store16:  # bf16 storage of the wide tensors (narrow ones, statistics and parameters stay fp32)
        for name in ("x", "dy", "res", "add"):
            if name in t and t[name].shape[-1] >= 32:
                t[name] = t[name].bfloat16()
    if dy16:    # the output gradient as a bf16 tensor (what gn_bwd(want16) hands over)
        t["dy"] = t["dy"].bfloat16()
    outputs = dict(gw=((Co, k, k, Ci), torch.float32), gb=((Co,), torch.float32))
    if gn:
        outputs.update(dgamma=((cpad,), torch.float32), dbeta=((cpad,), torch.float32))
    return t, outputs


def _conv_fn(kind, H, W, Ci, Co, *, xf=0, track=False, gstat=False, gnb=False, a16=False, aux=False, bias=True,
             fwd=True, dgrad=True, wgrad=True, dgrad_kw=None, stats_x="x"):
    def fn(ops, t):
        out = []
        x, dy = t["x"], t["dy"]
        wd = t["w"].permute(0, 3, 1, 2)
        b = t["b"] if bias else None
        M = dy.shape[0] * dy.shape[1] * dy.shape[2]
        st = None
        if xf or gnb or aux:
            st = ops.gn_stats(t[stats_x], t["gamma"], t["beta"])
            out += list(st)
        if aux:  # the GroupNorm helpers on the same statistics
            out += [ops.gn_apply(x, st, ops.XF_AFFINE), ops.gn_track(x, st)]
        img = ops.gn_apply_bf16(x, st, xf) if a16 else None
        if a16:
            out.append(img)
        if fwd:
            trk = ops.conv_track_buffer(M, Co, x.device) if track else None
            y = ops.conv_fwd(x, wd, b, kind, xf=xf, stats=st if xf else None, res=t.get("res"), track=trk, a16=img,
                             gstat_groups=32 if gstat else None)
            out.append(y)
            if track:
                out += [trk, ops.track_final(trk, M)]
            if gstat:
                out += list(ops.gn_stats(y, t["go"], t["bo"]))
        if dgrad and Ci != 3:
            ctx = ops.GnCtx(x, st, t["gamma"], t["beta"], xf == ops.XF_AFFINE_SILU, 32) if gnb else None
            dA = ops.conv_dgrad(dy, wd, kind, (H, W), gnb=ctx, **(dgrad_kw or {}))
            out.append(dA)
            if gnb:
                out += [ops.gn_bwd(x, dA, st, t["gamma"], t["beta"], xf == ops.XF_AFFINE_SILU, t.get("add"), t["dgamma"], t["dbeta"]),
                        t["dgamma"], t["dbeta"]]
        if wgrad:
            ops.conv_wgrad(dy, x, kind, t["gw"].permute(0, 3, 1, 2), t["gb"] if bias else None, xf=xf, stats=st if xf else None, x16=img)
            out += [t["gw"]] + ([t["gb"]] if bias else [])
        return out
    return fn


def _conv_case(cid, kind, B, H, W, Ci, Co, *, mode="f32", options=None, seed=0, res=False, xf=0, track=False, gstat=False,
               gnb=False, a16=False, aux=False, add=False, bias=True, fwd=True, dgrad=True, wgrad=True, dgrad_kw=None, dy16=False, **kw):
    gn = bool(xf or gnb or aux)
    operands, outputs = _conv_operands(kind, B, H, W, Ci, Co, 1000 + seed + Ci + Co + H, res=res, gn=gn, gstat=gstat, add=add,
                                       store16=mode == "act16", dy16=dy16)
    if not wgrad:
        outputs.pop("gw"), outputs.pop("gb")
    elif not bias:
        outputs.pop("gb")
    if gn and not gnb:
        outputs.pop("dgamma"), outputs.pop("dbeta")
    fn = _conv_fn(kind, H, W, Ci, Co, xf=xf, track=track, gstat=gstat, gnb=gnb, a16=a16, aux=aux, bias=bias, fwd=fwd, dgrad=dgrad,
                  wgrad=wgrad, dgrad_kw=dgrad_kw)
    return _check(f"conv {cid} {kind} {B}x{H}x{W} {Ci}->{Co}", operands, fn, outputs=outputs, mode=mode, options=options,
                  inplace=INPLACE["conv_wgrad"] + INPLACE["gn_bwd"], **kw)


@pytest.mark.parametrize("kind,B,H,W,Ci,Co", CONV_CASES)
def test_guarded_conv_fp32(cuda, kind, B, H, W, Ci, Co):
    """conv_fwd / conv_dgrad / conv_wgrad with bias, every kind, at the shapes of test_conv_fwd_dgrad_wgrad"""
    _conv_case("plain", kind, B, H, W, Ci, Co, track=(Ci == 3))


@pytest.mark.parametrize("C,H,W,silu", GN_FUSED_CASES)
def test_guarded_conv_behind_groupnorm_fp32(cuda, C, H, W, silu):
    """xf AFFINE / AFFINE_SILU with stats, residual, no bias; gn_apply and gn_track; dgrad with gnb= and gn_bwd with `add`"""
    _conv_case("gn", "c3", 2, H, W, C, 128, xf=2 if silu else 1, res=True, bias=False, gnb=True, aux=True, add=True, gstat=True)


@pytest.mark.parametrize("algo", ["f4", "f2"])
@pytest.mark.parametrize("B,H,W,Ci,Co", WINO_CASES)
def test_guarded_winograd_forward_and_dgrad(cuda, B, H, W, Ci, Co, algo):
    """both Winograd kernels (library option no_wino4 for F(2x2)): plain, and fused GroupNorm+SiLU + residual + statistics
    epilogue, dgrad with the GroupNorm-backward epilogue"""
    opts = {"no_wino4": 0 if algo == "f4" else 1}
    _conv_case(algo, "c3", B, H, W, Ci, Co, options=opts, wgrad=False)
    _conv_case(algo + " gn", "c3", B, H, W, Ci, Co, options=opts, xf=2, res=True, gstat=Co % 128 == 0, gnb=True, wgrad=False)


@pytest.mark.parametrize("B,H,W,Ci,Co", WINO_WGRAD_CASES)
def test_guarded_winograd_wgrad(cuda, B, H, W, Ci, Co):
    _conv_case("wino wgrad", "c3", B, H, W, Ci, Co, fwd=False, dgrad=False)
    _conv_case("wino wgrad gn", "c3", B, H, W, Ci, Co, xf=2, fwd=False, dgrad=False)


@pytest.mark.parametrize("B,H,W,Ci,Co", UPWINO_CASES)
def test_guarded_upsampler_winograd(cuda, B, H, W, Ci, Co):
    _, names, _ = _conv_case("upwino", "c3up", B, H, W, Ci, Co)
    assert names[:2] == ["conv3_upwino_kernel<false>", "conv3_upwino_kernel<true>"], names


# the library options that move a layer to another kernel, at the shapes the existing tests use them with
OPTION_CASES = [
    ("f32", {"no_wino": 1}, "c3", 2, 8, 32, 128, 128, {}),                       # direct halo-tile kernels
    ("f32", {"no_wino": 1}, "c3", 2, 32, 32, 128, 128, dict(xf=2, res=True, gstat=True, gnb=True)),
    ("f32", {"no_wino": 1}, "c3up") + UPCONV_PHASE_CASE + ({},),                 # four phase convolutions, fp32
    ("f32", {"flat_conv": 1}, "c3", 2, 8, 32, 128, 128, dict(xf=2, res=True)),   # the flat rows kernels on a tile shape
    ("f32", {"flat_conv": 1}, "c3up", 2, 4, 16, 128, 256, {}),
    ("bf16p", {"flat_conv": 1}, "c3", 2, 8, 32, 128, 128, {}),
    ("bf16p", {"no_wide": 1}, "c3", 3, 64, 64, 256, 512, dict(wgrad=False)),     # wide-tile shape on the 128-pixel tile kernel
    ("bf16p", {"no_wide": 1}, "c3up", 7, 32, 64, 128, 256, dict(wgrad=False, bias=False)),
    ("act16", {"no_thin_mfma": 1}, "c3", 2, 16, 32, 3, 128, dict(track=True)),   # conv_in on the VALU kernels
    ("act16", {"no_thin_mfma": 1}, "c3", 2, 16, 32, 128, 3, dict(xf=2, bias=False)),
    ("act16", {"no_wgrad_dma": 1}, "c3", 2, 16, 32, 64, 128, dict(fwd=False, dgrad=False)),
    ("act16", {"no_wgrad_dma": 1}, "c3s2", 3, 16, 64, 128, 128, dict(fwd=False, dgrad=False)),
]


@pytest.mark.parametrize("mode,options,kind,B,H,W,Ci,Co,kw", OPTION_CASES)
def test_guarded_conv_under_library_options(cuda, mode, options, kind, B, H, W, Ci, Co, kw):
    _conv_case("option", kind, B, H, W, Ci, Co, mode=mode, options=options, **kw)


# (5,128,128,128,128): 640 tiles on 512 persistent workgroups, the large shape that must stay (the persistent-loop case)
assert ("c3", 5, 128, 128, 128, 128) in BF16_CONV_CASES


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kind,B,H,W,Ci,Co", BF16_CONV_CASES)
def test_guarded_bf16_conv(cuda, packed, kind, B, H, W, Ci, Co):
    """bf16 arithmetic, fp32 storage, with and without the packed weight image (test_bf16_conv_fwd_dgrad)"""
    _conv_case("bf16", kind, B, H, W, Ci, Co, mode="bf16p" if packed else "bf16", wgrad=Ci % 64 == 0)


@pytest.mark.parametrize("kind,B,H,W,Ci,Co", BF16_FLAT_CASES)
def test_guarded_bf16_flat_conv(cuda, kind, B, H, W, Ci, Co):
    _conv_case("bf16 flat", kind, B, H, W, Ci, Co, mode="bf16")


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("C,H,W,silu", [(128, 16, 16, True), (512, 4, 4, True), (512, 6, 10, False), (128, 8, 32, True)])
def test_guarded_bf16_conv_behind_groupnorm(cuda, packed, C, H, W, silu):
    """fused GroupNorm(+SiLU) in the bf16 flat and tile kernels, bf16 gradient images into gn_bwd"""
    _conv_case("bf16 gn", "c3", 2, H, W, C, 256, mode="bf16p" if packed else "bf16", xf=2 if silu else 1, res=True, bias=False,
               gnb=True, add=True, dgrad_kw=dict(out_bf16=True))


@pytest.mark.parametrize("B,C,H,W,Co", [(2, 128, 8, 32, 256), (1, 256, 4, 64, 128)])
def test_guarded_bf16_activation_image(cuda, B, C, H, W, Co):
    """gn_apply_bf16 and the forward / weight gradient reading that image (a16= / x16=); statistics epilogue"""
    _conv_case("a16", "c3", B, H, W, C, Co, mode="bf16p", xf=2, a16=True, gstat=True, dgrad=False)


@pytest.mark.parametrize("B,H,W,Ci,Co", [BF16_UPCONV_PHASE_CASES[0], BF16_UPCONV_PHASE_CASES[1]])
def test_guarded_bf16_upconv_phase(cuda, B, H, W, Ci, Co):
    _conv_case("bf16 phase", "c3up", B, H, W, Ci, Co, mode="bf16p", bias=False, gstat=True)


@pytest.mark.parametrize("B,H,W,Ci,Co", [WIDE_CASES[0], WIDE_CASES[1]])
def test_guarded_bf16_wide_tile(cuda, B, H, W, Ci, Co):
    """the persistent wide-tile kernel: (5,128,128,128,128) runs a second tile on some workgroups"""
    _, names, _ = _conv_case("wide", "c3", B, H, W, Ci, Co, mode="bf16p", xf=2, a16=True, res=Ci > 128, gstat=True, dy16=True,
                             dgrad_kw=dict(out_bf16=True))
    # (the dgrad's channel tiles are over Ci: it needs its own >= 192 tiles to run on the wide kernel, as test_bf16_wide_tile_kernel says)
    dg = "conv3_wide_bf16_kernel<true,3>" if B * (H // 8) * (W // 32) * ((Ci + 127) // 128) >= 192 else "conv3_tile_bf16_kernel<true,false,0,true>"
    assert names[:2] == ["conv3_wide_bf16_kernel<false,3>", dg], names


@pytest.mark.parametrize("kind,B,H,W,Ci,Co,family", [c for c in ACT16_FWD_CASES if c[1:4] != (7, 40, 96)])
def test_guarded_conv_bf16_storage(cuda, kind, B, H, W, Ci, Co, family):
    """ops.ACT_BF16: bf16 tensors in and out, bf16 residual, statistics epilogue (test_conv_forward_and_dgrad_with_bf16_storage)"""
    _, names, _ = _conv_case("act16", kind, B, H, W, Ci, Co, mode="act16", res=True, gstat=True)
    assert names[0].startswith(family), names


ACT16_EXTRA = [
    ("c1", 2, 128, 128, 256, 128, dict(wgrad=False)),                  # conv1_bf16: streaming 1x1 with resident weights
    ("c3", 2, 16, 32, 3, 128, dict(track=True)),                        # conv_in: conv_thin_bf16 / wgrad_thin_bf16
    ("c3", 2, 16, 32, 128, 3, dict(xf=2, bias=False)),                  # conv_out: conv_thinn_bf16, thin dgrad and wgrad
    ("c3", 2, 16, 32, 128, 3, dict(xf=2)),
    ("c3", 2, 8, 8, 4, 512, {}),                                        # decoder.conv_in
    ("c3", 3, 8, 16, 4, 512, dict(fwd=False, dgrad=False)),             # its wgrad on whole 128-pixel tiles
    ("c3", 2, 16, 32, 64, 128, dict(fwd=False, dgrad=False)),           # wgrad3_dma_bf16
    ("c3", 1, 64, 64, 256, 136, dict(fwd=False, dgrad=False)),          #   a co tail: channels beyond M are never fetched
    ("c3", 5, 6, 96, 192, 128, dict(fwd=False, dgrad=False)),
    ("c3up", 2, 8, 32, 128, 128, dict(bias=True)),                      #   the four phase launches
    ("c3up", 13, 32, 64, 128, 256, dict(bias=False, wgrad=False)),      # >= 192 tiles: the phases on conv3_wide_bf16<*,2>
    ("c3s2", 3, 16, 64, 128, 128, dict(fwd=False, dgrad=False)),
    ("c3s2", 5, 6, 64, 64, 128, dict(fwd=False, dgrad=False)),
    ("c3", 2, 8, 32, 128, 256, dict(xf=2, res=True, gnb=True, add=True, bias=False)),
    ("c3", 2, 5, 7, 256, 128, dict(xf=1, res=True, gnb=True, add=True)),
]


@pytest.mark.parametrize("kind,B,H,W,Ci,Co,kw", ACT16_EXTRA)
def test_guarded_bf16_storage_special_kernels(cuda, kind, B, H, W, Ci, Co, kw):
    _conv_case("act16x", kind, B, H, W, Ci, Co, mode="act16", **kw)


def test_guarded_bf16_gradient_images(cuda):
    """gn_bwd(want16) leaves a bf16 image on its fp32 result; the dgrad and wgrad of the layer below read it (A16 / dY16)"""
    B, H, W, Cc = 2, 8, 32, 128
    gen = torch.Generator().manual_seed(61)
    operands = dict(x=torch.randn(B, H, W, Cc, generator=gen) + 0.3, g=torch.randn(B, H, W, Cc, generator=gen),
                    gamma=1 + 0.3 * torch.randn(Cc, generator=gen), beta=0.2 * torch.randn(Cc, generator=gen),
                    xin=torch.randn(B, H, W, Cc, generator=gen), w=torch.randn(Cc, 3, 3, Cc, generator=gen) / math.sqrt(9 * Cc))
    outputs = dict(dgamma=((Cc,), torch.float32), dbeta=((Cc,), torch.float32), gw=((Cc, 3, 3, Cc), torch.float32),
                   gb=((Cc,), torch.float32))

    def fn(ops, t):
        wd = t["w"].permute(0, 3, 1, 2)
        st = ops.gn_stats(t["x"], t["gamma"], t["beta"])
        dx = ops.gn_bwd(t["x"], t["g"], st, t["gamma"], t["beta"], True, None, t["dgamma"], t["dbeta"], want32=True, want16=True)
        assert getattr(dx, "_b16", None) is not None
        d16 = ops.gn_bwd(t["x"], t["g"], st, t["gamma"], t["beta"], True, None, t["dgamma"], t["dbeta"], want32=False, want16=True)
        dA = ops.conv_dgrad(dx, wd, "c3", (H, W), out_bf16=True)
        dB = ops.conv_dgrad(d16, wd, "c3", (H, W))
        ops.conv_wgrad(dx, t["xin"], "c3", t["gw"].permute(0, 3, 1, 2), t["gb"])
        return [dx, d16, dA, dB, t["gw"], t["gb"], t["dgamma"], t["dbeta"]]

    _check("bf16 gradient images", operands, fn, outputs=outputs, mode="bf16p", inplace=INPLACE["conv_wgrad"] + INPLACE["gn_bwd"])


# ------------------------------------------------------------------------------------------------- GroupNorm, moments
# (the small edge shapes of tests/norm_refs.py: fewer pixels than pixel rows, the clamped backward tail, an empty last chunk, B >= 64)
GN_EDGE_CASES = [SHAPES[k] for k in ("one_pixel", "seven_pixels", "tail_c256", "tail_c512", "last_empty", "b65")]


@pytest.mark.parametrize("store16", [False, True])
@pytest.mark.parametrize("B,C,H,W", GN_RAGGED_CASES[:2] + [(2, 128, 16, 16), (1, 512, 6, 10)] + GN_EDGE_CASES)
def test_guarded_groupnorm(cuda, B, C, H, W, store16):
    """gn_stats (ragged chunk plans: trailing chunks start beyond H*W), gn_apply, gn_apply_bf16, gn_track, gn_bwd with and
    without `add`, fp32 and bf16 storage"""
    gen = torch.Generator().manual_seed(5 + H)
    operands = dict(x=torch.randn(B, H, W, C, generator=gen) * 0.5 + 1.0, g=torch.randn(B, H, W, C, generator=gen),
                    add=torch.randn(B, H, W, C, generator=gen), gamma=1 + 0.2 * torch.randn(C, generator=gen),
                    beta=0.1 * torch.randn(C, generator=gen))
    if store16:
        operands.update({k: operands[k].bfloat16() for k in ("x", "g", "add")})
    outputs = {k: ((C,), torch.float32) for k in ("dgamma", "dbeta", "dgamma2", "dbeta2")}

    def fn(ops, t):
        st = ops.gn_stats(t["x"], t["gamma"], t["beta"])
        out = list(st) + [ops.gn_apply(t["x"], st, ops.XF_AFFINE_SILU), ops.gn_apply_bf16(t["x"], st, ops.XF_AFFINE), ops.gn_track(t["x"], st)]
        out.append(ops.gn_bwd(t["x"], t["g"], st, t["gamma"], t["beta"], True, None, t["dgamma"], t["dbeta"]))
        out.append(ops.gn_bwd(t["x"], t["g"], st, t["gamma"], t["beta"], False, t["add"], t["dgamma2"], t["dbeta2"], want32=not store16,
                              want16=store16))
        return out + [t[k] for k in outputs]

    _check(f"groupnorm {B}x{H}x{W}x{C} {'bf16' if store16 else 'fp32'}", operands, fn, outputs=outputs,
           inplace=tuple(outputs))


@pytest.mark.parametrize("Cc", [1, 3, 257, 128])
def test_guarded_moments(cuda, Cc):
    """moments over 1 / 3 / 257 channels, the 3-of-4 channel view of a padded image, behind a GroupNorm transform, on bf16"""
    B, H, W = 2, 12, 20
    gen = torch.Generator().manual_seed(70 + Cc)
    operands = dict(x=torch.randn(B, H, W, Cc, generator=gen) + 0.4, x4=torch.randn(B, H, W, 4, generator=gen))
    if Cc % 32 == 0:
        operands.update(gamma=1 + 0.2 * torch.randn(Cc, generator=gen), beta=0.1 * torch.randn(Cc, generator=gen))

    def fn(ops, t):
        out = [ops.moments(t["x"]), ops.moments(t["x4"][..., :3]), ops.map_snapshot(t["x"])]
        if "gamma" in t:
            st = ops.gn_stats(t["x"], t["gamma"], t["beta"])
            x16 = ops.to_bf16(t["x"])
            out += [ops.moments(t["x"], st, ops.XF_AFFINE_SILU), x16, ops.moments(x16, st, ops.XF_AFFINE), ops.map_snapshot(x16)]
        return out

    _check(f"moments C={Cc}", operands, fn)


def test_guarded_conv_track_buffer_and_final(cuda):
    """conv_track_buffer + track_final around a tracked conv_in and a tracked wide layer (M = 512 and a ragged M)"""
    for B, H, W, Ci, Co in [(2, 16, 16, 3, 128), (2, 5, 7, 128, 128), (2, 8, 32, 128, 128)]:
        _conv_case("track", "c3", B, H, W, Ci, Co, track=True, dgrad=False, wgrad=False)


# ------------------------------------------------------------------------------------------------- gemm, attention, softmax
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("z,M,N,K", [c for c in GEMM_CASES if c in [(3, 100, 36, 40), (2, 64, 64, 512)]])
def test_guarded_batched_gemms(cuda, mode, z, M, N, K):
    gen = torch.Generator().manual_seed(z * 100 + M)
    operands = dict(A=torch.randn(z, M, K, generator=gen), Bt=torch.randn(z, N, K, generator=gen), Bn=torch.randn(z, K, N, generator=gen),
                    At=torch.randn(z, K, M, generator=gen))
    _check(f"gemm {z}x{M}x{N}x{K}", operands,
           lambda ops, t: [ops.gemm_nt(t["A"], t["Bt"], 0.5), ops.gemm_nn(t["A"], t["Bn"]), ops.gemm_tn(t["At"], t["Bn"], 2.0)], mode=mode)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,T", [(3, 64), (2, 1024)])
def test_guarded_attention(cuda, mode, B, T):
    Cc = 512
    gen = torch.Generator().manual_seed(T)
    operands = {k: torch.randn(B, T, Cc, generator=gen) * s for k, s in (("q", 2.0), ("k", 2.0), ("v", 1.0), ("do", 1.0))}

    def fn(ops, t):
        o, saved = ops.attn_fwd(t["q"], t["k"], t["v"], Cc ** -0.5)
        dq, dk, dv = ops.attn_bwd(saved, o, t["do"], Cc ** -0.5)
        return [o, saved[3], dq, dk, dv]

    _check(f"attention {B}x{T}", operands, fn, mode=mode)


def test_guarded_softmax(cuda):
    gen = torch.Generator().manual_seed(3)
    operands = dict(S=torch.randn(2, 70, 300, generator=gen) * 3, dP=torch.randn(2, 70, 300, generator=gen))

    def fn(ops, t):
        P = ops.softmax_rows_(t["S"])
        return [P, ops.softmax_bwd_rows_(P, t["dP"])]

    _check("softmax (2,70,300)", operands, fn, inplace=INPLACE["softmax_rows_"] + INPLACE["softmax_bwd_rows_"])


# ------------------------------------------------------------------------------------------------- loss, layout, optimizer
def test_guarded_layout_and_pool(cuda):
    gen = torch.Generator().manual_seed(2)
    operands = dict(x=torch.randn(2, 3, 6, 10, generator=gen), s=torch.randn(2, 8, 12, 128, generator=gen),
                    n=torch.randn(3, 5, 7, 8, generator=gen))

    def fn(ops, t):
        y = ops.nchw_to_nhwc(t["x"], 4)
        ops.lib.call("vae_sumpool2x2", ops._p(t["s"]), 2, 4, 6, 128, ops._p(t["out"]), ops._stream())
        return [y, ops.nhwc_to_nchw(ops.nchw_to_nhwc(t["x"])), ops.nhwc_to_nchw(t["n"]), t["out"]]

    _check("layout + sumpool", operands, fn, outputs=dict(out=((2, 4, 6, 128), torch.float32)), inplace=INPLACE["sumpool"])


def test_guarded_sample_kl_mse(cuda):
    gen = torch.Generator().manual_seed(11)
    B, h, w, L, R = 3, 4, 4, 4, 32
    mom = torch.randn(B, h, w, 2 * L, generator=gen) * 2
    mom[0, 0, 0, L], mom[1, 1, 1, L + 1] = 25.0, -40.0
    operands = dict(mom=mom, eps=torch.randn(B, h, w, L, generator=gen), dz=torch.randn(B, h, w, L, generator=gen),
                    target=torch.rand(B, R, R, 3, generator=gen) * 2 - 1, recon=torch.randn(B, R, R, 3, generator=gen),
                    big=torch.randn(2, 160, 161, 3, generator=gen))

    def fn(ops, t):
        z, klp = ops.sample_kl(t["mom"], t["eps"])
        z0, klp0 = ops.sample_kl(t["mom"], None)
        return [z, klp, z0, klp0, ops.mse_kl_loss(t["recon"], t["target"], klp, 1e-3), ops.mse_bwd(t["recon"], t["target"]),
                ops.mse_kl_loss(t["big"], t["big"] * 0.5, klp, 1e-3), ops.mse_bwd(t["big"], t["big"] * 0.5, 0.25),
                ops.sample_kl_bwd(t["mom"], t["eps"], t["dz"], 1e-3)]

    _check("sample_kl / mse", operands, fn)


def test_guarded_elementwise_and_packing(cuda):
    gen = torch.Generator().manual_seed(13)
    n = 100003
    n16 = 100004  # (vae_add_bf16 takes multiples of 4)
    operands = dict(a=torch.randn(n, generator=gen), b=torch.randn(n, generator=gen), a16=torch.randn(n16, generator=gen).bfloat16(),
                    b16=torch.randn(n16, generator=gen), w=torch.randn(160, 3, 3, 96, generator=gen))

    def fn(ops, t):
        ops.pack_bf16(t["a"], t["dst"])
        return [ops.add(t["a"], t["b"]), ops.add(t["a16"], t["b16"]), ops.add(t["a16"], t["a16"]), t["dst"], ops.to_f32(t["a16"]),
                ops.to_bf16(t["b16"]), ops.upconv_phase_weights(t["w"])]

    _check("add / pack / phase weights", operands, fn, outputs=dict(dst=((n,), torch.bfloat16)), inplace=INPLACE["pack_bf16"])


def test_guarded_sqnorm_adamw(cuda):
    """n = 100003: no multiple of any vector width or block size"""
    gen = torch.Generator().manual_seed(21)
    n = 100003
    operands = dict(p=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen) * 3, m=torch.randn(n, generator=gen) * 0.1,
                    v=torch.rand(n, generator=gen) * 0.01, out=torch.zeros(1))

    def fn(ops, t):
        ops.sqnorm(t["g"], t["out"])
        ops.sqnorm(t["g"], t["out2"], t["ws"])
        ops.adamw(t["p"], t["g"], t["m"], t["v"], t["out"], 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 2)
        return [t["out"], t["out2"], t["p"], t["m"], t["v"]]

    _check("sqnorm + adamw", operands, fn, outputs=dict(out2=((1,), torch.float32), ws=((2048,), torch.float32)),
           inplace=INPLACE["adamw"] + INPLACE["sqnorm"] + ("out2",))


def test_guarded_preprocess(cuda):
    """the GPU input transform: uint8 in, odd sizes, grey and RGB.  Pixel values stay below 255 so that no legitimately written
    byte of the uint8 intermediate equals the poison pattern."""
    import numpy as np
    from vaehip import preprocess
    rng = np.random.RandomState(5)
    images = [rng.randint(0, 255, size=(37, 53, 3)).astype(np.uint8), rng.randint(0, 255, size=(37, 53, 3)).astype(np.uint8),
              rng.randint(0, 255, size=(71, 45)).astype(np.uint8), rng.randint(0, 255, size=(33, 33, 3)).astype(np.uint8)]

    def fn(ops, t):
        return [preprocess.GpuPreprocessor(32, "cuda")(images)]

    _check("preprocess", {}, fn, modules=(preprocess,))


# ------------------------------------------------------------------------------------------------- the engine step
def _gap_mask(arena):
    gap = torch.ones(arena.total, dtype=torch.bool)
    for _name, _p, off, n in arena.entries:
        gap[off:off + n] = False
    return gap.cuda()


@pytest.mark.parametrize("mode,ckpt", [("no", False), ("bf16", False), ("bf16", True)])
def test_guarded_engine_step(cuda, mode, ckpt):
    """one forward_backward in guarded memory with every parameter segment of arena.grad pre-filled with NaN: every gradient
    element is written (not accumulated onto), the alignment gaps stay exactly 0.0; then one HipTrainer.train_step: the gaps of
    arena.flat and of AdamW's exp_avg / exp_avg_sq stay exactly 0.0 (ParamArena's docstring; the fused clip + AdamW and the
    all-reduce run over the flat buffers relying on it)"""
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip import engine, ops, optim, trainer
    from vaehip.trainer import HipTrainer
    R, B, klw = 64, 2, 1e-4
    w = SDXLVAEWrapper("synthetic:1")
    w.to(cuda)
    arena, eng = w.vae.arena, w.vae.engine
    gap = _gap_mask(arena)
    assert int(gap.sum()) > 0 and float(arena.flat[gap].abs().max()) == 0.0
    x, eps = vo.synthetic_pixels(B, R, 42, 5).cuda(), vo.synthetic_eps(B, R, 42, 5).cuda()
    keep = (ops.PRECISION, ops.ACT_BF16, ops.WEIGHTS16, ops.PROFILER)
    try:
        eng.set_precision(mode)
        eng.checkpoint_decoder = ckpt
        res = eng.forward_backward(x, eps, klw)
        scalars, recon, grad = res["scalars"].clone(), res["reconstruction"].clone(), arena.grad.clone()
        assert bool(torch.isfinite(grad).all()) and float(grad[gap].abs().max()) == 0.0
        arena.grad.masked_fill_(~gap, NAN)
        pool = GuardedPool(cuda)
        xg, eg = pool.put(x, "pixel_values"), pool.put(eps, "eps")
        pool.snapshot()
        prof = ops.PROFILER = ops.LaunchProfiler()
        with guarded(pool, ops, engine, trainer, optim):
            res2 = eng.forward_backward(xg, eg, klw)
            torch.cuda.synchronize()
            names = [r[0] for r in prof.records]
            ops.PROFILER = None
            SEEN.update(_fam(n) for n in names)
            viol, changed = pool.violations(), pool.changed()
            unwritten = pool.unwritten_report()
            print(f"engine {mode} ckpt={ckpt}: {len(pool.blocks)} blocks, {len(names)} launches; violations {viol}; changed {changed}; "
                  f"unwritten {unwritten}")
            assert viol == [] and changed == [] and unwritten == [], (viol, changed, unwritten)
            assert torch.equal(res2["scalars"], scalars) and torch.equal(res2["reconstruction"], recon)
            bad = (arena.grad != grad) | torch.isnan(arena.grad)
            assert not bool(bad.any()), (int(bad.sum()), [n for n, _p, o, k in arena.entries if bool(bad[o:o + k].any())][:8])
            assert float(arena.grad[gap].abs().max()) == 0.0
            # one optimizer step on top, its state allocated from the pool
            tr = HipTrainer(w, lr=1e-3, kl_weight=klw, lr_warmup_steps=1, max_train_steps=10, mixed_precision=mode, checkpoint_decoder=ckpt)
            tr.train_step(xg, eg)
            tr.train_step(xg, eg)  # (the first step of the warm-up has lr = 0)
            torch.cuda.synchronize()
            opt = tr.optimizer
            assert any(b.tensor.data_ptr() == opt.exp_avg.data_ptr() for b in pool.blocks), "AdamW state is not guarded"
            viol = pool.violations()
            unwritten = pool.unwritten_report()
            print(f"engine {mode} ckpt={ckpt} + 2 train steps: {len(pool.blocks)} blocks; violations {viol}; unwritten {unwritten}")
            assert viol == [] and unwritten == [], (viol, unwritten)
            for name, buf in (("arena.flat", arena.flat), ("arena.grad", arena.grad), ("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq)):
                assert buf.shape == gap.shape and float(buf[gap].abs().max()) == 0.0, name
                assert bool(torch.isfinite(buf).all()), name
            assert float(opt.exp_avg.abs().max()) > 0.0  # the step did run
    finally:
        eng.set_precision("no")
        eng.checkpoint_decoder = False
        ops.PRECISION, ops.ACT_BF16, ops.WEIGHTS16, ops.PROFILER = keep


# ------------------------------------------------------------------------------------------------- misaligned operands
MISALIGNED_CASES = [("c3", 2, 12, 12, 128, 128), ("c1", 2, 8, 8, 256, 128), ("c3", 2, 16, 16, 128, 3), ("c3s2", 1, 10, 14, 128, 128),
                    ("c3up", 1, 5, 6, 256, 256)]
_UNVEC_ROWS = re.compile(r"igemm_rows_kernel<\d+,\d+,\d+,\d+,(true|false),false,[012]>$")
_UNVEC_WGRAD = re.compile(r"wgrad_kernel<\d+,\d+,\d+,\d+,false,[012]>$")


def _expect_unvectorised(names, Ci, Co, rx):
    """the unvectorised instantiation; a <= 4-channel side keeps its (scalar) VALU kernel whatever the alignment, as the
    `misaligned` rows of tests/golden/dispatch_table.json say (c3:128>3 -> conv_smallk / conv_smalln / wgrad_smallk)"""
    for n in names:
        if min(Ci, Co) <= 4 and re.match(r"(conv|wgrad)_small[kn]_kernel", n):
            continue
        assert rx.match(n), (n, names)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("which", ["activation", "weight"])
@pytest.mark.parametrize("xf", [0, 1, 2])
@pytest.mark.parametrize("kind,B,H,W,Ci,Co", MISALIGNED_CASES)
def test_misaligned_forward(cuda, kind, B, H, W, Ci, Co, xf, which, mode):
    operands, _ = _conv_operands(kind, B, H, W, Ci, Co, 1234 + Ci + Co + H, gn=bool(xf))
    from vaehip import ops
    from vaehip.lib import VaeHipError, lib
    x, w, b = operands["x"], operands["w"], operands["b"]
    operands["x_al"] = x.clone()  # vae_gn_stats_partial takes 16-byte aligned tensors only: the statistics come from an aligned copy
    fn = _conv_fn(kind, H, W, Ci, Co, xf=xf, dgrad=False, wgrad=False, stats_x="x_al")
    cid = f"misaligned fwd {which} xf={xf} {kind} {B}x{H}x{W} {Ci}->{Co}"
    offsets = {"x" if which == "activation" else "w": 4}
    geom = ops._fwd_geom(kind, B, H, W, x.shape[-1])
    if which == "activation" and xf and not lib.query("vae_xf_fusable_rows", ctypes.byref(geom), B * geom.Ho * geom.Wo, Ci):
        # a transform that cannot be fused at this size goes through vae_gn_apply first, which refuses the misaligned tensor
        # loudly: there is no launch of a conv kernel on it to compare
        with pytest.raises(VaeHipError, match="gn_apply: unaligned"):
            _check(cid, operands, fn, mode=mode, offsets=offsets, plain=False)
        return
    res, names, _ = _check(cid, operands, fn, mode=mode, offsets=offsets, plain=False)
    y = res[-1]
    if which == "activation":
        _expect_unvectorised(names, Ci, Co, _UNVEC_ROWS)
    r16 = (lambda t: t.bfloat16().float()) if any("bf16" in n for n in names) else (lambda t: t)
    xn = x.permute(0, 3, 1, 2)
    if xf:
        xn = F.group_norm(xn, 32, operands["gamma"], operands["beta"], 1e-6)
        xn = F.silu(xn) if xf == 2 else xn
    ref = _ref_conv(r16(xn), r16(w.permute(0, 3, 1, 2)), b, kind)
    err = _rel(y.permute(0, 3, 1, 2), ref)
    bar = (3e-5 if xf else 2e-5) if r16(x) is x else 5e-4  # (bf16 kernels behind a transform: test_bf16_flat_fused_gn's bar)
    print(f"  forward error {err:.2e} (bar {bar:.0e}) {names}")
    assert err < bar, (err, names)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("which", ["activation", "weight"])
@pytest.mark.parametrize("kind,B,H,W,Ci,Co", MISALIGNED_CASES)
def test_misaligned_dgrad(cuda, kind, B, H, W, Ci, Co, which, mode):
    operands, _ = _conv_operands(kind, B, H, W, Ci, Co, 1234 + Ci + Co + H)
    fn = _conv_fn(kind, H, W, Ci, Co, fwd=False, wgrad=False)
    res, names, _ = _check(f"misaligned dgrad {which} {kind} {B}x{H}x{W} {Ci}->{Co}", operands, fn, mode=mode,
                           offsets={"dy" if which == "activation" else "w": 4}, plain=False)
    if which == "activation" and not (kind == "c3up" and len(names) > 1):
        _expect_unvectorised(names, Ci, Co, _UNVEC_ROWS)
    r16 = (lambda t: t.bfloat16().float()) if any("bf16" in n for n in names) else (lambda t: t)
    xr = operands["x"].permute(0, 3, 1, 2).clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(_ref_conv(xr, r16(operands["w"].permute(0, 3, 1, 2)), None, kind), xr, r16(operands["dy"].permute(0, 3, 1, 2)))
    err = _rel(res[0].permute(0, 3, 1, 2), gx)
    print(f"  dgrad error {err:.2e} {names}")
    assert err < 2e-5, (err, names)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("which", ["dy"])
@pytest.mark.parametrize("xf", [0, 2])
@pytest.mark.parametrize("kind,B,H,W,Ci,Co", MISALIGNED_CASES)
def test_misaligned_wgrad(cuda, kind, B, H, W, Ci, Co, xf, which, mode):
    operands, outputs = _conv_operands(kind, B, H, W, Ci, Co, 1234 + Ci + Co + H, gn=bool(xf))
    outputs = {k: outputs[k] for k in ("gw", "gb")}
    fn = _conv_fn(kind, H, W, Ci, Co, xf=xf, fwd=False, dgrad=False)
    res, names, _ = _check(f"misaligned wgrad {which} xf={xf} {kind} {B}x{H}x{W} {Ci}->{Co}", operands, fn, outputs=outputs, mode=mode,
                           offsets={which: 4}, plain=False, inplace=INPLACE["conv_wgrad"])
    wnames = [n for n in names if n.startswith("wgrad")]
    if which == "dy" and not (kind == "c3up" and len(wnames) > 1):
        _expect_unvectorised(wnames, Ci, Co, _UNVEC_WGRAD)
    r16 = (lambda t: t.bfloat16().float()) if any("bf16" in n for n in wnames) else (lambda t: t)
    xn = operands["x"].permute(0, 3, 1, 2)
    if xf:
        xn = F.silu(F.group_norm(xn, 32, operands["gamma"], operands["beta"], 1e-6))
    wr = operands["w"].permute(0, 3, 1, 2).clone().requires_grad_(True)
    dy = operands["dy"].permute(0, 3, 1, 2)
    _ref_conv(r16(xn), wr, None, kind).backward(r16(dy))
    gw, gb = res[-2], res[-1]
    err_w, err_b = _rel(gw.permute(0, 3, 1, 2), wr.grad), _rel(gb, dy.sum(dim=(0, 2, 3)))
    bar = (5e-5 if xf else 3e-5) if r16(dy) is dy else 5e-4
    print(f"  wgrad error {err_w:.2e} (bar {bar:.0e}) bias {err_b:.2e} {names}")
    assert err_w < bar and err_b < 3e-5, (err_w, err_b, names)


# ------------------------------------------------------------------------------------------------- coverage (last)
def test_every_kernel_family_ran_guarded(cuda):
    """the union of kernel names recorded over the guarded runs of this module contains every family the dispatcher knows"""
    missing = [f for f in FAMILIES + EXTRA_FAMILIES if f not in SEEN]
    assert not missing, (missing, sorted(SEEN))
