"""Kernel-selection table of libvaehip: what every pure dispatch query answers over a grid of argument blocks.

The argument blocks are the ones vaehip.ops launches: every case is built by the launch descriptions of ops.py (fwd_args,
dgrad_args, ..., gemm_tn_args); only the fake pointers and the per-variant fields are added here.  For each convolution
launch it records the kernel name, the fused-epilogue chunk counts and the capability answers; for each weight gradient
the kernel name, the split plan and the capability answers; for each forward geometry the two bf16 image checks.  The pointers are fake (16-byte-aligned integers): no query dereferences them and none touches the HIP runtime,
so the table is built on any host.  Nothing here calls a launching entry point (vae_igemm_rows, vae_wgrad,
vae_wino_weights, vae_wgrad_wino): with fake pointers a launch would fault a real device.

    python tests/golden/make_dispatch_table.py [OUT]     (default: tests/golden/dispatch_table.json)

tests/test_dispatch_table.py rebuilds the same table and compares it with the committed one."""
import ctypes as C
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(ROOT, "vae-channel-dynamics_amd", "src")
if SRC not in sys.path:
    sys.path.insert(0, SRC)

from vaehip import ops  # noqa: E402
from vaehip.lib import lib  # noqa: E402

F32, BF16 = ops.PREC_F32, ops.PREC_BF16
OPTIONS = ("flat_conv", "no_wino", "no_wino4", "no_wide", "no_thin_mfma", "no_wgrad_dma")

# the SDXL-VAE's convolutions: (kind, Cin, Cout, divisor of the image size giving the layer's input map)
LAYERS = [
    ("c3", 3, 128, 1), ("c3", 128, 128, 1), ("c3", 128, 256, 2), ("c3", 256, 256, 2), ("c3", 256, 512, 4),
    ("c3", 512, 512, 4), ("c3", 512, 512, 8), ("c3", 512, 8, 8), ("c3", 4, 512, 8), ("c3", 512, 256, 2),
    ("c3", 256, 128, 1), ("c3", 128, 3, 1),
    ("c1", 128, 256, 2), ("c1", 256, 512, 4), ("c1", 8, 8, 8), ("c1", 4, 4, 8), ("c1", 512, 256, 2), ("c1", 256, 128, 1),
    ("c3s2", 128, 128, 1), ("c3s2", 256, 256, 2), ("c3s2", 512, 512, 4),
    ("c3up", 512, 512, 8), ("c3up", 512, 512, 4), ("c3up", 256, 256, 2),
]
SIZES = (32, 40, 48, 64, 128, 256, 512, 1024)
BATCHES = (1, 2, 16, 32)

_next = [0x10000000]


def ptr(misaligned=False):
    """a fresh fake device address, 16-byte aligned (or 4 bytes off)"""
    _next[0] += 0x100000
    return _next[0] + (4 if misaligned else 0)


P, MIS = "ptr", "misaligned"  # in a variant: a fresh fake pointer, a fresh one 4 bytes off 16-byte alignment


def _copy(a, **fields):
    b = type(a)()
    C.pointer(b)[0] = a
    for k, v in fields.items():
        setattr(b, k, ptr(v == MIS) if v in (P, MIS) else v)
    return b


# --------------------------------------------------------------------------- convolution (vae_igemm_args) cases
def conv_ptrs(a):
    """the block of a convolution launch with its operands (and the transform's scale / shift) in place"""
    return _copy(a, A=P, W=P, C=P, **(dict(scale=P, shift=P) if a.xf else {}))


def conv_variants(a, dgrad):
    """(tag, argument block) variants of one convolution launch"""
    bf16, xf = a.prec == BF16, a.xf
    gnb = dict(gnb_x=P, gnb_mean=P, gnb_rstd=P, gnb_gamma=P, gnb_beta=P, gnb_ws=P, gnb_groups=32, gnb_silu=1)
    v = [("", {})]
    if bf16:
        v += [("Wh", dict(Wh=P))]
        v += [("Wh,A16", dict(Wh=P, A16=P)), ("Wh,A16,out16", dict(Wh=P, A16=P, out_bf16=1))] if xf == 0 else [("Wh,a16", dict(Wh=P, a_bf16=1))]
        v += [("Wh,out16", dict(Wh=P, out_bf16=1)), ("Wh,out16,res16", dict(Wh=P, out_bf16=1, res=P, res_bf16=1)),
              ("Wh,res16", dict(Wh=P, res=P, res_bf16=1))]
    else:
        v += [("Wu", dict(Wu=P)), ("out16", dict(out_bf16=1))]
    if not dgrad:
        v += [("res,track", dict(res=P, track=P)), ("gstat", dict(gstat=P, gstat_groups=32, **(dict(Wh=P) if bf16 else {})))]
        v += [] if bf16 else [("gstat,Wu", dict(gstat=P, gstat_groups=32, Wu=P))]
    else:
        v += [("gnb", dict(gnb, **(dict(Wh=P) if bf16 else dict(Wu=P))))]
    v += [("misaligned", dict(A=MIS))]
    return [(tag, _copy(a, **kw)) for tag, kw in v]


def conv_result(dll, a):
    buf = C.create_string_buffer(256)
    rc = dll.vae_igemm_kernel_name(C.byref(a), buf, 256)
    return [buf.value.decode() if rc == 0 else f"rc={rc}",
            dll.vae_conv_gstat_chunks(C.byref(a)), dll.vae_conv_gnb_chunks(C.byref(a)), dll.vae_conv_phase_ok(C.byref(a)),
            dll.vae_conv_io16_ok(C.byref(a)), dll.vae_wino_ok(C.byref(a)), dll.vae_wino_weight_floats(C.byref(a)),
            dll.vae_xf_fusable_rows(C.byref(a.g), a.M, a.K)]


# --------------------------------------------------------------------------- weight-gradient (vae_wgrad_args) cases
def wgrad_ptrs(a):
    return _copy(a, dY=P, X=P, **(dict(scale=P, shift=P) if a.xf else {}))


def wgrad_variants(a):
    v = [("", {})]
    if a.prec == BF16:
        v += [("X16", dict(X16=P)), ("X16,dY16", dict(X16=P, dY16=P))] if a.xf == 0 else [("x16", dict(x_bf16=1))]
        v += [("dY16", dict(dY16=P)), ("dY16only", dict(dY=None, dY16=P)), ("y16", dict(y_bf16=1))]
    else:
        v += [("x16,y16", dict(x_bf16=1, y_bf16=1))]
    v += [("misaligned", dict(dY=MIS))]
    return [(tag, _copy(a, **kw)) for tag, kw in v]


def wgrad_result(dll, a):
    buf = C.create_string_buffer(256)
    rc = dll.vae_wgrad_kernel_name(C.byref(a), buf, 256)
    ns, fus, wns = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    prc = dll.vae_wgrad_plan(C.byref(a), C.byref(ns), C.byref(fus))
    wrc = dll.vae_wgrad_wino_plan(C.byref(a), C.byref(wns))
    return [buf.value.decode() if rc == 0 else f"rc={rc}", [prc, ns.value, fus.value],
            dll.vae_wgrad_phase_ok(C.byref(a)), dll.vae_wgrad_io16_ok(C.byref(a)), [wrc, wns.value],
            dll.vae_wgrad_wino_positions(C.byref(a))]


# --------------------------------------------------------------------------- the grid
# geometries recorded with every variant (no option): between them they reach every kernel family the sparse sample below
# might miss (the <= 4-channel matrix-pipe kernels, conv1_bf16, both wide-tile forms, both Winograd forms, the 9-position
# weight gradient)
ANCHORS = ("c3:3>128:128x128:B16", "c3:128>3:32x32:B1", "c1:256>128:64x64:B32", "c3:128>128:256x256:B16",
           "c3up:256>256:64x64:B16", "c3:128>128:48x48:B2")


def selection(key):
    """the option sets a candidate case is recorded under (none: not recorded).  A fixed pseudo-random sample of the grid,
    each case under no option or one option chosen by the same hash; every variant of the anchor geometries; the
    bf16-image weight gradients of the stride-2 and upsampler layers at B = 2 under both settings of no_wgrad_dma (which
    reaches their selection three ways)."""
    h = zlib.crc32(key.encode())
    one = () if h % 4 == 0 else (OPTIONS[(h >> 8) % len(OPTIONS)],)
    if any(f"|{a}|" in key + "|" for a in ANCHORS):
        return [()]
    if key.startswith(("wgrad|c3s2", "wgrad|c3up")) and ":B2|p1|xf0|X16,dY16" in key:
        return [(), ("no_wgrad_dma",)]
    rate = 8 if key.startswith(("geom|", "updgrad|", "gemm_")) else 40 if key.startswith(("phase|", "wphase|")) else 300
    return [one] if (h >> 16) % rate == 0 else []


def cases():
    """yields (key, kind, argument block or (geom, Co, Ci)); key names the case, kind is 'conv' / 'wgrad' / 'geom'"""
    for kind, Ci, Co, div in LAYERS:
        for R in SIZES:
            H = W = R // div
            if H < 2:
                continue
            for B in BATCHES:
                base = f"{kind}:{Ci}>{Co}:{H}x{W}:B{B}"
                yield f"geom|{base}", "geom", (ops._fwd_geom(kind, B, H, W, Ci), Co, Ci)
                for prec in (F32, BF16):
                    for xf in (0, 1, 2):
                        for tag, a in conv_variants(conv_ptrs(ops.fwd_args(kind, B, H, W, Ci, Co, Ci, xf=xf, prec=prec)), False):
                            yield f"fwd|{base}|p{prec}|xf{xf}|{tag}", "conv", a
                    for tag, a in conv_variants(conv_ptrs(ops.dgrad_args(kind, B, H, W, Co, Ci, prec=prec)), True):
                        yield f"dgrad|{base}|p{prec}|{tag}", "conv", a
                    for xf in (0, 2):
                        for tag, a in wgrad_variants(wgrad_ptrs(ops.wgrad_args(kind, B, H, W, Ci, Co, Ci, xf=xf, prec=prec))):
                            yield f"wgrad|{base}|p{prec}|xf{xf}|{tag}", "wgrad", a
                if kind == "c3s2":  # the plain DGRAD form of a stride-2 layer as well
                    for prec in (F32, BF16):
                        yield f"dgrad|{base}|p{prec}|nos2", "conv", conv_ptrs(ops.dgrad_args(kind, B, H, W, Co, Ci, s2=False, prec=prec))
                if kind == "c3up":
                    a = conv_ptrs(ops.up2x_dgrad_args(B, H, W, Co, Ci, prec=F32))
                    yield f"updgrad|{base}", "conv", a
                    yield f"updgrad|{base}|Wu", "conv", _copy(a, Wu=P)
                    # the four phase convolutions on the low-resolution grid
                    for prec in (F32, BF16):
                        for tm in (0x1b, 0x36, 0xd8, 0x1b0):
                            for dg in (False, True):
                                a = _copy(conv_ptrs(ops.phase_args(B, H, W, Co, Ci, dg, prec=prec)), tapmask=tm)
                                pre = f"phase|{base}|p{prec}|{'dg' if dg else 'fw'}|{tm:x}"
                                yield pre, "conv", a
                                v = ([("A16", dict(Wh=P, A16=P)), ("A16,out16", dict(Wh=P, A16=P, out_bf16=1)), ("out16", dict(Wh=P, out_bf16=1))]
                                     if prec == BF16 else [("xf2", dict(xf=2, scale=P, shift=P))])
                                for tag, kw in v:
                                    yield f"{pre}|{tag}", "conv", _copy(a, **kw)
                            w = _copy(wgrad_ptrs(ops.wgrad_phase_args(B, H, W, Co, Ci, prec=prec)), tapmask=tm)
                            yield f"wphase|{base}|p{prec}|{tm:x}", "wgrad", w
                            if prec == BF16:
                                for tag, kw in (("X16,dY16", dict(X16=P, dY16=P)), ("dY16", dict(dY16=P)), ("xf2", dict(xf=2, scale=P, shift=P))):
                                    yield f"wphase|{base}|p{prec}|{tm:x}|{tag}", "wgrad", _copy(w, **kw)
    # the attention contractions: batched GEMMs (gemm_nt / gemm_nn through the rows kernels, gemm_tn through wgrad)
    for T in (16, 25, 36, 64, 256, 1024, 4096):
        for z in (1, 2, 16):
            for prec in (F32, BF16):
                for Cc in (512,):
                    for nm, M, N, K, bkm in (("nt", T, T, Cc, False), ("nn", T, Cc, T, True), ("nt_c", T, Cc, T, False)):
                        a = conv_ptrs(ops.gemm_rows_args(M, N, K, bkm, 0.125, z, prec=prec))
                        yield f"gemm_{nm}|T{T}|z{z}|p{prec}", "conv", a
                        yield f"gemm_{nm}|T{T}|z{z}|p{prec}|misaligned", "conv", _copy(a, A=MIS)
                    for nm, K, M, N in (("tn", T, T, Cc), ("tn_c", T, Cc, Cc), ("tn_s", T, Cc, T)):
                        a = _copy(wgrad_ptrs(ops.gemm_tn_args(M, N, K, 1.0, z, prec=prec)), out=P)
                        yield f"gemm_{nm}|T{T}|z{z}|p{prec}", "wgrad", a
                        yield f"gemm_{nm}|T{T}|z{z}|p{prec}|odd_sXb", "wgrad", _copy(a, sXb=K * N + 1)


def evaluate(dll, kind, obj):
    if kind == "conv":
        return conv_result(dll, obj)
    if kind == "wgrad":
        return wgrad_result(dll, obj)
    g, Co, Ci = obj
    return [dll.vae_bf16_act_image_ok(C.byref(g), Co, Ci), dll.vae_bf16_grad_image_ok(C.byref(g), Co, Ci)]


def _set_option(dll, name, value):
    assert dll.vae_set_option(name.encode(), value) == 0, name


def build_table():
    """{case key: recorded answers}; each selected case under the option sets selection() assigns it (the key ends with them).
    Every option is restored to the value it had."""
    dll = lib.load()
    dll.vae_wino_weight_floats.restype = C.c_int64
    prev = {o: dll.vae_get_option(o.encode()) for o in OPTIONS}
    table = {}
    try:
        for o in OPTIONS:
            _set_option(dll, o, 0)
        for key, kind, obj in cases():
            for opts in selection(key):
                for o in opts:
                    _set_option(dll, o, 1)
                try:
                    table[key + "|" + ",".join(opts)] = evaluate(dll, kind, obj)
                finally:
                    for o in opts:
                        _set_option(dll, o, 0)
    finally:
        for o, v in prev.items():
            _set_option(dll, o, v)
    return table


def dumps(table):
    """sorted keys, one case per line"""
    lines = [json.dumps(k) + ": " + json.dumps(table[k], separators=(",", ":")) for k in sorted(table)]
    return "{\n" + ",\n".join(lines) + "\n}\n"


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "dispatch_table.json")
    with open(out, "w") as f:
        f.write(dumps(build_table()))
    print(out)
