"""A/B of the fp32 <= 4-channel kernels (csrc/skinny.hip) with matrix-pipe bodies against their VALU bodies, three arms in one
process: this build, the `make -C csrc thin_f32_valu` build (libvaehip_thin_valu.so, -DVAE_THIN_F32_MFMA=0) and the parent commit's
libvaehip.so (built in a scratch worktree; nothing of it is committed).  Launches: the five full-resolution ones of the fp32 step
(256^2, batch 16, 128 wide channels: encoder.conv_in forward and weight gradient, decoder.conv_out forward with GroupNorm + SiLU on
load, its dgrad and its weight gradient) and the latent ones (decoder.conv_in 4 -> 512 at 32^2 forward and weight gradient, a
1x1 4 -> 4 forward).  Operands are filled once; every arm launches through its own library into its own output.  Reported per launch:
  * the off arm's result against the parent's BIT FOR BIT (the off build is the parent's kernel);
  * two launches of the new arm bit for bit;
  * each arm's error against a float64 evaluation of the same operands on the device, on the scale of the result's max;
  * the time per arm, alternating launch by launch with the opening arm moving on by one every round, device events (warm-up,
    `--launches` launches per arm): median, quartiles, extremes, and whether the new arm's quartiles lie clear below the parent's;
  * the time of one plain streaming pass over the wide tensor's bytes (ops.moments of a tensor of that size, timed the same way in
    the same process) and each arm's ratio to it.

usage: python tools/thin_f32_ab.py NEW.so OFF.so PARENT.so [--launches 20] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vae-channel-dynamics_amd", "src"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from vaehip import ops  # noqa: E402
from vaehip.lib import IgemmArgs, WgradArgs, lib  # noqa: E402

NAMES = ("new", "off", "parent")
# name, form, kind, (B, H, W), Cs, Co, Ci, xf
LAUNCHES = [
    ("encoder.conv_in forward", "fwd", "c3", (16, 256, 256), 4, 128, 3, 0),
    ("encoder.conv_in wgrad", "wgrad", "c3", (16, 256, 256), 4, 128, 3, 0),
    ("decoder.conv_out forward", "fwd", "c3", (16, 256, 256), 128, 3, 128, 2),
    ("decoder.conv_out dgrad", "dgrad", "c3", (16, 256, 256), 128, 3, 128, 0),
    ("decoder.conv_out wgrad", "wgrad", "c3", (16, 256, 256), 128, 3, 128, 2),
    ("decoder.conv_in forward", "fwd", "c3", (16, 32, 32), 4, 512, 4, 0),
    ("decoder.conv_in wgrad", "wgrad", "c3", (16, 32, 32), 4, 512, 4, 0),
    ("post_quant_conv forward", "fwd", "c1", (16, 32, 32), 4, 4, 4, 0),
]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _open(path):
    lib.load()  # (one HIP runtime per process: the package's loader opens torch's copy first)
    dll = C.CDLL(os.path.abspath(path))
    ia, wa, vp, i32 = C.POINTER(IgemmArgs), C.POINTER(WgradArgs), C.c_void_p, C.POINTER(C.c_int32)
    for fn, argt in (("vae_igemm_rows", [ia, vp]), ("vae_wgrad", [wa, vp]), ("vae_wgrad_plan", [wa, i32, i32]),
                     ("vae_igemm_kernel_name", [ia, C.c_char_p, C.c_int32]), ("vae_wgrad_kernel_name", [wa, C.c_char_p, C.c_int32])):
        getattr(dll, fn).restype, getattr(dll, fn).argtypes = C.c_int, argt
    return dll


def _name(dll, fn, a):
    buf = C.create_string_buffer(128)
    getattr(dll, fn)(C.byref(a), buf, 128)
    return buf.value.decode()


def _shifted(t, kh, kw, k):
    """t [B,H,W,C] -> the tensor a tap (kh, kw) of a k x k 'same' kernel reads, zeros at padding"""
    if k == 1:
        return t
    B, H, W, _ = t.shape
    return F.pad(t, (0, 0, 1, 1, 1, 1))[:, kh:kh + H, kw:kw + W]


def _xf64(x, scale, shift, xf):
    x = x.double()
    if xf == 0:
        return x
    a = x * scale.double()[:, None, None, :] + shift.double()[:, None, None, :]
    return a * torch.sigmoid(a) if xf == 2 else a


def _ref_fwd(x, w, bias, k):
    """x [B,H,W,Ci] float64, w [Co,taps,Ci] -> [B*H*W, Co] float64"""
    y = sum(_shifted(x, t // k, t % k, k).reshape(-1, x.shape[-1]) @ w[:, t].double().T for t in range(k * k))
    return y + bias.double()


def _ref_dgrad(dy, w, k):
    """dy [B,H,W,Co] float64, w [Co,taps,Ci] -> [B*H*W, Ci]: the transposed taps"""
    return sum(_shifted(dy, k - 1 - t // k, k - 1 - t % k, k).reshape(-1, dy.shape[-1]) @ w[:, t].double() for t in range(k * k))


def _ref_wgrad(dy, x, k):
    """-> [Co,taps,Ci] float64"""
    d = dy.reshape(-1, dy.shape[-1]).T.contiguous()
    return torch.stack([d @ _shifted(x, t // k, t % k, k).reshape(-1, x.shape[-1]) for t in range(k * k)], dim=1)


def _stats(ms):
    ms = sorted(ms)
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def _rotate(calls, launches):
    """time the calls launch by launch, the opening arm moving on by one every round -> per call its times in ms"""
    for _ in range(3):
        for c in calls:
            c()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)] for _ in calls]
    for k in range(launches):
        for i in [(k + j) % len(calls) for j in range(len(calls))]:
            ev[i][k][0].record()
            calls[i]()
            ev[i][k][1].record()
    torch.cuda.synchronize()
    return [[e0.elapsed_time(e1) for e0, e1 in evs] for evs in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=3, help="NEW.so OFF.so PARENT.so")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    arg = ap.parse_args()
    dlls = [_open(s) for s in arg.libs]
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    rows, ok = [], True
    for name, form, kind, (B, H, W), Cs, Co, Ci, xf in LAUNCHES:
        g = torch.Generator(device=dev).manual_seed(len(rows) + 1)
        k = 1 if kind == "c1" else 3
        x = torch.randn((B, H, W, Cs), device=dev, generator=g)
        x[..., Ci:] = 1e4  # channels of the storage that no kernel may read
        dy = torch.randn((B, H, W, Co), device=dev, generator=g)
        w = torch.randn((Co, k * k, Ci), device=dev, generator=g) / (k * Ci ** 0.5)
        bias = torch.randn((Co,), device=dev, generator=g) * 0.5  # (forward only)
        scale = shift = None
        if xf:
            scale, shift = torch.rand((B, Cs), device=dev, generator=g) + 0.5, torch.randn((B, Cs), device=dev, generator=g) * 0.5
        wide_bytes = 4 * B * H * W * max(Co, Ci)
        if form == "wgrad":
            a = ops.wgrad_args(kind, B, H, W, Cs, Co, Ci, xf=xf, prec=ops.PREC_F32)
            a.dY, a.X, a.scale, a.shift = _p(dy), _p(x), _p(scale), _p(shift)
            ns, fus = C.c_int32(0), C.c_int32(0)
            plans = []
            for d in dlls:
                assert d.vae_wgrad_plan(C.byref(a), C.byref(ns), C.byref(fus)) == 0 and fus.value == 1
                plans.append(ns.value)
            assert len(set(plans)) == 1, plans
            a.nsplit = plans[0]
            n = Co * k * k * Ci
            outs = [torch.full((a.nsplit, n + Co), float("nan"), device=dev) for _ in range(4)]  # per split: the slab, then the bias partials
            kname = _name(dlls[0], "vae_wgrad_kernel_name", a)

            def call(i, out=None):
                o = outs[i] if out is None else out
                a.out, a.partial = (_p(o), None) if a.nsplit == 1 else (None, _p(o))
                a.bias_partial = C.c_void_p(o.data_ptr() + 4 * a.nsplit * n)
                rc = dlls[i].vae_wgrad(C.byref(a), st)
                assert rc == 0, (NAMES[i], rc)

            def value(o):
                flat = o.reshape(-1)
                return torch.cat([flat[:a.nsplit * n].reshape(a.nsplit, n).double().sum(0), flat[a.nsplit * n:].reshape(a.nsplit, Co).double().sum(0)])

            ref = torch.cat([_ref_wgrad(dy.double(), _xf64(x, scale, shift, xf)[..., :Ci], k).reshape(-1), dy.double().sum((0, 1, 2))])
            nref = n  # the figure is taken over dW; db is reported on its own scale
        else:
            a = ops.fwd_args(kind, B, H, W, Cs, Co, Ci, xf=xf, prec=ops.PREC_F32) if form == "fwd" else ops.dgrad_args(kind, B, H, W, Co, Ci, s2=False, prec=ops.PREC_F32)
            src = x if form == "fwd" else dy
            a.A, a.W, a.bias, a.scale, a.shift = _p(src), _p(w), (_p(bias) if form == "fwd" else None), _p(scale), _p(shift)
            outs = [torch.full((B * H * W, a.N), float("nan"), device=dev) for _ in range(4)]
            kname = _name(dlls[0], "vae_igemm_kernel_name", a)

            def call(i, out=None):
                a.C = _p(outs[i] if out is None else out)
                rc = dlls[i].vae_igemm_rows(C.byref(a), st)
                assert rc == 0, (NAMES[i], rc)

            def value(o):
                return o.double().reshape(-1)

            ref = (_ref_fwd(_xf64(x, scale, shift, xf)[..., :Ci], w, bias, k) if form == "fwd" else _ref_dgrad(dy.double(), w, k)).reshape(-1)
            nref = ref.numel()
        for i in range(3):
            call(i)
        call(0, outs[3])
        torch.cuda.synchronize()
        row = {"launch": name, "kernel": kname, "map": [B, H, W], "wide_tensor_MB": round(wide_bytes / 1e6, 1),
               "off_bitwise_equal_to_parent": bool(torch.equal(bits(outs[1]), bits(outs[2]))),
               "new_bitwise_equal_to_parent": bool(torch.equal(bits(outs[0]), bits(outs[2]))),
               "new_two_launches_bitwise_equal": bool(torch.equal(bits(outs[0]), bits(outs[3])))}
        for i in range(3):
            v = value(outs[i])
            row[f"{NAMES[i]}_err_of_max"] = float((v[:nref] - ref[:nref]).abs().max() / ref[:nref].abs().max())
            if form == "wgrad":
                row[f"{NAMES[i]}_db_err_of_max"] = float((v[nref:] - ref[nref:]).abs().max() / ref[nref:].abs().max())
        del ref
        ok = ok and row["off_bitwise_equal_to_parent"] and row["new_two_launches_bitwise_equal"]
        stream = torch.randn((wide_bytes // 4 // 128, 128), device=dev).reshape(1, 1, -1, 128)
        times = _rotate([lambda i=i: call(i) for i in range(3)] + [lambda: ops.moments(stream)], arg.launches)
        for nm, ms in zip(NAMES + ("stream",), times):
            row[nm] = _stats(ms)
        for nm in NAMES:
            row[nm + "_over_stream"] = round(row[nm]["median_ms"] / row["stream"]["median_ms"], 2)
        row["new_over_parent"] = round(row["new"]["median_ms"] / row["parent"]["median_ms"], 4)
        row["off_over_parent"] = round(row["off"]["median_ms"] / row["parent"]["median_ms"], 4)
        row["new_quartiles_clear_below_parent"] = bool(row["new"]["q3_ms"] < row["parent"]["q1_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
        del outs, x, dy, stream
    res = {"libs": dict(zip(NAMES, [os.path.basename(s) for s in arg.libs])), "launches_per_arm": arg.launches, "all_bitwise_checks_hold": ok, "rows": rows}
    if arg.out:
        with open(arg.out, "w") as f:
            json.dump(res, f, indent=1)
    print("off == parent, new launch == new launch, bit for bit:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
