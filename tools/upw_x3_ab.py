"""A/B of the fp32 upsampler convolution (csrc/conv3_upwino.hip) on split-bf16 products from bf16 planes of U and V against exact
fp32 products, three arms in one process: this build, the `make -C csrc upw_x3_off` build (libvaehip_upw_x3off.so,
-DVAE_UPW_X3=0) and the parent commit's libvaehip.so (built in a scratch worktree; nothing of it is committed).  Per layer and
direction the operands are filled once; every library builds its own transformed weights (vae_wino_weights into a buffer of
vae_wino_weight_bytes, or of 4 x vae_wino_weight_floats where a library does not have that query) and launches vae_igemm_rows
into its own output.  Reported per layer and direction:
  * the off arm's output and U against the parent's BIT FOR BIT (the off build is the parent's kernel);
  * two launches of the new arm bit for bit; the new arm's output against the parent's bit for bit, reported (it holds when the new
    build changes the tiling and not the sums: the workgroup width, off arm = `make -C csrc upw_nb2`);
  * the error of the new and the off arm against float64 on a corner: the first 8 output channels of the first 8 x 8 output pixels
    of image 0 (a float64 convolution of the crop that reaches them, on the device), on the scale of that corner's max;
  * the time of vae_igemm_rows per arm, alternating launch by launch (the order reversed every round) with device events (warm-up,
    `--launches` launches per arm): median, quartiles and extremes, and whether the new arm's quartiles lie clear below the
    parent's; the weights kernel's time per arm the same way (it runs once per launch in training and writes 1.5 x the bytes
    under the split build).
Layers: the three upsamplers of the fp32 step (256^2, batch 16): 512 -> 512 at 32^2 and 64^2, 256 -> 256 at 128^2 (low resolution).

--rotate: the opening arm moves on by one every round (N O P, O P N, ...).

usage: python tools/upw_x3_ab.py NEW.so OFF.so PARENT.so [--launches 20] [--rotate] [--out FILE]"""
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
from vaehip.lib import IgemmArgs, lib  # noqa: E402

# channels (Cin = Cout), low-resolution map, batch
BENCH = [(512, 32, 16), (512, 64, 16), (256, 128, 16)]
NAMES = ("new", "off", "parent")
SUB = 8  # output channels and output pixels (each way) of the corner held to float64


def _p(t):
    return C.c_void_p(t.data_ptr())


def _open(path):
    lib.load()  # (one HIP runtime per process: the package's loader opens torch's copy first)
    dll = C.CDLL(os.path.abspath(path))
    ia, vp = C.POINTER(IgemmArgs), C.c_void_p
    for fn, res, argt in (("vae_igemm_rows", C.c_int, [ia, vp]), ("vae_wino_ok", C.c_int, [ia]), ("vae_wino_weight_floats", C.c_int64, [ia]),
                          ("vae_wino_weights", C.c_int, [ia, vp, vp])):
        getattr(dll, fn).restype, getattr(dll, fn).argtypes = res, argt
    if hasattr(dll, "vae_wino_weight_bytes"):
        dll.vae_wino_weight_bytes.restype, dll.vae_wino_weight_bytes.argtypes = C.c_int64, [ia]
    return dll


def _wu_bytes(dll, a):
    return int(dll.vae_wino_weight_bytes(C.byref(a))) if hasattr(dll, "vae_wino_weight_bytes") else 4 * int(dll.vae_wino_weight_floats(C.byref(a)))


def _corner_f64(src, w, dgrad):
    """[SUB, SUB, SUB]: rows, columns, channels of image 0's first output pixels in float64 (w: OHWI)"""
    if dgrad:  # the gradient wrt the upsampled image from the dY rows that reach its first 2 SUB rows, summed 2 x 2
        dy = src[0, :2 * SUB + 2, :2 * SUB + 2].double().permute(2, 0, 1)[None]
        hi = F.conv_transpose2d(dy, w[..., :SUB].double().permute(0, 3, 1, 2), None, 1, 1)
        return F.avg_pool2d(hi, 2, divisor_override=1)[0, :, :SUB, :SUB].permute(1, 2, 0)
    x = src[0, :SUB // 2 + 2, :SUB // 2 + 2].double().permute(2, 0, 1)[None]
    y = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w[:SUB].double().permute(0, 3, 1, 2), None, 1, 1)
    return y[0, :, :SUB, :SUB].permute(1, 2, 0)


def _stats(ms):
    ms = sorted(ms)
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def _alternate(calls, launches, rotate=False):
    """time the calls, alternating launch by launch -> per call the list of its times in ms.  The order is reversed every round
    (N O P, P O N, ...): a launch reads 3-6 % slower right behind a launch of the split kernel than behind one of the exact kernel
    (identical code in two seats of a fixed order differed by that much), and this way the first and the last arm meet the same
    predecessors"""
    for _ in range(3):
        for c in calls:
            c()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)] for _ in calls]
    for k in range(launches):
        order = range(len(calls)) if k % 2 == 0 else range(len(calls) - 1, -1, -1)
        if rotate:  # the opening arm moves on by one every round (N O P, O P N, ...)
            order = [(k + j) % len(calls) for j in range(len(calls))]
        for i in order:
            ev[i][k][0].record()
            calls[i]()
            ev[i][k][1].record()
    torch.cuda.synchronize()
    return [[e0.elapsed_time(e1) for e0, e1 in evs] for evs in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=3, help="NEW.so OFF.so PARENT.so")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rotate", action="store_true", help="rotate the opening arm every round")
    ap.add_argument("--out", default="")
    arg = ap.parse_args()
    dlls = [_open(s) for s in arg.libs]
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    rows, ok = [], True
    for Ch, H, B in BENCH:
        g = torch.Generator(device=dev).manual_seed(Ch + H + B)
        w = torch.randn((Ch, 3, 3, Ch), device=dev, generator=g) / (3.0 * Ch ** 0.5)
        for dgrad in (False, True):
            src = torch.randn((B, 2 * H, 2 * H, Ch) if dgrad else (B, H, H, Ch), device=dev, generator=g)
            a = ops.up2x_dgrad_args(B, H, H, Ch, Ch, prec=ops.PREC_F32) if dgrad else ops.fwd_args("c3up", B, H, H, Ch, Ch, Ch, prec=ops.PREC_F32)
            oshape = (B, H, H, Ch) if dgrad else (B, 2 * H, 2 * H, Ch)
            outs = [torch.full(oshape, float("nan"), device=dev) for _ in dlls]
            a.A, a.W, a.C = _p(src), _p(w), _p(outs[0])
            assert all(d.vae_wino_ok(C.byref(a)) for d in dlls)
            wus = [torch.full(((_wu_bytes(d, a) + 3) // 4,), float("nan"), device=dev) for d in dlls]

            def weights(i):
                a.Wu = None
                rc = dlls[i].vae_wino_weights(C.byref(a), _p(wus[i]), st)
                assert rc == 0, (NAMES[i], rc)

            def call(i, out=None):
                a.C, a.Wu = _p(out if out is not None else outs[i]), _p(wus[i])
                rc = dlls[i].vae_igemm_rows(C.byref(a), st)
                assert rc == 0, (NAMES[i], rc)

            for i in range(3):
                weights(i)
                call(i)
            again = torch.full_like(outs[0], float("nan"))
            call(0, again)
            torch.cuda.synchronize()
            row = {"channels": Ch, "low_res_map": H, "batch": B, "direction": "dgrad" if dgrad else "forward",
                   "wu_bytes": {nm: int(t.numel() * 4) for nm, t in zip(NAMES, wus)},
                   "off_bitwise_equal_to_parent": bool(torch.equal(bits(outs[1]), bits(outs[2])) and torch.equal(bits(wus[1]), bits(wus[2]))),
                   "new_bitwise_equal_to_parent": bool(torch.equal(bits(outs[0]), bits(outs[2]))),
                   "new_two_launches_bitwise_equal": bool(torch.equal(bits(outs[0]), bits(again)))}
            ref = _corner_f64(src, w, dgrad)
            for i in (0, 1):
                row[f"{NAMES[i]}_err_of_corner_max"] = float((outs[i][0, :SUB, :SUB, :SUB].double() - ref).abs().max() / ref.abs().max())
            ok = ok and row["off_bitwise_equal_to_parent"] and row["new_two_launches_bitwise_equal"]
            for nm, ms in zip(NAMES, _alternate([lambda i=i: call(i) for i in range(3)], arg.launches, arg.rotate)):
                row[nm] = _stats(ms)
            for nm, ms in zip(NAMES, _alternate([lambda i=i: weights(i) for i in range(3)], arg.launches, arg.rotate)):
                row[nm + "_weights"] = _stats(ms)
            row["new_over_parent"] = round(row["new"]["median_ms"] / row["parent"]["median_ms"], 4)
            row["off_over_parent"] = round(row["off"]["median_ms"] / row["parent"]["median_ms"], 4)
            row["new_quartiles_clear_below_parent"] = bool(row["new"]["q3_ms"] < row["parent"]["q1_ms"])
            print(json.dumps(row), flush=True)
            rows.append(row)
            del outs, again, src, wus
    res = {"libs": dict(zip(NAMES, [os.path.basename(s) for s in arg.libs])), "launches_per_arm": arg.launches, "all_bitwise_checks_hold": ok, "rows": rows}
    if arg.out:
        with open(arg.out, "w") as f:
            json.dump(res, f, indent=1)
    print("off == parent (outputs and U), new launch == new launch, bit for bit:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
