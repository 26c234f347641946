"""A/B of the fp32 Winograd weight gradient (csrc/wgrad3_wino.hip) on split-bf16 products against exact fp32 products, three
arms in one process: this build, the `make -C csrc wgrad_x3_off` build (libvaehip_wgrad_x3off.so, -DVAE_WGRAD_X3=0) and the
parent commit's libvaehip.so (built in a scratch worktree; nothing of it is committed).  Per shape X and dY are filled once and
every library's vae_wgrad_wino writes its own slab and bias partials.  Reported per shape:
  * the off arm's slab and bias partials against the parent's BIT FOR BIT (the off build is the parent's kernel);
  * the error of the new and the off arm against float64: the slab goes through vae_wgrad_wino_reduce and the 8 x 8 channel corner
    dW[:8, :, :, :8] is compared with the sum over pixels in float64 (nine 8 x N by N x 8 products on the device), on the scale
    of that corner's max; the bias partials of the new arm against the off arm's bit for bit (the staging did not change);
  * two launches of the new arm bit for bit;
  * the time of the arms, alternating launch by launch with device events (warm-up, `--launches` launches per arm): median,
    quartiles and extremes per arm.
Shapes: the six distinct plain 3x3 launches of the fp32 step (256^2, batch 16) with the split count of vae_wgrad_wino_plan.

--upsampler: the same three arms for the upsampler weight gradient (csrc/wgrad3_upwino.hip, 9 positions; OFF = the
`make -C csrc upwgrad_x3_off` build, libvaehip_upwgrad_x3off.so, -DVAE_UPWGRAD_X3=0) on the step's three upsamplers: 512 -> 512 at
32^2 and 64^2, 256 -> 256 at 128^2 (low resolution).  --rotate: the opening arm moves on by one every round (N O P, O P N, ...).

usage: python tools/wgrad_x3_ab.py NEW.so OFF.so PARENT.so [--upsampler] [--rotate] [--launches 30] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vae-channel-dynamics_amd", "src"))
import torch  # noqa: E402
from vaehip import ops  # noqa: E402
from vaehip.lib import WgradArgs, lib  # noqa: E402

# Cin, Cout, map, batch
BENCH = [(128, 128, 256, 16), (256, 128, 256, 16), (256, 256, 128, 16), (512, 256, 128, 16), (512, 512, 64, 16), (512, 512, 32, 16)]
BENCH_UP = [(512, 512, 32, 16), (512, 512, 64, 16), (256, 256, 128, 16)]  # (map: the low-resolution x)
NAMES = ("new", "off", "parent")
SUB = 8  # channels of the corner held to float64


def _p(t):
    return C.c_void_p(t.data_ptr())


def _open(path):
    lib.load()  # (one HIP runtime per process: the package's loader opens torch's copy first)
    dll = C.CDLL(os.path.abspath(path))
    for fn, argt in (("vae_wgrad_wino", [C.POINTER(WgradArgs), C.c_void_p]), ("vae_wgrad_wino_plan", [C.POINTER(WgradArgs), C.POINTER(C.c_int32)])):
        getattr(dll, fn).restype, getattr(dll, fn).argtypes = C.c_int, argt
    return dll


def _corner_f64(x, dy, up=False):
    """dW[:SUB, :, :, :SUB] of the 3x3 stride-1 pad-1 weight gradient in float64: [SUB co][3][3][SUB ci] (up: of the nearest-
    upsampled x)"""
    xs = x[..., :SUB].double()
    if up:
        xs = xs.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    B, H, W, _ = xs.shape
    xp = torch.nn.functional.pad(xs, (0, 0, 1, 1, 1, 1))
    d = dy[..., :SUB].double().reshape(-1, SUB)
    out = torch.empty((SUB, 3, 3, SUB), dtype=torch.float64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            out[:, kh, kw, :] = d.T @ xp[:, kh:kh + H, kw:kw + W, :].reshape(-1, SUB)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=3, help="NEW.so OFF.so PARENT.so")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--upsampler", action="store_true", help="wgrad3_upwino_kernel on the step's three upsamplers")
    ap.add_argument("--rotate", action="store_true", help="rotate the opening arm every round")
    ap.add_argument("--out", default="")
    arg = ap.parse_args()
    dlls = [_open(s) for s in arg.libs]
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows, ok = [], True
    up = arg.upsampler
    npos = 9 if up else 16
    for Ci, Co, H, B in (BENCH_UP if up else BENCH):
        g = torch.Generator(device=dev).manual_seed(Ci + Co + H + B)
        x = torch.randn((B, H, H, Ci), device=dev, generator=g)
        dy = torch.randn((B, 2 * H, 2 * H, Co) if up else (B, H, H, Co), device=dev, generator=g)
        a = ops.wgrad_args("c3up" if up else "c3", B, H, H, Ci, Co, Ci, prec=ops.PREC_F32)
        a.dY, a.X = _p(dy), _p(x)
        n = C.c_int32(0)
        assert dlls[0].vae_wgrad_wino_plan(C.byref(a), C.byref(n)) == 0 and n.value > 0
        ns = a.nsplit = n.value
        outs = [(torch.full((ns, npos * Ci * Co), float("nan"), device=dev), torch.full((ns, Co), float("nan"), device=dev)) for _ in dlls]

        def call(i, out=None):
            slab, bpart = out or outs[i]
            a.partial, a.bias_partial = _p(slab), _p(bpart)
            rc = dlls[i].vae_wgrad_wino(C.byref(a), st)
            assert rc == 0, (NAMES[i], rc)

        for i in range(3):
            call(i)
        again = (torch.full_like(outs[0][0], float("nan")), torch.full_like(outs[0][1], float("nan")))
        call(0, again)
        torch.cuda.synchronize()
        bits = lambda t: t.view(torch.int32)  # noqa: E731
        row = {"Cin": Ci, "Cout": Co, "map": H, "batch": B, "nsplit": ns,
               "off_bitwise_equal_to_parent": bool(torch.equal(bits(outs[1][0]), bits(outs[2][0])) and torch.equal(bits(outs[1][1]), bits(outs[2][1]))),
               "new_bias_partials_bitwise_equal_to_off": bool(torch.equal(bits(outs[0][1]), bits(outs[1][1]))),
               "new_two_launches_bitwise_equal": bool(torch.equal(bits(outs[0][0]), bits(again[0])) and torch.equal(bits(outs[0][1]), bits(again[1])))}
        ref = _corner_f64(x, dy, up)
        for i in (0, 1):
            dW = torch.full((Co, 3, 3, Ci), float("nan"), device=dev)
            lib.call("vae_wgrad_wino_reduce", _p(outs[i][0]), ns, npos, Ci, Co, None, _p(dW), None, None, st)
            row[f"{NAMES[i]}_err_of_corner_max"] = float((dW[:SUB, :, :, :SUB].double() - ref).abs().max() / ref.abs().max())
        ok = ok and row["off_bitwise_equal_to_parent"] and row["new_bias_partials_bitwise_equal_to_off"] and row["new_two_launches_bitwise_equal"]
        for _ in range(3):
            for i in range(3):
                call(i)
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(arg.launches)] for _ in dlls]
        for k in range(arg.launches):
            for i in ([(k + j) % 3 for j in range(3)] if arg.rotate else range(3)):
                ev[i][k][0].record()
                call(i)
                ev[i][k][1].record()
        torch.cuda.synchronize()
        for i, nm in enumerate(NAMES):
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[i])
            q = statistics.quantiles(ms, n=4)
            row[nm] = {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(ms[0], 4),
                       "max_ms": round(ms[-1], 4)}
        row["new_over_parent"] = round(row["new"]["median_ms"] / row["parent"]["median_ms"], 4)
        row["off_over_parent"] = round(row["off"]["median_ms"] / row["parent"]["median_ms"], 4)
        row["new_quartiles_clear_below_parent"] = bool(row["new"]["q3_ms"] < row["parent"]["q1_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
        del outs, again, x, dy
    res = {"libs": dict(zip(NAMES, [os.path.basename(s) for s in arg.libs])), "launches_per_arm": arg.launches, "all_bitwise_checks_hold": ok, "rows": rows}
    if arg.out:
        with open(arg.out, "w") as f:
            json.dump(res, f, indent=1)
    print("off == parent, new bias == off bias, new launch == new launch, bit for bit:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
