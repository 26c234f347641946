"""A/B of two (or more) builds of the fp32 Winograd weight gradient (csrc/wgrad3_wino.hip) in one process: this build against the
parent commit's libvaehip.so (built in a scratch worktree; nothing of it is committed), further builds optional.  Per shape X
and dY are filled once, every library's vae_wgrad_wino writes its own slab and bias partials, and they are compared with the
first library's BIT FOR BIT; then the arms are timed alternately with device events (warm-up, `--launches` launches per arm,
interleaved launch by launch): median, quartiles and extremes per arm.  Shapes: the plain 3x3 layers of the fp32 step (256^2,
batch 16) with the split count of vae_wgrad_wino_plan, and the small control-flow cases of tests/test_wgrad_stagger_gpu.py
(bitwise only).

usage: python tools/wgrad_stagger_ab.py NEW.so PARENT.so [name=OTHER.so ...] [--launches 30] [--out FILE]"""
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

# Cin, Cout, H, W, batch, xf, nsplit (0: the plan's)
BENCH = [(128, 128, 256, 256, 16, 0, 0), (256, 128, 256, 256, 16, 0, 0), (256, 256, 128, 128, 16, 0, 0), (512, 256, 128, 128, 16, 0, 0),
         (512, 512, 64, 64, 16, 0, 0), (512, 512, 32, 32, 16, 0, 0)]
SMALL = ([(32, 128, H, 16, B, 0, ns) for B, H in [(1, 2), (2, 2), (1, 6), (2, 4), (1, 10)] for ns in (1, 2, 4)]
         + [(64, 256, 8, 32, 1, 0, ns) for ns in (2, 3, 8)] + [(64, 128, 4, 16, 2, 2, 1), (32, 128, 2, 32, 3, 1, 2)])


def _p(t):
    return C.c_void_p(t.data_ptr())


def _open(path):
    lib.load()  # (one HIP runtime per process: the package's loader opens torch's copy first)
    dll = C.CDLL(os.path.abspath(path))
    for fn, argt in (("vae_wgrad_wino", [C.POINTER(WgradArgs), C.c_void_p]), ("vae_wgrad_wino_plan", [C.POINTER(WgradArgs), C.POINTER(C.c_int32)])):
        getattr(dll, fn).restype, getattr(dll, fn).argtypes = C.c_int, argt
    return dll


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="NEW.so PARENT.so [name=OTHER.so ...]")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default="")
    arg = ap.parse_args()
    assert len(arg.libs) >= 2, "two libraries: this build and the parent's"
    names = ["new", "parent"] + [s.split("=", 1)[0] for s in arg.libs[2:]]
    dlls = [_open(s.split("=", 1)[-1]) for s in arg.libs]
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows, all_equal = [], True
    for Ci, Co, H, W, B, xf, ns in BENCH + SMALL:
        timed = ns == 0
        g = torch.Generator(device=dev).manual_seed(Ci + Co + H + B)
        x = torch.randn((B, H, W, Ci), device=dev, generator=g)
        dy = torch.randn((B, H, W, Co), device=dev, generator=g)
        scale, shift = torch.rand((B, Ci), device=dev, generator=g) + 0.5, torch.randn((B, Ci), device=dev, generator=g)
        a = ops.wgrad_args("c3", B, H, W, Ci, Co, Ci, xf=xf, prec=ops.PREC_F32)
        a.dY, a.X = _p(dy), _p(x)
        if xf:
            a.scale, a.shift = _p(scale), _p(shift)
        if ns == 0:
            n = C.c_int32(0)
            assert dlls[0].vae_wgrad_wino_plan(C.byref(a), C.byref(n)) == 0 and n.value > 0
            ns = n.value
        a.nsplit = ns
        outs = []
        for d in dlls:
            slab = torch.full((ns, 16 * Ci * Co), float("nan"), device=dev)
            bpart = torch.full((ns, Co), float("nan"), device=dev)
            outs.append((slab, bpart))

        def call(i):
            a.partial, a.bias_partial = _p(outs[i][0]), _p(outs[i][1])
            rc = dlls[i].vae_wgrad_wino(C.byref(a), st)
            assert rc == 0, (names[i], rc)

        for i in range(len(dlls)):
            call(i)
        torch.cuda.synchronize()
        eq = {names[i]: bool(torch.equal(outs[i][0].view(torch.int32), outs[0][0].view(torch.int32))
                             and torch.equal(outs[i][1].view(torch.int32), outs[0][1].view(torch.int32))) for i in range(1, len(dlls))}
        finite = bool(torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all())
        all_equal = all_equal and all(eq.values()) and finite
        row = {"Cin": Ci, "Cout": Co, "H": H, "W": W, "batch": B, "xf": xf, "nsplit": ns, "bitwise_equal_to_new": eq, "finite": finite}
        if timed:
            for _ in range(3):
                for i in range(len(dlls)):
                    call(i)
            ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(arg.launches)] for _ in dlls]
            for k in range(arg.launches):
                for i in range(len(dlls)):
                    ev[i][k][0].record()
                    call(i)
                    ev[i][k][1].record()
            torch.cuda.synchronize()
            for i, nm in enumerate(names):
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[i])
                q = statistics.quantiles(ms, n=4)
                row[nm] = {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(ms[0], 4),
                           "max_ms": round(ms[-1], 4)}
            row["new_over_parent"] = round(row["new"]["median_ms"] / row["parent"]["median_ms"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del outs, x, dy
    res = {"libs": dict(zip(names, [s.split("=", 1)[-1] and os.path.basename(s.split("=", 1)[-1]) for s in arg.libs])), "launches_per_arm": arg.launches,
           "all_bitwise_equal": all_equal, "rows": rows}
    if arg.out:
        with open(arg.out, "w") as f:
            json.dump(res, f, indent=1)
    print("all slabs and bias partials bitwise equal:", all_equal)
    return 0 if all_equal else 1


if __name__ == "__main__":
    sys.exit(main())
