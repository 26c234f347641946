"""Where a step of the fp32 Winograd weight gradient (csrc/wgrad3_wino.hip) spends its time: shader-clock stamps of waves 0 and 4
(the two waves of SIMD 0) of workgroups 0..7 for steps 2..9, instrumented build (`make -C csrc timing`, loaded through
VAEHIP_LIB; `make timing TIMING_FLAGS=-DVAE_WGRAD_DEFER=0 TIMING_LIB=libvaehip_timing_d0.so` for all waves on one program).
Per step a wave of the exact loop (-DVAE_WGRAD_X3=0) owes 32 v_mfma_f32_32x32x2_f32 of 64 cycles = 2048 cycles of matrix work, a SIMD
4096; in the split-bf16 loop a step is a PAIR of units, 48 v_mfma_f32_32x32x16_bf16 of 32 cycles = 1536 per wave, 3072 per SIMD,
and nothing is held back (`held` reads zero).  Segments per step:
  held   the MFMAs held back from the step before (waves 4..7 only; 0 in waves 0..3)
  head   LDS reads and operand building up to the first own MFMA (waves 0..3: their LDS stores of the next unit included)
  mfma   first to last own MFMA issued, operand building of the later blocks interleaved
  tail   behind the last MFMA up to the barrier (waves 4..7: their LDS stores)
  wait   at the barrier
`both heads` = cycles per step in which wave 0 and wave 4 are both in a segment without MFMAs of their own (head, tail, wait):
the matrix pipe of the SIMD has nothing to do.  The stamps are intrusive: read the segments as a picture.
usage: VAEHIP_LIB=vae-channel-dynamics_amd/csrc/libvaehip_timing.so python tools/wgrad_timing.py [--json FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from vaehip import ops  # noqa: E402
from vaehip.lib import LIB_PATH, lib  # noqa: E402

# Cin, Cout, map size, batch: the plain 3x3 layers of the fp32 step at 256^2, batch 16
SHAPES = [(128, 128, 256, 16), (256, 128, 256, 16), (256, 256, 128, 16), (512, 256, 128, 16), (512, 512, 64, 16), (512, 512, 32, 16)]
TSN, NW = 8, 4 + 8 * 5
SEG = ("held", "head", "mfma", "tail", "wait")


def idle_overlap(a, b):
    """cycles in which both waves are outside [step begin, last MFMA issued) minus their head, per step (interval arithmetic
    on the absolute stamps of one workgroup): a, b = [TSN][5] stamps of wave 0 and wave 4"""
    def quiet(t):  # intervals without own MFMAs: [held done, first MFMA) and [last MFMA, next step's begin)
        iv = []
        for s in range(TSN - 1):
            iv += [(t[s, 1], t[s, 2]), (t[s, 3], t[s + 1, 0])]
        return iv
    tot = 0.0
    for x0, x1 in quiet(a):
        for y0, y1 in quiet(b):
            tot += max(0.0, min(x1, y1) - max(x0, y0))
    return tot / (TSN - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    arg = ap.parse_args()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for Ci, Co, H, B in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn((B, H, H, Ci), device=dev, generator=g)
        dy = torch.randn((B, H, H, Co), device=dev, generator=g)
        a = ops.wgrad_args("c3", B, H, H, Ci, Co, Ci, prec=ops.PREC_F32)
        a.dY, a.X = C.c_void_p(dy.data_ptr()), C.c_void_p(x.data_ptr())
        ns = C.c_int32(0)
        lib.call("vae_wgrad_wino_plan", C.byref(a), C.byref(ns))
        slab = torch.empty((ns.value, 16 * Ci * Co), device=dev)
        stamps = torch.zeros(8 * 2 * NW, device=dev, dtype=torch.int64)
        a.nsplit, a.partial, a.out = ns.value, C.c_void_p(slab.data_ptr()), C.c_void_p(stamps.data_ptr())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(10):
            stamps.zero_()
            e0.record()
            lib.call("vae_wgrad_wino", C.byref(a), st)
            e1.record()
        torch.cuda.synchronize()
        t = stamps.cpu().numpy().reshape(8, 2, NW).astype("float64")
        if not t[:, :, 0].any():
            sys.exit(f"no stamps: {LIB_PATH} is not an instrumented build (make -C csrc timing)")
        units = B * (H // 2) * (H // 16)
        print(f"Cin {Ci} Cout {Co} {H}x{H} batch {B}: nsplit {ns.value}, {units // ns.value} units per workgroup, {e0.elapsed_time(e1):.3f} ms", flush=True)
        seg = np.zeros((8, 2, 5))
        per, both = np.zeros(8), np.zeros(8)
        for wg in range(8):
            s = t[wg, :, 4:].reshape(2, TSN, 5)
            for wv in range(2):
                d = np.diff(s[wv], axis=1)[:-1]                       # held, head, mfma, tail of steps 0..TSN-2
                wait = s[wv, 1:, 0] - s[wv, :-1, 4]
                seg[wg, wv] = np.append(d.mean(axis=0), wait.mean())
            per[wg] = (s[0, -1, 0] - s[0, 0, 0]) / (TSN - 1)
            both[wg] = idle_overlap(s[0], s[1])
            ghz = (t[wg, 0, 1] - t[wg, 0, 0]) / max(t[wg, 0, 3] - t[wg, 0, 2], 1) * 0.1
            print(f"  wg {wg}: {per[wg]:5.0f} cycles/step, both heads {both[wg]:5.0f}, clock {ghz:4.2f} GHz | " + " | ".join(
                f"wave {4 * wv}: " + " ".join(f"{n} {v:5.0f}" for n, v in zip(SEG, seg[wg, wv])) for wv in range(2)), flush=True)
        rows.append({"Cin": Ci, "Cout": Co, "map": H, "batch": B, "nsplit": ns.value, "cycles_per_step": round(float(per.mean())),
                     "both_waves_without_mfma": round(float(both.mean())),
                     **{f"wave{4 * wv}_{n}": round(float(seg[:, wv, i].mean())) for wv in range(2) for i, n in enumerate(SEG)}})
    if arg.json:
        with open(arg.json, "w") as f:
            json.dump({"lib": os.path.basename(LIB_PATH), "steps": "2..9 of workgroups 0..7, means", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
