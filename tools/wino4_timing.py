"""Where a workgroup of the fp32 Winograd F(4x4,3x3) forward (csrc/conv3_wino4.hip) spends its time: shader-clock stamps of waves
0, 4, 8 (the first wave of each wave group: the three waves of SIMD 0, in dispatch order) of workgroups 0..7, instrumented build
(`make -C csrc timing`, loaded through VAEHIP_LIB).  Per step 24 MFMAs of 64 cycles per wave = 1536 cycles of matrix work per
wave, 4608 per SIMD.  Phases of a step, summed by each wave over steps 2..9 in scalar registers (the kernel has no vector register
to spare for stamps): begin | MFMA groups 0-1 with their transform slices | groups 2-3 | groups 4-5 and the DMA wait -> arrival
at the barrier | barrier wait.  Waves 0-3 transform row pair {1,2}, waves 4-7 {3,4}, waves 8-11 {0,5}.
The stamps are intrusive (each one drains the wave's LDS queue): read the phases as a picture, not as the production kernel's times.
usage: VAEHIP_LIB=vae-channel-dynamics_amd/csrc/libvaehip_timing.so python tools/wino4_timing.py [c128 c256 c512] [--json FILE]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from vaehip import ops  # noqa: E402

SHAPES = {"c128": (16, 256, 128, 128), "c256": (16, 128, 256, 256), "c512": (16, 64, 512, 512)}
REC = 16  # uint64 per (workgroup, wave group): 10 edges, 4 phase sums over the stamped steps, their span, their number
argv = sys.argv[1:]
jout = argv.pop(argv.index("--json") + 1) if "--json" in argv else ""
argv = [a for a in argv if a != "--json"]
result = {}
for nm in (argv or list(SHAPES)):
    B, H, Ci, Co = SHAPES[nm]
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((B, H, H, Ci), device="cuda", generator=g)
    bias = torch.randn(Co, device="cuda", generator=g)
    w = (torch.randn((Co, 3, 3, Ci), device="cuda", generator=g) / math.sqrt(9 * Ci)).permute(0, 3, 1, 2)
    stamps = torch.zeros(max(8 * 3 * REC, ((B * H * H + 127) // 128) * Co // 2 + 1), device="cuda", dtype=torch.int64)
    tr = stamps.view(torch.float32)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(40):
        stamps.zero_()
        e0.record()
        ops.conv_fwd(x, w, bias, "c3", track=tr)
        e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    t = stamps[:8 * 3 * REC].cpu().numpy().reshape(8, 3, REC).astype("float64")
    print(f"{nm}: {ms:.3f} ms incl. the weight transform; {Ci // 8} steps per workgroup", flush=True)
    groups = [[] for _ in range(3)]
    for wg in range(8):
        for wv in range(3):
            v = t[wg, wv, :10]
            if v[0] == 0:
                continue
            n = max(t[wg, wv, 15], 1.0)  # stamped steps (8)
            ph1, ph2, ph3, wait = (t[wg, wv, 10 + i] / n for i in range(4))
            per = t[wg, wv, 14] / n
            groups[wv].append((per, ph1, ph2, ph3, wait, (v[2] - v[1]) / (Ci // 8), v[1] - v[0], v[7] - v[2]))
            print(f"  wg {wg} wave {4 * wv}: prologue {v[1]-v[0]:6.0f}  main loop {v[2]-v[1]:7.0f} ({(v[2]-v[1]) / (Ci // 8):5.0f}/step)  block 0: to LDS {v[3]-v[2]:5.0f} "
                  f"transform+store {v[4]-v[3]:6.0f}  block 1: to LDS {v[5]-v[4]:5.0f} transform+store {v[6]-v[5]:6.0f}  tail {v[7]-v[6]:5.0f}  total {v[7]-v[0]:7.0f}  "
                  f"clock {(v[7]-v[0])/max(v[9]-v[8],1)*0.1:5.2f} GHz | steps 2..9: {per:5.0f}/step: groups 0-1 {ph1:5.0f} groups 2-3 {ph2:5.0f} "
                  f"groups 4-5 + DMA wait {ph3:5.0f} barrier wait {wait:5.0f}", flush=True)
    result[nm] = {"ms_with_weight_transform": round(ms, 3), "steps": Ci // 8, "wave_groups": {}}
    for wv in range(3):
        if groups[wv]:
            m = np.mean(np.array(groups[wv]), axis=0)
            result[nm]["wave_groups"][f"waves {4 * wv}-{4 * wv + 3}"] = dict(zip(
                ("cycles_per_step", "groups_0_1", "groups_2_3", "groups_4_5_to_barrier", "barrier_wait", "loop_cycles_per_step", "prologue", "epilogue"),
                (int(round(float(q))) for q in m)))
            print(f"  mean over workgroups, waves {4 * wv}-{4 * wv + 3}: {result[nm]['wave_groups'][f'waves {4 * wv}-{4 * wv + 3}']}", flush=True)
if jout:
    with open(jout, "w") as f:
        json.dump(result, f, indent=1)
