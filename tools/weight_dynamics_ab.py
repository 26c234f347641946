"""Time of ops.weight_dynamics (six sums and max |w| per output slice and per input slice of every default target, in one read of
the parameter, gradient and Adam-moment arenas) on the full SDXL-VAE arena with default targets and both views, against
  dead_scan       vae_dead_scan over the same tensors: the one-array streaming pass this code base already has, and
  torch_formulas  the tracker's float64 torch formulas (tracking.weightdynamics.raw_sums_torch) on the same device tensors.
Device events around each call after a warm-up, the arms alternated in one process, median and quartiles per arm; the pass is
checked against the torch formulas before anything is timed.  Bytes: the four arenas' listed tensors once, the column workspace
once out and once back in.
    python tools/weight_dynamics_ab.py [--reps 20] [--torch-reps 3] [--out profiles/weight_dynamics_measured.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "weight_dynamics_measured.json")
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12  # bytes / s of the MI355X: the specification's, and what streaming kernels reach
STEP_MS_FP32 = 154.0  # the fp32 benchmark step the 0.1 % condition refers to
HP = (0.9, 0.999, 1e-8, 7)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(v):
    s = sorted(v)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median_ms": round(q(0.5), 4), "q1_ms": round(q(0.25), 4), "q3_ms": round(q(0.75), 4), "min_ms": round(s[0], 4),
            "ms": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured on the CPU")
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.weightdynamics import WeightDynamicsTracker, adam_constants, raw_sums_torch
    from vaehip import ops
    from vaehip.lib import lib
    from vaehip.weight_table import WeightTable
    dev = torch.device("cuda:0")
    w = SDXLVAEWrapper("synthetic:42", device=dev)
    arena = w.vae.arena
    items = WeightDynamicsTracker({"enabled": True}).targets(w.vae)
    table = WeightTable(arena, items)
    gen = torch.Generator(device=dev).manual_seed(5)
    flat = arena.flat
    grad = torch.randn(flat.shape, device=dev, generator=gen) * 1e-3
    m = torch.randn(flat.shape, device=dev, generator=gen) * 1e-3
    v = (torch.randn(flat.shape, device=dev, generator=gen) * 1e-3).square() + 1e-10
    numel = sum(p.numel() for _, p in items)

    # the dead-weight scan's tables over the same tensors (tracking/deadneuron.py)
    ch = lib.query("vae_dead_scan_chunk")
    offs = [(arena.offset_of[id(p)], arena.offset_of[id(p)] + p.numel()) for _, p in items]
    seg = torch.tensor(offs, dtype=torch.int64).to(dev).view(-1)
    c0 = np.concatenate([[0], np.cumsum([max(1, -(-(e - b) // ch)) for b, e in offs])]).astype(np.int32)
    chunk0, nchunk = torch.from_numpy(c0).to(dev), int(c0[-1])
    p_ = ops._p

    def dead_scan():
        n = len(offs)
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        abssum = torch.empty(n, dtype=torch.float64, device=dev)
        pcnt = torch.empty(nchunk, dtype=torch.int64, device=dev)
        psum = torch.empty(nchunk, dtype=torch.float64, device=dev)
        lib.call("vae_dead_scan", p_(flat), p_(seg), p_(chunk0), n, nchunk, 1e-5, p_(pcnt), p_(psum), p_(counts), p_(abssum), ops._stream())
        return counts, abssum

    consts = adam_constants(*HP)
    views = [(p, [arena.view_of(t, p, arena.offset_of[id(p)]) for t in (flat, grad, m, v)]) for _, p in items]

    def torch_formulas():
        return [raw_sums_torch(*ts, consts) for _, ts in views]

    def the_pass():
        return ops.weight_dynamics(flat, grad, m, v, table, *HP)

    # the pass against the torch formulas, loosely (the tests hold it to the derived bounds): 1e-4 of each vector's largest sum
    res, ref = the_pass(), torch_formulas()
    for s, r in zip(table.slots, ref):
        for view, sl, sums, amax in (("out", table.out_slice(s), res[0], res[2]), ("in", table.in_slice(s), res[1], res[3])):
            if view in r:
                scale = r[view][0].abs().amax(dim=0).clamp_min(1e-300)
                assert bool(((sums[sl] - r[view][0]).abs() <= 1e-4 * scale).all()), (s.name, view)
                assert torch.equal(amax[sl], r[view][1]), (s.name, view)
    del ref
    arms = {"weight_dynamics": the_pass, "dead_scan": dead_scan}
    for fn in arms.values():
        for _ in range(3):
            fn()
    t = {k: [] for k in arms}
    for _ in range(a.reps):  # alternated
        for k, fn in arms.items():
            t[k].append(timed(fn))
    t["torch_formulas"] = []
    torch_formulas()
    for _ in range(a.torch_reps):
        t["torch_formulas"].append(timed(torch_formulas))
    out = {"gpu": torch.cuda.get_device_name(0), "reps": a.reps, "torch_reps": a.torch_reps,
           "what": "ops.weight_dynamics (mode w+g+m+v, partial + final pass, allocations included) on the full SDXL-VAE arena, default "
                   "targets, both views, against vae_dead_scan over the same tensors and the float64 torch formulas on the same device "
                   "tensors; device events per call, arms alternated in one process, median and quartiles",
           "parameters": len(items), "elements": numel, "out_slices": table.n_out, "in_slices": table.n_in,
           "workgroups": table.nchunk, "workspace_bytes": table.nwords * 4, "input_bytes": 4 * numel * 4}
    for k in t:
        out[k] = spread(t[k])
    med = out["weight_dynamics"]["median_ms"] * 1e-3
    ds = out["dead_scan"]["median_ms"] * 1e-3
    out["weight_dynamics_bytes_per_s"] = round((out["input_bytes"] + 2 * out["workspace_bytes"]) / med, 0)
    out["dead_scan_bytes_per_s"] = round(numel * 4 / ds, 0)
    out["memory_bound_ms_at_achievable"] = round(out["input_bytes"] / HBM_ACHIEVABLE * 1e3, 4)
    out["share_of_achievable_bandwidth"] = round(out["weight_dynamics_bytes_per_s"] / HBM_ACHIEVABLE, 3)
    out["ratio_pass_over_4_dead_scans"] = round(med / (4 * ds), 3)
    out["ratio_torch_over_pass"] = round(out["torch_formulas"]["median_ms"] * 1e-3 / med, 1)
    out["added_share_of_fp32_step_at_interval_100"] = round(med * 1e3 / 100 / STEP_MS_FP32, 6)
    out["within_0p1_percent_of_the_step"] = bool(med * 1e3 < 0.001 * STEP_MS_FP32 * 100)
    print(json.dumps({k: (x if not isinstance(x, dict) else {y: z for y, z in x.items() if y != "ms"}) for k, x in out.items()}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
