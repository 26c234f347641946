"""Time of ops.changrad (per-channel mean |g|, max |g|, gain gradient and Taylor saliency of one backward pass in one read of the
pair (output, gradient)) at the benchmark shapes: 16 x 256 x 256 x 128 with both operands fp32 (2 x 537 MB) and 32 x 256 x 256 x
128 with both bf16 (2 x 537 MB), against the torch formulas on the same device tensors (tracking.monitor.compute_grad_metrics)
and against two ops.moments passes, one per operand: the same bytes read by the streaming kernel the project already has.  Then
a train step at 256 x 256, batch 16, fp32, with the five gradient trackers of configs/experiment_synthetic_channel_grad.yaml on
against off.  Device events around each call after a warm-up, the arms alternated in one process, median and quartiles per arm;
the results are checked against the torch formulas before anything is timed.
    python tools/changrad_bench.py [--reps 20] [--step-reps 8] [--out profiles/changrad_measured.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402

CASES = (("fp32_16x256x256x128", (16, 256, 256, 128), torch.float32), ("bf16_32x256x256x128", (32, 256, 256, 128), torch.bfloat16))
DEFAULT_OUT = os.path.join(ROOT, "profiles", "changrad_measured.json")
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12  # bytes / s of the MI355X: the specification's, and what streaming kernels reach
RES = "vae.decoder.up_blocks.1.resnets.0"
TARGETS = [RES, RES + ".conv1", "vae.decoder.up_blocks.1.upsamplers.0", "vae.decoder", "vae.quant_conv"]
FOUR = ["mean_abs_gradient_per_channel", "abs_max_gradient_per_channel", "gain_gradient_per_channel", "taylor_saliency_per_channel"]


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


def measure(shape, dtype, reps):
    from tracking.monitor import compute_grad_metrics
    from vaehip import ops
    from vaehip.lib import lib
    dev = torch.device("cuda:0")
    B, H, W, Cc = shape
    torch.manual_seed(3)
    a = (torch.randn(shape, device=dev) * 0.8 + 0.3).to(dtype)
    g = (torch.randn(shape, device=dev) * 0.01).to(dtype)
    torch_arm = lambda: compute_grad_metrics(a.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2))  # noqa: E731
    sums, amax = ops.changrad(a, g)
    rs, ra = torch_arm()
    assert torch.equal(amax, ra), "max |g| differs from torch's"
    # fp32 sums of a chunk against float64 ones: (per + 2) 2^-24 of the absolute terms, which are above every |sum| here
    nch = ops.changrad_chunks(B, H * W, Cc)
    per = (H * W + nch - 1) // nch
    scale = torch.stack([rs[0], (a.double() * g.double()).abs().sum(dim=(0, 1, 2)), (a.double() * g.double()).abs().sum(dim=(0, 1, 2)) / B])
    assert bool(((sums - rs).abs() <= (per + 2) * 2.0 ** -24 * scale).all()), "sums outside the kernel's bound"
    n = ctypes.c_int64(0)
    lib.call("vae_changrad_workspace", B, H * W, Cc, nch, ctypes.byref(n))
    arms = {"changrad": lambda: ops.changrad(a, g), "two_moments": lambda: (ops.moments(a), ops.moments(g)), "torch_formulas": torch_arm}
    for fn in arms.values():
        for _ in range(3):
            fn()
    t = {k: [] for k in arms}
    for _ in range(reps):  # alternated
        for k, fn in arms.items():
            t[k].append(timed(fn))
    in_bytes = (a.numel() + g.numel()) * a.element_size()
    res = {"shape": list(shape), "dtype": str(dtype)[6:], "input_bytes": in_bytes, "workspace_bytes": n.value * 4,
           "workgroups": B * nch * ((Cc + 255) // 256), "pixels_per_chunk": per}
    for k in arms:
        res[k] = spread(t[k])
    med = res["changrad"]["median_ms"] * 1e-3
    # both operands once; the workspace once out and once back in
    res["changrad_bytes_per_s"] = round((in_bytes + 2 * n.value * 4) / med, 0)
    res["two_moments_bytes_per_s"] = round(in_bytes / (res["two_moments"]["median_ms"] * 1e-3), 0)
    res["memory_bound_ms_at_peak"] = round(in_bytes / HBM_PEAK * 1e3, 4)
    res["memory_bound_ms_at_achievable"] = round(in_bytes / HBM_ACHIEVABLE * 1e3, 4)
    res["share_of_achievable_bandwidth"] = round(res["changrad_bytes_per_s"] / HBM_ACHIEVABLE, 3)
    m = res["two_moments"]
    res["ratio_changrad_over_two_moments"] = round(res["changrad"]["median_ms"] / m["median_ms"], 3)
    res["changrad_within_two_moments_plus_spread"] = bool(res["changrad"]["median_ms"] <= m["median_ms"] + (m["q3_ms"] - m["q1_ms"]))
    return res


def measure_step(reps):
    """train steps at 256 x 256, batch 16, fp32: the five gradient trackers registered against none, alternated"""
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from vaehip.trainer import HipTrainer
    dev = torch.device("cuda:0")
    w = SDXLVAEWrapper("synthetic:42", device=dev)
    tr = HipTrainer(w, lr=1e-5, max_grad_norm=1.0, kl_weight=1e-6, lr_warmup_steps=100, max_train_steps=1000)
    x, e = vo.synthetic_pixels(16, 256, 42).to(dev), vo.synthetic_eps(16, 256, 42).to(dev)
    cfg = {"enabled": True, "track_interval": 1,
           "target_layers": [{"name": n, "capture_point": "output_grad", "metrics": FOUR} for n in TARGETS]}
    for _ in range(2):
        tr.train_step(x, e)
    t = {"trackers_on": [], "trackers_off": []}
    passes = 0
    for _ in range(reps):
        mon = ActivityMonitor(w, cfg)
        t["trackers_on"].append(timed(lambda: tr.train_step(x, e)))
        passes += sum(len(v[FOUR[0]]) for v in mon.hook_collected_buffer.values())
        mon.remove_hooks()
        t["trackers_off"].append(timed(lambda: tr.train_step(x, e)))
    assert passes == reps * len(TARGETS), passes  # every tracker fired once per step
    res = {k: spread(v) for k, v in t.items()}
    res.update(batch=16, resolution=256, dtype="float32", trackers=TARGETS,
               added_ms_median=round(res["trackers_on"]["median_ms"] - res["trackers_off"]["median_ms"], 4))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=8)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured on the CPU")
    res = {"gpu": torch.cuda.get_device_name(0), "reps": a.reps,
           "what": "ops.changrad against two ops.moments passes and the torch formulas on the same device tensors (each call: partial "
                   "pass + final pass, allocations included); device events per call, arms alternated in one process, median and "
                   "quartiles; then a train step with the five gradient trackers on against off"}
    for name, shape, dtype in CASES:
        res[name] = measure(shape, dtype, a.reps)
        print(name, json.dumps({k: (v if not isinstance(v, dict) else {x: y for x, y in v.items() if x != "ms"})
                                for k, v in res[name].items()}), flush=True)
    if a.step_reps:
        res["train_step"] = measure_step(a.step_reps)
        print("train_step", json.dumps({k: (v if not isinstance(v, dict) else {x: y for x, y in v.items() if x != "ms"})
                                        for k, v in res["train_step"].items()}), flush=True)
    if a.out:
        try:  # the oracle errors and bars of tests/test_changrad_gpu.py live in the same file: keep them
            res["oracle"] = json.load(open(a.out))["oracle"]
        except Exception:
            pass
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
