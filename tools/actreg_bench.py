"""Time of the activation-penalty kernels (csrc/actreg.hip) at the benchmark shapes, 16 x 256 x 256 x 128 fp32 and 32 x 256 x 256 x
128 bf16 (537 MB each): ops.actreg_stats against ops.chanhist on the same tensor (the same bytes read, comparable work per
element), and ops.actreg_inject against ops.add at the same element count (three streams of the same bytes).  Then a train step
at 256 x 256, batch 16, fp32, with the two penalties of configs/experiment_synthetic_activation_penalty.yaml registered
against none.  Device events around each call after a warm-up, the arms alternated in one process in a seeded random order per round, median
and quartiles per arm; the results are held to the bounds of tests/actreg_refs.py on a slice before anything is timed.
    python tools/actreg_bench.py [--reps 20] [--step-reps 8] [--out profiles/actreg_measured.json]
The default step against the parent commit is bench.py's to measure: run `bench.py --gpus 1 --steps 10 --warmup 3` of a checkout
of the parent and of this tree alternately (parent first), collect the JSON result lines in a file, and
    python tools/actreg_bench.py --merge-bench LINES [--out profiles/actreg_measured.json]
records them as the file's "bench_parent_vs_new" section (needs no GPU)."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

CASES = (("fp32_16x256x256x128", (16, 256, 256, 128), torch.float32), ("bf16_32x256x256x128", (32, 256, 256, 128), torch.bfloat16))
DEFAULT_OUT = os.path.join(ROOT, "profiles", "actreg_measured.json")
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12  # bytes / s of the MI355X: the specification's, and what streaming kernels reach
TARGETS = [("vae.decoder.up_blocks.1.resnets.0", dict(kind="ceiling", threshold=0.5, weight=1.0)),
           ("vae.quant_conv", dict(kind="floor", threshold=0.3, weight=10.0, channels=(0, 3)))]  # the config's
KEPT = ("oracle", "bench_parent_vs_new")  # sections other runs write into the same file


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


def within(new, old):
    """no slower than the other arm plus the arms' own interquartile spread"""
    iqr = max(new["q3_ms"] - new["q1_ms"], old["q3_ms"] - old["q1_ms"])
    return bool(new["median_ms"] <= old["median_ms"] + iqr)


def measure(shape, dtype, reps):
    import actreg_refs as R
    from vaehip import ops
    dev = torch.device("cuda:0")
    B, H, W, Cc = shape
    torch.manual_seed(3)
    a = (torch.randn(shape, device=dev) * 0.8 + 0.3).to(dtype)
    g = (torch.randn(shape, device=dev) * 0.01).to(dtype)
    # checked on one image's first rows (the float64 reference of the whole tensor is a matter of minutes on the host)
    sl, gl = a[:1, :64].clone(memory_format=torch.contiguous_format), g[:1, :64].clone(memory_format=torch.contiguous_format)
    for kind, thr, weight in (("ceiling", 0.5, 1.0), ("floor", 0.9, 10.0)):
        st = ops.actreg_stats(sl, kind, thr, weight)
        R.check_stats(st, sl, kind, thr, weight, ops.actreg_chunks(1, 64 * W, Cc))
        R.check_inject(ops.actreg_inject(sl, gl, kind, thr, st[2]), sl, gl, kind, thr, st[2])
    coef = ops.actreg_stats(a, "ceiling", 0.5, 1.0)[2]
    arms = {"actreg_stats": lambda: ops.actreg_stats(a, "ceiling", 0.5, 1.0), "chanhist": lambda: ops.chanhist(a),
            "actreg_inject_ceiling": lambda: ops.actreg_inject(a, g, "ceiling", 0.5, coef),
            "actreg_inject_floor": lambda: ops.actreg_inject(a, g, "floor", 0.5, coef), "add": lambda: ops.add(a, g)}
    for fn in arms.values():
        for _ in range(3):
            fn()
    t = {k: [] for k in arms}
    # alternated, in a new seeded order every round: a 537 MB tensor does not fit the memory-side cache, and an arm that always
    # ran behind the same other arm would inherit that arm's cache contents and pending writes (a kernel trace showed the same
    # kernel 20 % apart between a fixed first and a fixed second place)
    rng = random.Random(0)
    for _ in range(reps):
        order = list(arms)
        rng.shuffle(order)
        for k in order:
            t[k].append(timed(arms[k]))
    nbytes = a.numel() * a.element_size()
    nch = ops.actreg_chunks(B, H * W, Cc)
    res = {"shape": list(shape), "dtype": str(dtype)[6:], "tensor_bytes": nbytes, "workgroups": B * nch * ((Cc + 255) // 256),
           "workspace_bytes": B * nch * Cc * 3 * 4}
    for k in arms:
        res[k] = spread(t[k])
    res["actreg_stats_bytes_per_s"] = round((nbytes + 2 * res["workspace_bytes"]) / (res["actreg_stats"]["median_ms"] * 1e-3), 0)
    res["chanhist_bytes_per_s"] = round(nbytes / (res["chanhist"]["median_ms"] * 1e-3), 0)
    for k in ("actreg_inject_ceiling", "actreg_inject_floor", "add"):
        res[k + "_bytes_per_s"] = round(3 * nbytes / (res[k]["median_ms"] * 1e-3), 0)
    res["memory_bound_ms_at_achievable"] = {"one_stream": round(nbytes / HBM_ACHIEVABLE * 1e3, 4), "three_streams": round(3 * nbytes / HBM_ACHIEVABLE * 1e3, 4)}
    res["ratio_stats_over_chanhist"] = round(res["actreg_stats"]["median_ms"] / res["chanhist"]["median_ms"], 3)
    res["ratio_inject_ceiling_over_add"] = round(res["actreg_inject_ceiling"]["median_ms"] / res["add"]["median_ms"], 3)
    res["ratio_inject_floor_over_add"] = round(res["actreg_inject_floor"]["median_ms"] / res["add"]["median_ms"], 3)
    res["stats_within_chanhist_plus_spread"] = within(res["actreg_stats"], res["chanhist"])
    res["inject_ceiling_within_add_plus_spread"] = within(res["actreg_inject_ceiling"], res["add"])
    res["inject_floor_within_add_plus_spread"] = within(res["actreg_inject_floor"], res["add"])
    return res


def measure_step(reps):
    """train steps at 256 x 256, batch 16, fp32: the config's two penalties registered against none, alternated"""
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip.actreg import ActivationPenalty
    from vaehip.trainer import HipTrainer
    dev = torch.device("cuda:0")
    w = SDXLVAEWrapper("synthetic:42", device=dev)
    tr = HipTrainer(w, lr=1e-5, max_grad_norm=1.0, kl_weight=1e-6, lr_warmup_steps=100, max_train_steps=1000)
    eng = w.vae.engine
    x, e = vo.synthetic_pixels(16, 256, 42).to(dev), vo.synthetic_eps(16, 256, 42).to(dev)
    for _ in range(2):
        tr.train_step(x, e)
    t = {"penalties_on": [], "penalties_off": []}
    values = []
    for _ in range(reps):
        hs = [eng.add_activation_penalty(w.get_submodule(n), ActivationPenalty(**s)) for n, s in TARGETS]
        t["penalties_on"].append(timed(lambda: values.append(tr.train_step(x, e)["activation_penalty"])))
        for h in hs:
            h.remove()
        t["penalties_off"].append(timed(lambda: tr.train_step(x, e)))
    assert all(v is not None and float(v) >= 0 for v in values)
    res = {k: spread(v) for k, v in t.items()}
    res.update(batch=16, resolution=256, dtype="float32", targets=[n for n, _ in TARGETS], first_penalty=float(values[0]),
               added_ms_median=round(res["penalties_on"]["median_ms"] - res["penalties_off"]["median_ms"], 4))
    return res


def bench_section(path):
    """bench.py result lines, parent and new alternating (parent first) -> the "bench_parent_vs_new" section"""
    runs = []
    for line in open(path):
        if line.startswith('{"metric"'):
            j = json.loads(line)
            runs.append({"build": "parent" if len(runs) % 2 == 0 else "new", "ms_per_step": j["ms_per_step"],
                         "ms_per_step_median": j["ms_per_step_median"], "images_per_s": j["value"], "loss": j["loss"],
                         "step_ms": j["step_ms"]})
    assert runs and len(runs) % 2 == 0, f"{len(runs)} result lines: expected parent / new pairs"
    med = lambda k: sorted(r["ms_per_step_median"] for r in runs if r["build"] == k)  # noqa: E731
    mid = lambda v: v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])  # noqa: E731
    return {"what": "bench.py --gpus 1 --steps 10 --warmup 3 of the parent commit's tree and library against this one, alternated "
                    "in one session on one MI355X; no penalty is registered, so no new launch happens",
            "runs": runs, "loss_bitwise_identical": len({json.dumps(r["loss"], sort_keys=True) for r in runs}) == 1,
            "median_of_medians_ms": {k: round(mid(med(k)), 3) for k in ("parent", "new")},
            "range_of_medians_ms": {k: [med(k)[0], med(k)[-1]] for k in ("parent", "new")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge-bench", default=None, help="file of bench.py result lines, parent / new alternating: record them and exit")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=8)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if a.merge_bench:
        res = json.load(open(a.out))
        res["bench_parent_vs_new"] = bench_section(a.merge_bench)
        json.dump(res, open(a.out, "w"), indent=1)
        print("bench_parent_vs_new", json.dumps({k: v for k, v in res["bench_parent_vs_new"].items() if k != "runs"}))
        return
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured on the CPU")
    res = {"gpu": torch.cuda.get_device_name(0), "reps": a.reps,
           "what": "ops.actreg_stats against ops.chanhist on the same tensor and ops.actreg_inject against ops.add at the same element "
                   "count (each call with its allocations); device events per call, arms alternated in one process, median and "
                   "quartiles; then a train step with the config's two penalties on against off"}
    brief = lambda d: {k: (v if not (isinstance(v, dict) and "ms" in v) else {x: y for x, y in v.items() if x != "ms"}) for k, v in d.items()}  # noqa: E731
    for name, shape, dtype in CASES:
        res[name] = measure(shape, dtype, a.reps)
        print(name, json.dumps(brief(res[name])), flush=True)
    if a.step_reps:
        res["train_step"] = measure_step(a.step_reps)
        print("train_step", json.dumps(brief(res["train_step"])), flush=True)
    if a.out:
        try:  # the oracle figures of tests/test_actreg_gpu.py and the bench.py comparison live in the same file: keep them
            old = json.load(open(a.out))
            res.update({k: old[k] for k in KEPT if k in old})
        except Exception:
            pass
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
