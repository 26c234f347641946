#!/usr/bin/env python
"""Throughput of the SDXL-VAE fine-tune step (fwd + loss + bwd + clip + AdamW, tracking on) on
N MI355X GPUs of one node.  One process per GPU (torch.distributed / RCCL when N > 1).

Workload at every N (weak scaling) = BASELINE.json configs[1]: SDXL-VAE, 256x256 synthetic RGB,
batch 16 per GPU, fp32, ActivityMonitor on the 3 shipped layers + classifier, no intervention.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times --steps steps, writes --dump-outputs and prints the
headline (value, ms_per_step, the per-step medians, loss, peak memory, comm when N > 1).  --full adds what takes runs of its
own, after the headline region:
  profiled_region / roofline / step_flops / kernels -- the same loop with HIP events around every launch: the dominant
                  contraction kernel's executed MFMA TFLOP/s vs the dense MFMA peak (frac <= 1) + the algorithmic
                  (direct-convolution) rate; step_flops gives the same split per step
  tracker_overhead -- trackers registered vs removed, interleaved A/B
  bf16_configs2  -- BASELINE configs[2]'s per-GPU shape in bf16 mode
  cpu_baseline   -- the CPU oracle (plain PyTorch restatement of the reference path) on a bounded sample
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

RES = 256
BATCH_PER_GPU = 16
MFMA_F32_PEAK_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md, dense fp32 matrix peak
MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16 (the 5 PF headline includes 2:1 sparsity)
TRACKING_CFG = {
    "enabled": True, "track_interval": 20,
    "target_layers": [
        {"name": "vae.encoder.conv_in", "capture_point": "output", "metrics": ["mean_abs_activation_per_channel"]},
        {"name": "vae.encoder.down_blocks.0.resnets.0.norm1", "capture_point": "output", "metrics": ["mean_abs_activation_per_channel"]},
        {"name": "vae.decoder.up_blocks.1.resnets.0.norm1", "capture_point": "output", "metrics": ["mean_abs_activation_per_channel"]},
    ],
}
CLASSIFY_CFG = {
    "enabled": True, "method": "threshold_groupnorm_activity", "threshold": 0.2,
    "target_metric_key": "mean_abs_activation_per_channel",
    "layers_to_classify": ["vae.encoder.down_blocks.0.resnets.0.norm1.output", "vae.decoder.up_blocks.1.resnets.0.norm1.output"],
}


def host_cpu_share():
    """(threads to use, description): the CPU share this process really has -- scheduler affinity capped by the cgroup CPU
    quota -- capped at 16 (the share of a one-GPU box).  torch's default (one thread per logical CPU of the HOST, 128 on the
    GPU boxes) oversubscribes that share, which is what made round 2's figure differ 2.4x between boxes."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()
            if q != "max":
                quota = max(1, int(float(q) / float(per)))
    except Exception:
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                q, per = int(f.read()), int(g.read())
                if q > 0:
                    quota = max(1, q // per)
        except Exception:
            quota = None
    phys = None
    try:
        cores = set()
        pid = cid = None
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("physical id"):
                    pid = ln.split(":")[1].strip()
                elif ln.startswith("core id"):
                    cid = ln.split(":")[1].strip()
                elif not ln.strip():
                    if pid is not None and cid is not None:
                        cores.add((pid, cid))
                    pid = cid = None
        phys = len(cores) or None
    except Exception:
        phys = None
    n = min(x for x in (aff, quota, 16) if x)
    return n, f"{n} threads (affinity {aff} logical CPUs, cgroup quota {quota if quota else 'none'}, host physical cores {phys if phys else 'unknown'}; capped at 16)"


def cpu_baseline(batch: int = 4, max_seconds: float = 55.0):
    """reference-equivalent CPU path (PyTorch oracle) on the host cores: full train steps (fwd+loss+bwd+clip+AdamW, 3 tracker
    hooks) on a bounded sample of the same workload.  Thread count fixed explicitly (host_cpu_share); one untimed warm-up
    step at the SAME shape, then timed steps while the budget lasts (at least one, at most three); every step time is
    reported and `value` comes from the fastest one (the most reproducible statistic on a shared host)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import vae_oracle as vo
    cores, how = host_cpu_share()
    prev = torch.get_num_threads()
    torch.set_num_threads(cores)
    try:
        o = vo.OracleWrapper(seed=42)
        hooks = []
        for conf in TRACKING_CFG["target_layers"]:
            mod = o.get_submodule(conf["name"])
            def hook(m, i, out):  # the reference's hook body (monitor.py:66-67); must return None
                vo.mean_abs_per_channel(out)
            hooks.append(mod.register_forward_hook(hook))
        tr = vo.OracleTrainer(o, max_steps=100)
        x, e = vo.synthetic_pixels(batch, RES, 42), vo.synthetic_eps(batch, RES, 42)
        t_begin = time.perf_counter()
        tr.step(x, e)  # warm-up at the same shape, untimed
        warm = time.perf_counter() - t_begin
        times = []
        while len(times) < 3 and (not times or (time.perf_counter() - t_begin) + min(times) < max_seconds):
            t0 = time.perf_counter()
            tr.step(x, e)
            times.append(time.perf_counter() - t0)
        for h in hooks:
            h.remove()
    finally:
        torch.set_num_threads(prev)
    best = min(times)
    return {"value": round(batch / best, 4), "unit": "images/sec", "cores": cores, "kind": "port",
            "step_seconds": [round(t, 2) for t in times], "min_step_seconds": round(best, 2), "warmup_step_seconds": round(warm, 2),
            "sample": f"{len(times)} timed full train steps at batch {batch} (config batch is {BATCH_PER_GPU}: bounded sample), value = batch / "
                      f"fastest step, after one untimed warm-up step at the same shape; 256x256, fp32, torch CPU, {how}; oracle = "
                      f"plain-PyTorch restatement of the reference diffusers path"}


def _free_port() -> int:
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch(n: int) -> int:
    """`bench.py --gpus N` without a launcher: start N ranks of this script through torch.distributed.run (one process
    per GPU, 127.0.0.1 rendezvous) BEFORE this process touches the GPU, pass their output through and return the exit
    code.  Rank 0 of the children prints the JSON line."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # the host driver supports dmabuf IPC only (RCCL needs it)
    return subprocess.run(cmd, env=env).returncode


def workload_label(dtype: str, R: int, B: int, ckpt: bool, nudge: int, tracking: bool) -> str:
    """which BASELINE.json config this run is (by shape), in words"""
    if dtype == "f32":
        idx = 1 if (R == 256 and B == 16) else None
    else:
        idx = {256: 2, 512: 3, 1024: 4}.get(R)
    head = f"BASELINE configs[{idx}]" if idx is not None else "off-baseline shape"
    prec = "fp32" if dtype == "f32" else "bf16 MFMA compute (fp32 accumulate, fp32 master weights and statistics; activations stored as bf16)"
    extra = (", decoder activation-checkpointed" if ckpt else "") + (f", gentle nudge every {nudge} steps" if nudge else ", no nudge")
    return (f"{head}: SDXL-VAE {R}x{R} synthetic RGB, batch {B}/GPU, {prec}, "
            f"tracking {'on (3 layers) + classifier' if tracking else 'off'}{extra}; random-init weights (synthetic:42)")


class Job:
    """one configured training job on this rank: wrapper + trainer + tracker / classifier (+ nudger) + resident inputs"""

    def __init__(self, dtype, B, R, dev, world, rank, *, tracking=True, act_fp32=False, checkpoint_decoder=False, nudge_interval=0,
                 one_rank_exchange=False):
        from models.sdxl_vae_wrapper import SDXLVAEWrapper
        from tracking.monitor import ActivityMonitor
        from classification.classifier import RegionClassifier
        from vaehip.trainer import HipTrainer
        from vaehip import ops
        self.ops, self.dev, self.world, self.rank, self.B, self.R, self.dtype = ops, dev, world, rank, B, R, dtype
        self.dist_on = world > 1 or one_rank_exchange  # (--rccl-selftest: the collectives of the N > 1 path on a one-rank RCCL group)
        ops.ACT_BF16 = not act_fp32
        torch.manual_seed(42)
        self.w = SDXLVAEWrapper("synthetic:42", device=dev)
        self.trainer = HipTrainer(self.w, lr=1e-5, max_grad_norm=1.0, kl_weight=1e-6, lr_warmup_steps=100,
                                  max_train_steps=10000, scheduler_steps_per_update=world,
                                  mixed_precision="bf16" if dtype == "bf16" else "no", checkpoint_decoder=checkpoint_decoder,
                                  time_comm=self.dist_on, one_rank_exchange=one_rank_exchange)
        self.monitor = ActivityMonitor(self.w, TRACKING_CFG) if tracking else None
        self.classifier = RegionClassifier(self.w.vae, CLASSIFY_CFG) if tracking else None
        self.nudger = None
        self.nudge_interval = nudge_interval
        if nudge_interval > 0 and tracking:
            from intervention.nudger import InterventionHandler
            self.nudger = InterventionHandler(self.w.vae, {"enabled": True, "strategy": "gentle_nudge_groupnorm_scale", "nudge_factor": 1.10,
                                                           "max_scale_value": 1.5, "intervention_interval": nudge_interval})
        self.track_interval = TRACKING_CFG["track_interval"] if not self.nudger else min(TRACKING_CFG["track_interval"], nudge_interval)
        if self.monitor is not None:
            self.monitor.config["track_interval"] = self.track_interval
        self.tracking_on = tracking
        gen = torch.Generator(device=dev).manual_seed(42 + rank)
        self.x = torch.rand((B, 3, R, R), device=dev, generator=gen) * 2 - 1  # resident in HBM before any timed region
        self.eps = torch.randn((B, 4, R // 8, R // 8), device=dev, generator=gen)

    def one_step(self):
        tr = self.trainer
        tr.train_step(self.x, self.eps)
        if self.monitor is not None and self.tracking_on and tr.global_step % self.track_interval == 0:
            self.monitor.step(tr.global_step)
            data = self.monitor.get_data_for_step(tr.global_step)
            if data:
                found = self.classifier.classify(data, tr.global_step)
                if self.nudger is not None and found and tr.global_step % self.nudge_interval == 0:
                    self.nudger.intervene(found, tr.global_step)  # every rank applies the same nudge to the live arena

    def timed_region(self, steps):
        """-> (wall seconds of `steps` steps: barrier + synchronize on both sides, max over ranks; this rank's per-step
        milliseconds from one event per step on the launch stream)"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        if self.dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        for i in range(steps):
            self.one_step()
            ev[i + 1].record()
        torch.cuda.synchronize()
        if self.dist_on:
            dist.barrier()
        dt = time.perf_counter() - t0
        tt = torch.tensor([dt], device=self.dev, dtype=torch.float64)
        if self.dist_on:
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item()), [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]

    def profiled_region(self, steps):
        """the same loop with ops.PROFILER installed on rank 0 -> (per-kernel summary or None, wall seconds, per-step ms)"""
        prof = None
        if self.rank == 0:
            prof = self.ops.LaunchProfiler()
            self.ops.PROFILER = prof
        try:
            dt, ms = self.timed_region(steps)
        finally:
            self.ops.PROFILER = None
        return (prof.summary() if prof is not None else None), dt, ms

    def set_tracking(self, on: bool):
        if self.monitor is None or on == self.tracking_on:
            return
        if on:
            self.monitor._register_hooks()
        else:
            self.monitor.remove_hooks()
        self.tracking_on = on

    def tracker_overhead(self, rounds=2, steps=5):
        """A/B inside one process: `rounds` x (steps with the trackers registered, steps with them removed), interleaved so
        that clock / temperature drift hits both arms; medians of the per-step event times of each arm"""
        on, off = [], []
        for _ in range(rounds):
            self.set_tracking(True)
            self.one_step()  # (one untimed step after each switch)
            on += self.timed_region(steps)[1]
            self.set_tracking(False)
            self.one_step()
            off += self.timed_region(steps)[1]
        self.set_tracking(True)
        m_on, m_off = sorted(on)[len(on) // 2], sorted(off)[len(off) // 2]
        return {"tracking_on_ms_median": round(m_on, 3), "tracking_off_ms_median": round(m_off, 3),
                "overhead_frac": round(m_on / m_off - 1.0, 5), "steps_per_arm": len(on),
                "on_ms": [round(t, 2) for t in on], "off_ms": [round(t, 2) for t in off],
                "note": "same process, same job: ActivityMonitor's fused trackers (3 layers) + classifier every track_interval steps "
                        "registered vs removed, arms interleaved; replaces the reference's host-synchronising hook (monitor.py:66-67)"}

    def comm_block(self, steps):
        tr = self.trainer
        ex = torch.tensor([tr.exposed_comm_ms() / max(steps, 1)], device=self.dev, dtype=torch.float64)
        dist.all_reduce(ex, op=dist.ReduceOp.MAX)
        return {"world_size": dist.get_world_size(), "backend": dist.get_backend() + (" (RCCL)" if dist.get_backend() == "nccl" else ""),
                "gradient_bytes_per_step": int(self.w.vae.arena.grad.numel()) * 4, "bucket_mb": tr.bucket_mb,
                "buckets": len(tr.reducer.buckets) if tr.reducer is not None else 0,
                "exposed_ms_per_step_max_over_ranks": round(float(ex.item()), 3),
                "wide_reserved_cus": self.ops.get_option("wide_reserved_cus"),
                "note": "exposed = time the compute stream waits in reducer.finish() for all-reduces the backward pass did not hide"}

    def release(self):
        if self.monitor is not None:
            self.monitor.remove_hooks()
        self.trainer = self.monitor = self.classifier = self.nudger = self.w = self.x = self.eps = None


# --dump-outputs: elements kept per output (float32); larger outputs are written as a fixed, seeded sample of this size.
# The caps add up to 40 MB; with the small outputs beside them the dump stays inside 64 MB.
DUMP_CAP = {"reconstruction": 1 << 22, "moments": 1 << 20, "latents": 1 << 20, "params": 1 << 21, "grads": 1 << 21}
DUMP_MAX_BYTES = 64 << 20
DUMP_SEED = 42


def _dump_sample(t: torch.Tensor, cap: int, seed: int):
    """float32 host copy of `t` in its logical shape when it has at most `cap` elements, else the elements of the flattened
    tensor at `cap` sorted indices drawn without replacement by a generator seeded with `seed` (the same for every run)"""
    if t.numel() <= cap:
        return t.detach().float().cpu().numpy()
    idx = np.sort(np.random.default_rng(seed).choice(t.numel(), size=cap, replace=False))
    return t.detach().reshape(-1)[torch.from_numpy(idx).to(t.device)].float().cpu().numpy()


def capture_outputs(job):
    """what a caller of the timed path holds after its last step, as float32 host arrays in the layouts the wrapper's callers
    see (NCHW activations, parameters and their .grad in named_parameters order), not the engine's internal ones: the loss
    scalars [mse, kl, total], the gradient norm, the reconstruction, the encoder moments and the sampled latents of that
    step, the updated parameters and their gradients, and the tracker statistics when the last step ran the tracker"""
    res, vae = job.trainer.last, job.w.vae
    params = [p for _, p, _, _ in vae.arena.entries]
    out = {"loss": res["scalars"].detach().float().cpu().numpy(),
           "grad_norm": job.trainer.optimizer.grad_norm().reshape(1).float().cpu().numpy()}
    for i, key in enumerate(("reconstruction", "moments", "latents")):
        out[key] = _dump_sample(res[key].permute(0, 3, 1, 2), DUMP_CAP[key], DUMP_SEED + i)
    out["params"] = _dump_sample(torch.cat([p.detach().reshape(-1) for p in params]), DUMP_CAP["params"], DUMP_SEED + 3)
    out["grads"] = _dump_sample(torch.cat([p.grad.reshape(-1) for p in params]), DUMP_CAP["grads"], DUMP_SEED + 3)  # params' indices
    if job.monitor is not None and job.tracking_on:
        for layer, metrics in job.monitor.get_data_for_step(job.trainer.global_step).items():
            for metric, v in metrics.items():
                if isinstance(v, (torch.Tensor, np.ndarray)):
                    out[f"tracker.{layer}.{metric}"] = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float32)
    assert sum(a.nbytes for a in out.values()) <= DUMP_MAX_BYTES, {k: a.nbytes for k, a in out.items()}
    return out


def write_outputs(outputs, d):
    os.makedirs(d, exist_ok=True)
    for name, arr in outputs.items():
        np.save(os.path.join(d, name + ".npy"), arr)
    return {"dir": d, "files": sorted(n + ".npy" for n in outputs), "bytes": sum(a.nbytes for a in outputs.values())}


def _pmc_file(tag):
    """HBM bytes from the committed rocprofv3 --pmc passes (separate runs of this command; offline), newest round first"""
    for tfile in (f"r04_hbm_traffic_{tag}.json", f"r03_hbm_traffic_{tag}.json"):
        try:
            with open(os.path.join(ROOT, "profiles", tfile)) as f:
                pmc = json.load(f)
            pmc["_file"] = "profiles/" + tfile
            pmc["_src"] = (f"rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE (separate passes), {pmc['_file']}, measured at commit "
                           f"{pmc.get('commit', 'unrecorded')}")
            return pmc
        except Exception:
            continue
    return None


def roofline_blocks(summ, prof_dt, prof_steps, dtype, B, R, ckpt, pmc_shape=None):
    """(roofline, step_flops, kernels) from a LaunchProfiler summary over `prof_steps` steps that took `prof_dt` seconds"""
    if summ is None:
        return None, None, {}
    tag = "f32" if dtype == "f32" else "bf16"
    pmc = _pmc_file(tag)
    want_shape = pmc_shape or (BATCH_PER_GPU, RES)
    pmc_ok = pmc is not None and (B, R) == want_shape and not ckpt
    kernels = {}
    for k, v in sorted(summ.items(), key=lambda kv: -kv[1]["ms"]):
        kernels[k] = {"launches_per_step": v["launches"] / prof_steps, "ms_per_step": round(v["ms"] / prof_steps, 3),
                      "tflops_algorithmic": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 and v["flops"] > 0 else None,
                      "tflops_executed": round(v["executed"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 and v["flops"] > 0 else None}
    contr = {k: v for k, v in summ.items() if v["flops"] > 0}
    tot_ms = sum(v["ms"] for v in contr.values())
    dom = max(contr.items(), key=lambda kv: kv[1]["ms"])
    sec = dom[1]["ms"] * 1e-3
    alg, exe = dom[1]["flops"] / sec / 1e12, dom[1]["executed"] / sec / 1e12
    traffic = None
    if pmc_ok:
        hit = pmc.get("kernels", {}).get(dom[0].replace(" ", ""))
        if hit:
            traffic = round(hit["hbm_bytes_per_launch"])
    peak = MFMA_F32_PEAK_TFLOPS if "bf16" not in dom[0] else MFMA_BF16_PEAK_TFLOPS
    # `achieved` / `frac`: the matrix work the kernel EXECUTES against the dense MFMA peak (<= 1: a utilisation).  The
    # spec's algorithmic figure (direct-convolution FLOPs of the layers / time) is kept beside it: a Winograd kernel issues
    # fewer multiplications than the direct convolution it replaces, so its algorithmic rate can exceed the peak.
    roof = {"bound": "mfma", "achieved": round(exe, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(exe / peak, 4),
            "algorithmic": round(alg, 2), "algorithmic_frac": round(alg / peak, 4),
            "traffic": traffic, "traffic_source": pmc["_src"] if traffic is not None else None,
            "algorithmic_flops_per_launch": round(dom[1]["flops"] / dom[1]["launches"]),
            "executed_flops_per_launch": round(dom[1]["executed"] / dom[1]["launches"]),
            "kernel": dom[0], "launches": dom[1]["launches"],
            "avg_launch_ms": round(dom[1]["ms"] / dom[1]["launches"], 4),
            "note": "achieved/frac = executed MFMA work of the dominant contraction kernel (HIP events on the launch stream over the "
                    "profiled region) / dense peak; algorithmic = FLOPs of the same layers as direct convolutions / the same time"}
    step_s = prof_dt / prof_steps
    fa, fe = sum(v["flops"] for v in contr.values()) / prof_steps, sum(v["executed"] for v in contr.values()) / prof_steps
    pk = MFMA_F32_PEAK_TFLOPS if dtype == "f32" else MFMA_BF16_PEAK_TFLOPS
    step_flops = {"algorithmic_tflop_per_step": round(fa / 1e12, 3), "executed_tflop_per_step": round(fe / 1e12, 3),
                  "algorithmic_tflops": round(fa / step_s / 1e12, 2), "executed_tflops": round(fe / step_s / 1e12, 2),
                  "peak": pk, "executed_frac_of_peak": round(fe / step_s / 1e12 / pk, 4),
                  "contraction_ms_per_step": round(tot_ms / prof_steps, 2),
                  "contraction_kernels_executed_tflops": round(fe * prof_steps / (tot_ms * 1e-3) / 1e12, 2),
                  "note": "whole step (all kernels, wall time of the profiled region): FLOPs of every contraction launch / step time"}
    return roof, step_flops, kernels


def hbm_block(dtype, B, R, ckpt, step_seconds):
    """step-level HBM rate (north_star: achieved HBM GB/s vs the 8 TB/s roofline) from the committed PMC passes"""
    pmc = _pmc_file("f32" if dtype == "f32" else "bf16")
    if pmc is None or (B, R) != (BATCH_PER_GPU, RES) or ckpt or not pmc.get("total_hbm_bytes_both_steps"):
        return None
    per_step = pmc["total_hbm_bytes_both_steps"] / 2.0
    gbps = per_step / step_seconds / 1e9
    return {"bytes_per_step": round(per_step), "achieved": round(gbps, 1), "peak": 8000.0, "unit": "GB/s",
            "frac": round(gbps / 8000.0, 4), "source": pmc["_src"]}


def bf16_configs2_leg(dev, world, rank, steps=10, warmup=3, profile=True, one_rank_exchange=False):
    """BASELINE configs[2]'s per-GPU shape (256x256, batch 32, bf16 MFMA compute, tracking on) timed like the headline; an
    extra key of the one JSON line, the headline fields are untouched"""
    B, R = 32, RES
    torch.cuda.reset_peak_memory_stats(dev)
    job = Job("bf16", B, R, dev, world, rank, tracking=True, one_rank_exchange=one_rank_exchange)
    for _ in range(warmup):
        job.one_step()
    if job.dist_on:
        job.trainer.exposed_comm_ms()
    dt, step_ms = job.timed_region(steps)
    comm = job.comm_block(steps) if job.dist_on else None
    sc = job.trainer.last["scalars"].cpu().tolist()
    out = None
    summ = prof_dt = None
    psteps = max(1, min(steps, 5))
    if profile:
        summ, prof_dt, _ = job.profiled_region(psteps)
    if rank == 0:
        med = sorted(step_ms)[len(step_ms) // 2]
        out = {"value": round(world * B * steps / dt, 3), "unit": "images/sec", "n_gpus": world, "steps": steps, "warmup": warmup,
               "ms_per_step": round(dt / steps * 1e3, 2), "ms_per_step_median": round(med, 2),
               "value_at_median_step": round(world * B / (med * 1e-3), 3), "dtype": "bf16",
               "workload": workload_label("bf16", R, B, False, 0, True), "global_batch": world * B,
               "loss": {"mse": sc[0], "kl": sc[1], "total": sc[2]},
               "peak_hbm_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2), "comm": comm}
        if summ is not None:
            roof, sf, kernels = roofline_blocks(summ, prof_dt, psteps, "bf16", B, R, False, pmc_shape=(-1, -1))
            out["dominant_kernel"] = {k: roof[k] for k in ("kernel", "achieved", "peak", "frac", "avg_launch_ms", "launches")}
            out["executed_frac_of_peak"] = sf["executed_frac_of_peak"]
            out["executed_tflops"] = sf["executed_tflops"]
            out["profiled_ms_per_step"] = round(prof_dt / psteps * 1e3, 2)
            out["kernels"] = {k: v for k, v in list(kernels.items())[:12]}
    job.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=BATCH_PER_GPU, help="per-GPU batch (default = BASELINE config)")
    ap.add_argument("--res", type=int, default=RES)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32",
                    help="f32 = BASELINE configs[1] (the metric); bf16 = configs[2]-style compute (bf16 MFMA, fp32 accumulate, bf16 activation storage)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline region also run the profiled region (roofline, step_flops, kernels), the tracker-overhead "
                         "A/B, the bf16 configs[2] leg and the CPU oracle baseline; a plain run prints the headline only")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle baseline")
    ap.add_argument("--act-fp32", action="store_true",
                    help="bf16 mode A/B switch: keep activations and their gradients as fp32 tensors with bf16 images beside them (round 2's "
                         "layout) instead of storing them as bf16")
    ap.add_argument("--no-tracking", action="store_true", help="A/B switch for the tracker-overhead measurement")
    ap.add_argument("--no-profile", action="store_true", help="with --full: skip the profiled region (per-kernel HIP-event timing)")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="with --full: headline (+ profiled region) only: skip the tracker-overhead A/B and the bf16 configs[2] leg")
    ap.add_argument("--nudge-interval", type=int, default=0,
                    help="InterventionHandler (gentle nudge x1.10, cap 1.5) every K steps inside the timed loop (BASELINE configs[3]: 100)")
    ap.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl", help="nccl = RCCL over xGMI (the product path)")
    ap.add_argument("--one-device", action="store_true",
                    help="rehearsal on a one-GPU box: every rank uses cuda:0 (needs --dist-backend gloo; RCCL refuses two ranks per device)")
    ap.add_argument("--rccl-selftest", action="store_true",
                    help="with --gpus 1: form a ONE-rank RCCL process group and run every collective of the N > 1 path on it (bucketed "
                         "ReduceOp.AVG all-reduces under the backward pass, barriers, the max-over-ranks reductions, the comm block): "
                         "the lines a one-GPU box otherwise never executes.  The collectives are identities; the number is not a headline")
    ap.add_argument("--rendezvous-only", action="store_true",
                    help="launch the ranks, form the process group, all-reduce one number and print it: the multi-rank "
                         "plumbing without touching a GPU (CPU test of the launcher, with --dist-backend gloo)")
    ap.add_argument("--rendezvous-fail-rank", type=int, default=-1,
                    help="with --rendezvous-only: this rank exits with status 3 after the all-reduce (CPU test: a failing child "
                         "rank must make the self-launching parent return non-zero)")
    ap.add_argument("--checkpoint-decoder", action="store_true",
                    help="training.gradient_checkpointing: decoder (BASELINE configs[4], 1024x1024): decoder segments keep only their inputs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them computed on rank 0 (loss, gradient norm, reconstruction, "
                         "moments, latents, parameters and gradients; seeded samples of the large ones, under 64 MB in all) as "
                         "DIR/<name>.npy (float32).  Inputs and weights are seeded: the same arguments give the same inputs every run")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full:  # a plain run is the headline alone: every leg that costs runs of its own is off
        args.no_profile = args.no_extra_legs = args.no_cpu_baseline = True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(self_launch(args.gpus))  # nothing has touched the GPU in this process
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if args.rendezvous_only:
        dist.init_process_group(args.dist_backend, rank=rank, world_size=world)
        t = torch.tensor([float(rank + 1)])
        if args.dist_backend == "nccl":
            torch.cuda.set_device(local_rank)
            t = t.cuda()
        dist.all_reduce(t)
        if rank == args.rendezvous_fail_rank:
            sys.exit(3)
        if rank == 0:
            print(json.dumps({"rendezvous": "ok", "world": dist.get_world_size(), "backend": dist.get_backend(),
                              "allreduce_sum": float(t.item())}))
        dist.destroy_process_group()
        return
    if args.one_device:
        if world > 1 and args.dist_backend != "gloo":
            raise SystemExit("--one-device needs --dist-backend gloo")
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    selftest = bool(args.rccl_selftest) and world == 1
    if world > 1:
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
    elif selftest:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        dist.init_process_group(args.dist_backend, rank=0, world_size=1, **({"device_id": dev} if args.dist_backend == "nccl" else {}))

    job = Job(args.dtype, args.batch, args.res, dev, world, rank, tracking=not args.no_tracking, act_fp32=args.act_fp32,
              checkpoint_decoder=args.checkpoint_decoder, nudge_interval=args.nudge_interval, one_rank_exchange=selftest)
    B, R = args.batch, args.res
    for _ in range(args.warmup):
        job.one_step()
    if job.dist_on:
        job.trainer.exposed_comm_ms()  # discard the warm-up's wait events (first-step RCCL initialisation included)

    # ---- the headline region: EXACTLY --steps steps between barrier + synchronize; one event per step (for the median), no
    # per-kernel events (those run in the profiled region below with --full, whose cost is printed next to this one)
    dt, step_ms = job.timed_region(args.steps)
    sc = job.trainer.last["scalars"].cpu().tolist()
    comm = job.comm_block(args.steps) if job.dist_on else None
    dumped = None
    if args.dump_outputs and rank == 0:  # before any further step overwrites the engine's buffers
        dumped = write_outputs(capture_outputs(job), args.dump_outputs)

    # ---- profiled region (rank 0 records two HIP events around every kernel launch, on the launch stream): roofline + kernels
    summ, prof_dt, prof_steps = None, None, 0
    if not args.no_profile:
        prof_steps = max(1, min(args.steps, 10))
        summ, prof_dt, _ = job.profiled_region(prof_steps)

    # ---- tracker overhead: the same loop with the trackers removed, interleaved with tracking on (north_star: "zero measurable overhead")
    tracker = None
    if not args.no_tracking and not args.no_extra_legs:
        tracker = job.tracker_overhead(rounds=2, steps=max(3, min(args.steps, 8)))

    peak_gib = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    label = workload_label(args.dtype, R, B, args.checkpoint_decoder, args.nudge_interval if job.nudger else 0, not args.no_tracking)
    grad_bytes = int(job.w.vae.arena.grad.numel()) * 4

    # ---- the bf16 leg (BASELINE configs[2]'s per-GPU shape: 256x256, batch 32, bf16 MFMA compute), same process, after the
    # headline: north_star's 2000 images/s on 8 GPUs is only reachable in this mode (reference src/train.py:147-154)
    bf16_leg = None
    if args.dtype == "f32" and not args.no_extra_legs and R == RES and B == BATCH_PER_GPU and not args.checkpoint_decoder:
        job.release()
        del job
        torch.cuda.empty_cache()
        try:
            bf16_leg = bf16_configs2_leg(dev, world, rank, steps=max(3, min(args.steps, 10)), warmup=max(2, min(args.warmup, 3)),
                                         profile=not args.no_profile, one_rank_exchange=selftest)
        except Exception as e:  # the headline must survive a failure of the extra leg
            bf16_leg = {"error": f"{type(e).__name__}: {e}"}

    if rank == 0:
        roof, step_flops, kernels = roofline_blocks(summ, prof_dt, prof_steps, args.dtype, B, R, args.checkpoint_decoder)
        hbm = hbm_block(args.dtype, B, R, args.checkpoint_decoder, dt / args.steps)
        cpu = None
        if not args.no_cpu_baseline and world == 1:
            cpu = cpu_baseline()
        med = float(sorted(step_ms)[len(step_ms) // 2]) if step_ms else None
        line = {
            "metric": f"images/sec SDXL-VAE train step @{R}x{R} (tracking {'off' if args.no_tracking else 'on'})",
            "value": round(world * B * args.steps / dt, 3), "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "full": args.full,
            "ms_per_step": round(dt / args.steps * 1e3, 2), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": label, "global_batch": world * B, "resolution": R, "parallelism": f"dp{world}"},
            "ms_per_step_median": round(med, 2) if med is not None else None,
            "value_at_median_step": round(world * B / (med * 1e-3), 3) if med else None,
            "step_ms": [round(t, 2) for t in step_ms],
            "timing_note": "value = N*B*steps / wall time of the whole region (barrier + synchronize on both sides, max over ranks); "
                           "ms_per_step_median = median of rank 0's per-step times from one HIP event per step on the launch stream "
                           "(SURVEY 8d asks for the median); the headline region carries no per-kernel events",
            "profiled_region": None if prof_dt is None else {
                "steps": prof_steps, "ms_per_step": round(prof_dt / prof_steps * 1e3, 2),
                "event_cost_frac": round(prof_dt / prof_steps / (dt / args.steps) - 1.0, 4),
                "note": "the same loop right after the headline region with two HIP events around every kernel launch (rank 0): "
                        "source of roofline / step_flops / kernels; event_cost_frac = its step time / the headline's - 1"},
            "loss": {"mse": sc[0], "kl": sc[1], "total": sc[2]},
            "peak_hbm_gib": peak_gib,
            "roofline": roof, "step_flops": step_flops, "hbm_step": hbm, "tracker_overhead": tracker,
            "bf16_configs2": bf16_leg, "cpu_baseline": cpu, "comm": comm, "kernels": kernels,
        }
        if dumped is not None:
            line["dump_outputs"] = dumped
        if selftest:
            line["rccl_selftest"] = "one-rank process group: the collectives of the N > 1 path ran as identities (see comm)"
        print(json.dumps(line))
    if world > 1 or selftest:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
