"""SDXL-VAE fine-tuning with channel-dynamics tracking on MI355X.

Drop-in for the reference entry point (reference src/train.py:100-464): same `--config_path` CLI,
same YAML keys, same output files (config.yaml, chkpt-N/, final_model/{model.safetensors,
optimizer.bin, scheduler.bin, random_states_0.pkl, vae/}, tracked_activation_stats.csv,
intervention_history.csv).  Launch one process per GPU:

    python vae-channel-dynamics_amd/src/train.py --config_path <yaml>                       # 1 GPU
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
           vae-channel-dynamics_amd/src/train.py --config_path <yaml>                       # 8 GPUs, RCCL/xGMI
    (`accelerate launch ...` sets the same RANK/WORLD_SIZE environment and works too.)

What differs from the reference, on purpose:
  * the step body (train.py:283-306) is HipTrainer.train_step: HIP kernels + RCCL bucketed gradient mean,
    no per-step host sync (the reference does 3 gathers + 3 .item() every step, train.py:292-297);
    the logging scalars are summed on the device and read once per log interval / epoch.
  * tracker statistics are averaged over ranks and classification + intervention run on EVERY rank,
    so replicas stay identical (the reference nudges rank 0 only and never re-broadcasts).
  * wandb / tensorboard are optional: when unavailable, metrics go to <output_dir>/metrics.jsonl.
  * plots are not produced (reporting only); every CSV the plots were made from is still written.
  * logit_lens.enabled draws (analysis/logit_lens.py, arithmetic in csrc/lens.hip): its layer entries may carry the
    `.full_activation_map` suffix the reference's configs document but its loop never matched.
"""
import argparse
import csv
import json
import logging
import math
import os
import pickle
import random
import re
import sys
import time

import numpy as np
import torch
import torch.distributed as dist
import yaml

from utils.config_utils import load_config
from utils.logging_utils import setup_logging
from data_utils import load_and_preprocess_dataset, create_dataloader
from models.sdxl_vae_wrapper import SDXLVAEWrapper
from tracking.monitor import ActivityMonitor
from tracking.deadneuron import DeadNeuronTracker
from tracking.weightdynamics import CSV_FIELDS as WD_CSV_FIELDS, WeightDynamicsTracker
from classification.classifier import RegionClassifier
from intervention.nudger import InterventionHandler
from vaehip.trainer import HipTrainer
from vaehip.dp import allreduce_mean_
from vaehip.losses import KINDS as LOSS_KINDS, SSIM_WINDOW, ReconLoss
from vaehip.actreg import from_mapping as penalty_from_mapping

setup_logging()
logger = logging.getLogger(__name__)

target_layer_classes = (torch.nn.Conv1d, torch.nn.Conv2d, torch.nn.Conv3d, torch.nn.Linear, torch.nn.GroupNorm)


def parse_args():
    p = argparse.ArgumentParser(description="Train/Fine-tune SDXL VAE with channel dynamics analysis.")
    p.add_argument("--config_path", type=str, required=True, help="Path to the YAML configuration file for the experiment.")
    return p.parse_args()


class MetricLogger:
    """wandb / tensorboard when importable and requested, always a JSONL file on the main process."""

    def __init__(self, report_to, output_dir, logging_dir, project, run_name, config, entity, is_main):
        self.is_main = is_main
        self.wandb = None
        self.tb = None
        self.fh = None
        if not is_main:
            return
        os.makedirs(output_dir, exist_ok=True)
        self.fh = open(os.path.join(output_dir, "metrics.jsonl"), "a")
        if report_to in ("wandb", "all"):
            try:
                import wandb
                wandb.init(project=project, name=run_name, config=config, dir=output_dir, entity=entity)
                self.wandb = wandb
            except Exception as e:
                logger.error(f"W&B init failed: {e}. No W&B logging.")
        if report_to in ("tensorboard", "all"):
            try:
                from torch.utils.tensorboard import SummaryWriter
                self.tb = SummaryWriter(logging_dir)
            except Exception as e:
                logger.warning(f"tensorboard unavailable ({e}); metrics.jsonl only.")

    def log(self, metrics: dict, step: int):
        if not self.is_main:
            return
        clean = {k: (float(v) if isinstance(v, (int, float, np.floating, np.integer)) else v) for k, v in metrics.items()}
        self.fh.write(json.dumps({"step": step, **clean}) + "\n")
        self.fh.flush()
        if self.wandb is not None:
            self.wandb.log(clean, step=step)
        if self.tb is not None:
            for k, v in clean.items():
                if isinstance(v, float):
                    self.tb.add_scalar(k, v, step)

    def close(self):
        if self.fh:
            self.fh.close()
        if self.wandb is not None:
            self.wandb.finish()
        if self.tb is not None:
            self.tb.close()


def with_last(iterable):
    """yields (item, is_last): accelerate's dataloader wrapper knows the end of a pass one batch ahead
    (gradient_state.end_of_dataloader), which is what forces an optimizer update on a partial accumulation window"""
    it = iter(iterable)
    try:
        prev = next(it)
    except StopIteration:
        return
    for cur in it:
        yield prev, False
        prev = cur
    yield prev, True


_CTRL_GROUP = None


def all_ranks_ok(ok: bool, world: int) -> bool:
    """control-plane agreement on a host flag (MIN over ranks) through a gloo group: a rank whose batch failed to
    decode must not leave its peers alone in the gradient exchange.  CPU tensors, so no device synchronisation."""
    global _CTRL_GROUP
    if world <= 1:
        return ok
    if _CTRL_GROUP is None:
        _CTRL_GROUP = dist.new_group(backend="gloo")
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=_CTRL_GROUP)
    return bool(flag.item())


def agreed_batches(loader, world: int):
    """yields (batch, every rank's batch is valid, last of the pass).  The agreement on batch k+1 (all_ranks_ok's int32 MIN
    all-reduce on the gloo control group) is STARTED when the look-ahead of `with_last` fetches that batch and awaited one step
    later, so it runs behind batch k's host work instead of in front of every step (blocking: 0.36 ms per call at 2 ranks,
    0.9 ms at 8 on an 8-core host, tools/ctrl_allreduce_cost.py).  Every rank issues the same collectives in the same order."""
    global _CTRL_GROUP

    def start(b):
        ok = valid_batch(b)
        if world <= 1:
            return ok, None, None
        global _CTRL_GROUP
        if _CTRL_GROUP is None:
            _CTRL_GROUP = dist.new_group(backend="gloo")
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
        return ok, flag, dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=_CTRL_GROUP, async_op=True)

    def finish(tok):
        ok, flag, work = tok
        if work is None:
            return ok
        work.wait()
        return bool(flag.item())

    it = iter(loader)
    try:
        cur = next(it)
    except StopIteration:
        return
    tok = ntok = start(cur)
    try:
        for nxt in it:
            ntok = start(nxt)
            yield cur, finish(tok), False
            cur, tok = nxt, ntok
        yield cur, finish(tok), True
    finally:  # a consumer that stops early (max_train_steps) leaves one look-ahead all-reduce in flight: complete it here,
        if ntok is not None and ntok[2] is not None:  # before the caller's barrier / destroy_process_group
            ntok[2].wait()


def valid_batch(batch) -> bool:
    pv = batch.get("pixel_values") if batch else None  # guards the reference's None-batch crash (data_utils.py:215)
    return pv is not None and pv.ndim == 4 and pv.shape[0] > 0


STATE_FILES = ("model.safetensors", "optimizer.bin", "scheduler.bin", "trainer_state.bin")


def save_state(path: str, wrapper, trainer, rank: int = 0):
    """file layout of accelerate.save_state (accelerate/utils/constants.py:20-31) used by train.py:358-362,392-405, plus
    trainer_state.bin: what a restart needs beside those (step counters, the gradient sum of a pending accumulation window,
    the generator).  With training.use_ema the weight average rides in optimizer.bin."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    sd = {k: v.detach().cpu().contiguous() for k, v in wrapper.state_dict().items()}
    save_file(sd, os.path.join(path, "model.safetensors"), metadata={"format": "pt"})
    tsd = trainer.state_dict()
    torch.save(tsd.pop("optimizer"), os.path.join(path, "optimizer.bin"))
    torch.save(tsd.pop("lr_scheduler"), os.path.join(path, "scheduler.bin"))
    torch.save(tsd, os.path.join(path, "trainer_state.bin"))
    states = {"step": trainer.global_step, "random_state": random.getstate(), "numpy_random_seed": np.random.get_state(),
              "torch_manual_seed": torch.get_rng_state(),
              "torch_cuda_manual_seed": torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None}
    with open(os.path.join(path, f"random_states_{rank}.pkl"), "wb") as f:
        pickle.dump(states, f)


def load_state(path: str, wrapper, trainer, rank: int = 0) -> int:
    """restores what save_state wrote: the model into the arena, the trainer state (optimizer with its weight average,
    scheduler, step counters, pending gradient sum, generator) and the Python / numpy / torch / torch.cuda RNG states of
    random_states_<rank>.pkl (a rank without a file of its own keeps its RNG).  Returns the optimizer step to continue from.

    Not restored: in a one-process run the order of the resumed epoch is a fresh shuffle (the RandomSampler draws from the
    torch RNG when the iterator is made), and the in-memory histories of ActivityMonitor and DeadNeuronTracker cover only
    the steps since the resume."""
    from safetensors.torch import load_file
    missing = [n for n in STATE_FILES if not os.path.isfile(os.path.join(path, n))]
    if missing:
        raise FileNotFoundError(f"{path} is not a training state written by save_state: missing {', '.join(missing)}")
    wrapper.load_state_dict(load_file(os.path.join(path, "model.safetensors")))
    tsd = torch.load(os.path.join(path, "trainer_state.bin"), map_location="cpu", weights_only=False)
    tsd["optimizer"] = torch.load(os.path.join(path, "optimizer.bin"), map_location="cpu", weights_only=False)
    tsd["lr_scheduler"] = torch.load(os.path.join(path, "scheduler.bin"), map_location="cpu", weights_only=False)
    trainer.load_state_dict(tsd)
    rpath = os.path.join(path, f"random_states_{rank}.pkl")
    if os.path.isfile(rpath):
        with open(rpath, "rb") as f:
            states = pickle.load(f)
        random.setstate(states["random_state"])
        np.random.set_state(states["numpy_random_seed"])
        torch.set_rng_state(states["torch_manual_seed"])
        if states.get("torch_cuda_manual_seed") is not None and torch.cuda.is_available():
            torch.cuda.set_rng_state_all(states["torch_cuda_manual_seed"])
    else:
        logger.warning(f"{rpath} not found: rank {rank} keeps its RNG state")
    return trainer.global_step


def ema_settings(training_cfg: dict):
    """training.use_ema / training.ema_decay (not keys of the reference) -> (use_ema, ema_decay)"""
    decay = float(training_cfg.get("ema_decay", 0.9999))
    if not 0.0 < decay < 1.0:
        raise ValueError(f"training.ema_decay={decay!r}: must lie in (0, 1)")
    return bool(training_cfg.get("use_ema", False)), decay


def recon_loss_settings(training_cfg: dict, resolution=None) -> ReconLoss:
    """training.reconstruction_loss (mse | l1 | huber), training.huber_delta, training.ssim_weight (not keys of the reference) ->
    the spec of vaehip.losses; the defaults (`mse`, weight 0) are the default spec, the reference's loss.  `resolution`:
    data.resolution, which an SSIM term needs to be at least its window."""
    kind = training_cfg.get("reconstruction_loss", "mse")
    if not isinstance(kind, str) or kind not in LOSS_KINDS:
        raise ValueError(f"training.reconstruction_loss={kind!r}: expected one of {', '.join(LOSS_KINDS)}")

    def number(key, default):
        v = training_cfg.get(key, default)
        try:
            if isinstance(v, bool):
                raise TypeError
            return float(v)  # YAML reads 1e-1 as a string
        except (TypeError, ValueError):
            raise ValueError(f"training.{key}={v!r}: expected a number") from None
    delta, weight = number("huber_delta", 1.0), number("ssim_weight", 0.0)
    if not 0.0 < delta < float("inf"):
        raise ValueError(f"training.huber_delta={delta!r}: must be a finite number > 0")
    if not 0.0 <= weight < float("inf"):
        raise ValueError(f"training.ssim_weight={weight!r}: must be a finite number >= 0")
    if weight > 0.0 and resolution is not None and int(resolution) < SSIM_WINDOW:
        raise ValueError(f"training.ssim_weight={weight!r} with data.resolution={resolution!r}: the SSIM window is "
                         f"{SSIM_WINDOW} x {SSIM_WINDOW} pixels and images must be at least that large")
    return ReconLoss(kind=kind, huber_delta=delta if kind == "huber" else 1.0, ssim_weight=weight)


AP_CSV_FIELDS = ("step", "name", "kind", "penalty", "elements_over_threshold", "channels_under_floor")


def activation_penalty_settings(config: dict):
    """the YAML section `activation_penalty:` (not a section of the reference) -> the `activation_penalties` argument of
    HipTrainer, a list of (module name, vaehip.actreg.ActivationPenalty); [] when the section is absent or not enabled.
    `targets:` entries: name (as a tracking.target_layers name), kind (ceiling | floor), threshold, weight (default 1.0) and
    channels (optional list).  A bad entry is refused with its position and name."""
    sec = config.get("activation_penalty") or {}
    if not isinstance(sec, dict):
        raise ValueError(f"activation_penalty={sec!r}: expected a section with `enabled` and `targets`")
    if not sec.get("enabled", False):
        return []
    targets = sec.get("targets")
    if not isinstance(targets, (list, tuple)) or not targets:
        raise ValueError(f"activation_penalty.targets={targets!r}: expected a non-empty list of targets")
    out = []
    for i, entry in enumerate(targets):
        where = f"activation_penalty.targets[{i}]"
        if not isinstance(entry, dict):
            raise ValueError(f"{where}={entry!r}: expected a mapping with name, kind, threshold")
        name = entry.get("name")
        if not isinstance(name, str) or not name:
            raise ValueError(f"{where}: `name` is missing")
        rest = {k: v for k, v in entry.items() if k != "name"}
        for key in ("threshold", "weight"):  # YAML reads 1e-1 as a string
            if isinstance(rest.get(key), str):
                try:
                    rest[key] = float(rest[key])
                except ValueError:
                    raise ValueError(f"{where} ({name}): {key}={rest[key]!r}: expected a number") from None
        try:
            out.append((name, penalty_from_mapping(rest)))
        except ValueError as e:
            raise ValueError(f"{where} ({name}): {e}") from None
    return out


def trainable_setting(training_cfg: dict):
    """training.trainable_modules (not a key of the reference) -> the `trainable` argument of HipTrainer: absent or 'all' trains
    everything, 'decoder' / 'encoder' are the shorthands of vaehip.trainable, a list holds module-name prefixes of the VAE"""
    v = training_cfg.get("trainable_modules", "all")
    if v is None:
        return "all"
    if isinstance(v, str):
        return v
    if isinstance(v, (list, tuple)) and all(isinstance(x, str) for x in v):
        return [x[4:] if x.startswith("vae.") else x for x in v]  # the tracking keys of the YAMLs carry the wrapper's `vae.`
    raise ValueError(f"training.trainable_modules={v!r}: expected 'all', 'decoder', 'encoder' or a list of module-name prefixes")


def resolve_resume(resume, output_dir: str, prefix: str = "chkpt"):
    """training.resume_from_checkpoint -> directory to load, or None to start fresh.  "latest": the highest-numbered
    <prefix>-<step> directory under the run's output_dir (None when there is none); a path: that directory itself."""
    if not resume:
        return None
    if resume != "latest":
        return str(resume)
    best, best_step = None, -1
    if os.path.isdir(output_dir):
        for name in os.listdir(output_dir):
            m = re.fullmatch(re.escape(prefix) + r"-(\d+)", name)
            if m and os.path.isdir(os.path.join(output_dir, name)) and int(m.group(1)) > best_step:
                best, best_step = os.path.join(output_dir, name), int(m.group(1))
    return best


def lens_activations(entries, step_data: dict) -> dict:
    """the full activation maps a logit_lens layer list names, by monitor layer id.  An entry is a monitor layer id
    (`vae.<module>.<input|output>`) or that id followed by `.full_activation_map`, the form the reference's base_config.yaml
    documents and its own loop never matched; an entry without data for the step is reported and left out"""
    acts = {}
    for entry in entries:
        layer_id = entry[:-len(".full_activation_map")] if entry.endswith(".full_activation_map") else entry
        fmap = (step_data.get(layer_id) or {}).get("full_activation_map")
        if fmap is None:
            logger.warning(f"LogitLens: no full_activation_map for '{entry}' in the tracked data of this step. Skipping.")
            continue
        acts[layer_id] = fmap
    return acts


def run_logit_lens(lens, ll_cfg: dict, step_data: dict, global_step: int):
    """channel maps (always) and mini-decoder projections (logit_lens.run_mini_decoder_projection) of the step's tracked maps"""
    if not step_data:
        logger.warning(f"LogitLens: No activation data for step {global_step}.")
        return
    entries = ll_cfg.get("layers_to_analyze_direct") or ll_cfg.get("target_tracked_metrics") or []
    acts = lens_activations(entries, step_data)
    n_samples = ll_cfg.get("num_batch_samples_to_viz", 1)
    for layer_id, fmap in acts.items():
        lens.visualize_channel_activation_maps(fmap, layer_id, global_step, num_channels_to_viz=ll_cfg.get("num_channels_to_viz"),
                                               num_batch_samples_to_viz=n_samples, colormap=ll_cfg.get("colormap", "viridis"))
    if acts and ll_cfg.get("run_mini_decoder_projection", True):
        lens.run_logit_lens_with_activations(global_step=global_step, layers_to_analyze=list(acts), num_batch_samples_to_viz=n_samples,
                                             projection_type=ll_cfg.get("projection_type", "mini_decoder_single_channel"),
                                             activations_to_process=acts)


def run_validation(trainer: HipTrainer, val_dataloader, kl_weight: float, global_step: int, mlog: MetricLogger, device, world: int):
    """train.py:53-97: eval forward with mode(), SUM-reduced MSE and kl().sum(), per-sample averages.
    Hooks/trackers stay attached, so validation forwards enter the monitor buffer exactly as in the reference.
    With training.use_ema the pass runs a second time on the averaged weights and logs the same keys under validation_ema/."""
    m = _validation_pass(trainer, val_dataloader, kl_weight, global_step, mlog, device, world, "validation")
    if trainer.optimizer.use_ema:
        with trainer.ema_weights():
            _validation_pass(trainer, val_dataloader, kl_weight, global_step, mlog, device, world, "validation_ema")
    return m


def _validation_pass(trainer, val_dataloader, kl_weight, global_step, mlog, device, world, prefix):
    logger.info(f"--- Running Validation for Global Step: {global_step}{' (EMA weights)' if prefix != 'validation' else ''} ---")
    trainer.wrapper.eval()
    sums = torch.zeros(3, device=device, dtype=torch.float64)  # rec_sum, kl_sum, samples
    for batch, ok_everywhere, _ in agreed_batches(val_dataloader, world):
        if not ok_everywhere:  # every rank skips together (tracker buffers stay aligned)
            logger.warning("Validation: Invalid batch data, skipping.")
            continue
        pv = batch["pixel_values"]
        r = trainer.eval_step(pv.to(device, dtype=torch.float32, non_blocking=True))
        sums[0] += r["rec_sum"].double()
        sums[1] += r["kl_sum"].double()
        sums[2] += pv.shape[0]
    if world > 1:
        dist.all_reduce(sums)
    rec_sum, kl_sum, n = sums.tolist()
    avg_rec = rec_sum / n if n > 0 else 0
    avg_kl = kl_sum / n if n > 0 else 0
    avg = avg_rec + kl_weight * avg_kl
    logger.info(f"  Avg Validation Loss (Total): {avg:.4e}, Rec: {avg_rec:.4e}, KL: {avg_kl:.4e}; validated on {int(n)} samples.")
    m = {f"{prefix}/avg_total_loss": avg, f"{prefix}/avg_reconstruction_loss": avg_rec, f"{prefix}/avg_kl_divergence": avg_kl}
    mlog.log(m, global_step)
    trainer.wrapper.train()
    return m


def main():
    args = parse_args()
    config = load_config(args.config_path)
    run_name = config.get("run_name", "vae_run")
    threshold_dn = float(config.get("threshold", 1e-8))
    mean_percentage_dn = float(config.get("mean_percentage", .01))
    dead_type_dn = config.get("dead_type", "threshold")
    output_dir = os.path.join(config.get("output_dir", "./results"), run_name)
    logging_dir = os.path.join(output_dir, "logs")
    logging_cfg = config.get("logging", {})
    report_to = logging_cfg.get("report_to", "tensorboard")
    training_cfg = config.get("training", {})
    mixed_precision = training_cfg.get("mixed_precision", "no")
    if mixed_precision not in ("no", "bf16"):
        raise NotImplementedError(f"training.mixed_precision={mixed_precision!r}: this path has 'no' (exact fp32 MFMA) and "
                                  "'bf16' (bf16 MFMA products, fp32 accumulate, fp32 master weights and statistics)")
    grad_accum = int(training_cfg.get("gradient_accumulation_steps", 1))
    # not a key of the reference's YAMLs (it never checkpoints): "decoder" re-runs the decoder forward before its backward
    # instead of keeping its activations (BASELINE config 5)
    grad_ckpt = training_cfg.get("gradient_checkpointing", False)
    if grad_ckpt not in (False, None, "decoder", True):
        raise NotImplementedError(f"training.gradient_checkpointing={grad_ckpt!r}: only 'decoder' exists")
    # not keys of the reference either: a fused fp32 average of the weights, and continuing from a state save_state wrote
    use_ema, ema_decay = ema_settings(training_cfg)
    resume = training_cfg.get("resume_from_checkpoint", None)
    # not a key of the reference: which parameters train ('all', 'decoder', 'encoder' or module-name prefixes); the rest is frozen
    trainable = trainable_setting(training_cfg)
    # not keys of the reference: the pixel term (mse | l1 | huber) and an SSIM term of the training loss; validation and
    # evaluate.py keep the reference's MSE, so runs stay comparable
    recon_loss = recon_loss_settings(training_cfg, config.get("data", {}).get("resolution", 256))
    # not a section of the reference: loss terms on module outputs (an outlier ceiling, a channel floor), vaehip/actreg.py
    penalties = activation_penalty_settings(config)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: this trainer runs on MI355X only (no CPU fallback)")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("nccl", device_id=device)
    is_main = rank == 0
    logger.info(f"rank {rank}/{world} on {device}; running experiment: {run_name}")
    if config.get("seed") is not None:
        seed = int(config["seed"])
        random.seed(seed); np.random.seed(seed); torch.manual_seed(seed); torch.cuda.manual_seed_all(seed)
    if is_main:
        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, "config.yaml"), "w") as f:
            yaml.dump(config, f, default_flow_style=False)
    mlog = MetricLogger(report_to, output_dir, logging_dir, config.get("project_name", "vae_project"), run_name, config,
                        logging_cfg.get("entity", None), is_main)
    if world > 1:
        dist.barrier()

    model_cfg = config.get("model", {})
    # parameters stay fp32 in every mode (the reference casts them to bf16 when mixed_precision is bf16,
    # train.py:147-154: no master copy -- SURVEY 3.4; here bf16 is a compute mode only)
    vae_wrapper = SDXLVAEWrapper(pretrained_model_name_or_path=model_cfg.get("pretrained_vae_name", "stabilityai/sdxl-vae"),
                                 torch_dtype=None, device=device)
    data_cfg = config.get("data", {})
    bs = data_cfg.get("batch_size", 4)
    # data.gpu_preprocess (not a key of the reference): workers only decode; Resize / CenterCrop / Normalize run on the GPU
    gpu_pre = None
    if data_cfg.get("gpu_preprocess", False):
        from vaehip.preprocess import GpuPreprocessor
        gpu_pre = GpuPreprocessor(data_cfg.get("resolution", 256), device)
    train_dataset = load_and_preprocess_dataset(
        gpu_preprocess=gpu_pre is not None,
        dataset_name=data_cfg.get("dataset_name"), dataset_config_name=data_cfg.get("dataset_config_name", None),
        image_column=data_cfg.get("image_column", "image"), resolution=data_cfg.get("resolution", 256),
        max_samples=data_cfg.get("max_samples", None), split=data_cfg.get("train_split_name", "train"))
    train_dataloader = create_dataloader(train_dataset, batch_size=bs, num_workers=data_cfg.get("num_workers", 0),
                                         shuffle=True, rank=rank, world_size=world, seed=int(config.get("seed") or 0),
                                         gpu_preprocess=gpu_pre)
    val_dataloader = None
    if data_cfg.get("do_validation", False):
        try:
            vds = load_and_preprocess_dataset(
                gpu_preprocess=gpu_pre is not None,
                dataset_name=data_cfg.get("validation_dataset_name", data_cfg.get("dataset_name")),
                dataset_config_name=data_cfg.get("validation_dataset_config_name", data_cfg.get("dataset_config_name", None)),
                image_column=data_cfg.get("image_column", "image"), resolution=data_cfg.get("resolution", 256),
                max_samples=data_cfg.get("validation_max_samples", None), split=data_cfg.get("validation_split_name", "validation"))
            val_dataloader = create_dataloader(vds, batch_size=data_cfg.get("validation_batch_size", bs),
                                               num_workers=data_cfg.get("num_workers", 0), shuffle=False, rank=rank, world_size=world,
                                               gpu_preprocess=gpu_pre)
        except Exception as e:
            logger.error(f"Failed to load validation data: {e}. Disabling validation.")
            data_cfg["do_validation"] = False

    # schedule arithmetic exactly as train.py:188-195 (max_train_steps ignores the world size)
    n_train = len(train_dataset) if hasattr(train_dataset, "__len__") else None
    steps_per_epoch = math.ceil(n_train / bs / grad_accum) if n_train else training_cfg.get("max_steps_per_epoch_iterable", 10000)
    num_train_epochs = int(training_cfg.get("num_train_epochs", 1))
    max_train_steps = num_train_epochs * steps_per_epoch
    kl_weight = float(training_cfg.get("kl_weight", 1e-6))
    max_grad_norm = float(training_cfg.get("max_grad_norm", 1.0))
    trainer = HipTrainer(
        vae_wrapper, lr=float(training_cfg.get("learning_rate", 1e-5)),
        betas=(training_cfg.get("adam_beta1", 0.9), training_cfg.get("adam_beta2", 0.999)),
        eps=training_cfg.get("adam_epsilon", 1e-08), weight_decay=training_cfg.get("adam_weight_decay", 1e-2),
        max_grad_norm=max_grad_norm, kl_weight=kl_weight, lr_warmup_steps=int(training_cfg.get("lr_warmup_steps", 100)),
        max_train_steps=max_train_steps, scheduler_steps_per_update=world,  # accelerate steps the scheduler `world` times
        mixed_precision=mixed_precision, gradient_accumulation_steps=grad_accum, checkpoint_decoder=bool(grad_ckpt),
        use_ema=use_ema, ema_decay=ema_decay, trainable=trainable, recon_loss=recon_loss, activation_penalties=penalties)
    if penalties:
        logger.info("activation penalties: " + "; ".join(f"{n}: {p.kind} {p.threshold:g} x {p.weight:g}" for n, p in penalties))
    n_tr = sum(p.numel() for p in vae_wrapper.vae.parameters() if p.requires_grad)
    logger.info(f"trainable_modules={trainable!r}: {n_tr} of {sum(p.numel() for p in vae_wrapper.vae.parameters())} parameters train, "
                f"in {len(trainer.trainable_ranges)} arena range(s)")

    core_vae = vae_wrapper.vae
    dnt_cfg = config.get("dead_neuron_tracking", {})
    dnt = DeadNeuronTracker(target_layer_classes, dnt_cfg.get("target_layer_names_for_raw_weights", []), threshold_dn,
                            mean_percentage_dn, dead_type_dn) if dnt_cfg.get("enabled", False) else None
    wd_cfg = config.get("weight_dynamics", {}) or {}
    # main rank only and no collective: after the gradient all-reduce every rank holds the same four arenas
    wdt = WeightDynamicsTracker(wd_cfg) if wd_cfg.get("enabled", False) and is_main else None
    monitor_cfg = config.get("tracking", {})
    monitor = ActivityMonitor(vae_wrapper, monitor_cfg) if monitor_cfg.get("enabled", False) else None
    cls_cfg = config.get("classification", {})
    classifier = RegionClassifier(model=core_vae, config=cls_cfg) if cls_cfg.get("enabled", False) else None
    int_cfg = config.get("intervention", {})
    intervention = InterventionHandler(model=core_vae, config=int_cfg) if int_cfg.get("enabled", False) else None
    ll_cfg = config.get("logit_lens", {}) or {}
    lens = None
    if ll_cfg.get("enabled", False) and is_main:
        from analysis.logit_lens import VAELogitLens
        lens = VAELogitLens(model_for_lens=core_vae, logit_lens_config=ll_cfg, main_experiment_output_dir=output_dir)
    logger.info("VAELogitLens initialized for main process." if lens else "VAELogitLens disabled or not main process.")
    lens_interval = int(ll_cfg.get("visualization_interval", 1000)) if lens else -1

    log_interval = int(logging_cfg.get("log_interval", 10))
    save_interval = int(config.get("saving", {}).get("save_interval_steps", 500))
    ckpt_prefix = config.get("saving", {}).get("checkpoint_dir_prefix", "chkpt")
    track_interval = int(monitor_cfg.get("track_interval", 100)) if monitor else -1
    dnt_interval = int(dnt_cfg.get("track_interval", 100)) if dnt else -1
    val_epochs = int(training_cfg.get("validation_epochs", 0))
    val_steps = int(training_cfg.get("validation_steps", 0))

    logger.info(f"***** Running training: {num_train_epochs} epochs x {steps_per_epoch} steps, batch {bs}/GPU x {world} GPU *****")
    global_step = 0
    resume_dir = resolve_resume(resume, output_dir, ckpt_prefix)
    if resume_dir is not None:
        global_step = load_state(resume_dir, vae_wrapper, trainer, rank)
        logger.info(f"Resumed from {resume_dir}: continuing after optimizer step {global_step}")
    elif resume:
        logger.info(f"resume_from_checkpoint: {resume}: no {ckpt_prefix}-<step> under {output_dir}, starting fresh")
    first_epoch = global_step // steps_per_epoch
    # batches of the resumed epoch that the saved updates (and a pending accumulation window) consumed
    skip_batches = (global_step % steps_per_epoch) * grad_accum + trainer.pending_micro_batches
    step0 = global_step
    t_start = time.time()
    for epoch in range(first_epoch, num_train_epochs):
        vae_wrapper.train()
        if hasattr(train_dataloader.sampler, "set_epoch"):
            train_dataloader.sampler.set_epoch(epoch)
        epoch_sums = torch.zeros(3, device=device, dtype=torch.float64)  # mse, kl, total (this rank)
        steps_in_epoch = 0
        sc = torch.zeros(3, device=device)
        res = None
        for batch, ok_everywhere, last_batch in agreed_batches(train_dataloader, world):
            if skip_batches > 0:
                skip_batches -= 1
                continue
            if not ok_everywhere:  # all ranks skip the batch, or none does
                if last_batch and trainer.pending_micro_batches:
                    trainer.flush()  # the pass ends on a skipped batch: update with what has accumulated
                else:
                    continue
            else:
                pv = batch["pixel_values"]
                # the last batch of a pass always ends in an optimizer update (accelerate.accumulate, train.py:286)
                res = trainer.train_step(pv.to(device, dtype=torch.float32, non_blocking=True), end_of_dataloader=last_batch)
                sc = res["scalars"]
                epoch_sums += sc.double()
                steps_in_epoch += 1
            if not trainer.sync_gradients:  # micro-batch of an accumulated update (train.py:286,300)
                continue
            global_step += 1
            # after the update, before any intervention of this step: lr * u is the Adam part of the update just applied
            if wdt and global_step % wdt.track_interval == 0:
                mlog.log(wdt.track(core_vae, trainer.optimizer, global_step), global_step)
            activity_logs = {}
            if monitor and global_step % track_interval == 0:
                activity_logs = monitor.step(global_step)
            classification = {}
            if classifier and monitor and global_step % track_interval == 0:
                tracked = monitor.get_data_for_step(global_step)
                if tracked:
                    classification = classifier.classify(tracked, global_step)
                if not classification:
                    logger.info(f"Step {global_step}: Classifier found no inactive channels.")
            if lens and global_step % lens_interval == 0:
                run_logit_lens(lens, ll_cfg, monitor.get_data_for_step(global_step) if monitor else {}, global_step)
            if intervention and global_step % int_cfg.get("intervention_interval", 200) == 0:
                if classification:
                    intervention.intervene(classification, global_step)
                    inactive_total = sum(len(v["inactive_channel_indices"]) for v in classification.values())
                    nudged = intervention.num_nudges_applied
                    mlog.log({"inactive_channels": inactive_total, "nudged_scales": nudged}, global_step)
                    if is_main:
                        with open(os.path.join(output_dir, "intervention_history.csv"), "a") as fh:
                            fh.write(f"{global_step},{inactive_total},{nudged}\n")
                else:
                    logger.info(f"Step {global_step}: Intervention due, but no regions classified.")
            if global_step % log_interval == 0:
                # device values of the last micro-batch of the main rank, read behind the sync
                ap = trainer.activation_penalty_report() if is_main else None
                step_loss = allreduce_mean_(sc[2:3].clone()).item()  # the only host sync of a logging step
                if is_main:
                    loss_logs = {}
                    if ap is not None:
                        rows = ap.tolist()
                        loss_logs["train/activation_penalty"] = math.fsum(r[0] for r in rows)
                        new_file = not os.path.exists(os.path.join(output_dir, "activation_penalty_history.csv"))
                        with open(os.path.join(output_dir, "activation_penalty_history.csv"), "a", newline="") as fh:
                            wr = csv.writer(fh)
                            if new_file:
                                wr.writerow(AP_CSV_FIELDS)
                            for (name, handle), (value, over, under) in zip(trainer.activation_penalties, rows):
                                loss_logs[f"train/activation_penalty/{name}"] = value
                                wr.writerow([global_step, name, handle.spec.kind, repr(value), int(over) if over == over else "",
                                             int(under) if under == under else ""])
                    if res is not None and not recon_loss.is_default:  # this rank's terms of the last micro-batch (ssim: with an SSIM term only)
                        terms = res["loss_terms"].tolist()
                        loss_logs["train/pixel_loss"] = terms[0]
                        if recon_loss.ssim_weight > 0:
                            loss_logs["train/ssim"] = terms[1]
                    mlog.log({"train_loss_step": step_loss, "lr": trainer.lr_scheduler.get_last_lr()[0], "epoch_current": epoch,
                              **loss_logs, **activity_logs}, global_step)
                    logger.info(f"step {global_step}/{max_train_steps} loss {step_loss:.4e} lr {trainer.lr_scheduler.get_last_lr()[0]:.3e} "
                                f"({(time.time() - t_start) / (global_step - step0) * 1e3:.0f} ms/step)")
            if dnt and global_step % dnt_interval == 0:
                dnt.track_dead_neurons(core_vae, global_step)
            if global_step % save_interval == 0 and is_main:
                d = os.path.join(output_dir, f"{ckpt_prefix}-{global_step}")
                save_state(d, vae_wrapper, trainer)
                logger.info(f"Saved periodic training state to {d}")
            if val_dataloader and data_cfg.get("do_validation", False) and val_steps > 0 and global_step % val_steps == 0:
                run_validation(trainer, val_dataloader, kl_weight, global_step, mlog, device, world)
            if global_step >= max_train_steps:
                break
        if world > 1:
            dist.all_reduce(epoch_sums)
            epoch_sums /= world
        es = (epoch_sums / max(steps_in_epoch, 1)).tolist()
        nan = float("nan")
        mlog.log({"train/epoch_avg_loss": es[2] if steps_in_epoch else nan, "train/epoch_avg_rec_loss": es[0] if steps_in_epoch else nan,
                  "train/epoch_avg_kl_loss": es[1] if steps_in_epoch else nan, "epoch_completed": epoch}, global_step)
        logger.info(f"Epoch {epoch} completed. Avg Train Loss: {es[2] if steps_in_epoch else nan:.4e}")
        if val_dataloader and data_cfg.get("do_validation", False) and val_epochs > 0 and (epoch + 1) % val_epochs == 0 and val_steps <= 0:
            run_validation(trainer, val_dataloader, kl_weight, global_step, mlog, device, world)
        if global_step >= max_train_steps:
            logger.info("Reached max_train_steps.")
            break
    if world > 1:
        dist.barrier()
    logger.info("Training finished.")

    if is_main:
        final_dir = os.path.join(output_dir, "final_model")
        save_state(final_dir, vae_wrapper, trainer)
        core_vae.save_pretrained(os.path.join(final_dir, "vae"))  # what evaluate.py loads (evaluate.py:91-102)
        if use_ema:
            with trainer.ema_weights():
                core_vae.save_pretrained(os.path.join(final_dir, "vae_ema"))  # evaluate.py --use_ema
        logger.info(f"Final training state and unwrapped VAE saved under {final_dir}")
        if monitor:
            recs = monitor.export_all_processed_data_to_records()
            if recs:
                path = os.path.join(output_dir, "tracked_activation_stats.csv")
                with open(path, "w", newline="") as f:
                    wr = csv.DictWriter(f, fieldnames=list(recs[0].keys()))
                    wr.writeheader()
                    wr.writerows(recs)
                logger.info(f"Saved activation stats to {path}")
        if wdt and wdt.history:
            path = os.path.join(output_dir, "weight_dynamics_history.csv")
            with open(path, "w", newline="") as f:
                wr = csv.DictWriter(f, fieldnames=list(WD_CSV_FIELDS))
                wr.writeheader()
                wr.writerows(wdt.export_records())
            logger.info(f"Saved weight dynamics to {path}")
        if dnt and dnt.percent_history:
            path = os.path.join(output_dir, "dead_neuron_percentage_history.csv")
            with open(path, "w", newline="") as f:
                wr = csv.writer(f)
                wr.writerow(["layer", "step", "percentage"])
                for name, hist in dnt.percent_history.items():
                    for step, pct in hist:
                        wr.writerow([name, step, pct])
            logger.info(f"Saved dead-weight percentages to {path}")
    mlog.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except Exception as e:
        logging.getLogger(__name__).error(f"Unhandled exception in main: {e}", exc_info=True)
        sys.exit(1)
