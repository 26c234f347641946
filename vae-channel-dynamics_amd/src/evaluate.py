"""Evaluation of a trained VAE checkpoint (reference src/evaluate.py:78-328): same CLI flags, loads
`<checkpoint_path>/vae`, deterministic reconstruction (latent mode), Average MSE / KL / PSNR / SSIM,
sample PNGs and `eval_metrics.txt` in the reference's format.

The forward runs on the HIP engine, and so do the metrics: MSE, PSNR (data_range 1.0 on [0,1]-clamped
images) and SSIM (11x11 gaussian, sigma 1.5; the reference needs torchmetrics) come from one fused device
kernel per batch (vaehip.ops.image_metrics, accumulated by vaehip.metrics.ImageMetrics), read straight from
the engine's channels-last reconstruction; KL is summed on the device too, so the loop synchronises the host
only to save the sample PNGs.  `to_unit`, `psnr_sums` and `ssim_per_image` below are the CPU definition the
kernel is held to (tests/test_eval_metrics.py, tests/test_image_metrics_gpu.py).

With `--enable_logit_lens` (on by default, as in the reference) the first batch's activations of `--logit_lens_layers` are
captured on the device (SDXLVAEWrapper.add_device_captures) and analysis.logit_lens.VAELogitLens draws their channel maps
and mini-decoder projections under `<output_dir>/<logit_lens.visualization_output_subdir>/step_0/<layer>/`; its arithmetic
runs in csrc/lens.hip on the captured tensors, only the pictures' pixels come to the host.  `first_batch_activations.pt`
(the captured tensors as logical (B, C, H, W) fp32 CPU tensors) is still written unless `--save_first_batch_activations
false`, which spares the whole-tensor transfer.
"""
import argparse
import logging
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from utils.config_utils import load_config
from utils.logging_utils import setup_logging
from data_utils import load_and_preprocess_dataset, create_dataloader
from models.sdxl_vae_wrapper import SDXLVAEWrapper
from vaehip.metrics import ImageMetrics

setup_logging()
logger = logging.getLogger(__name__)


def parse_args():
    p = argparse.ArgumentParser(description="Evaluate a trained SDXL VAE model.")
    p.add_argument("--config_path", type=str, required=True)
    p.add_argument("--checkpoint_path", type=str, required=True)
    p.add_argument("--eval_split", type=str, default="test")
    p.add_argument("--output_dir", type=str, default=None)
    p.add_argument("--num_samples_to_save", type=int, default=16)
    p.add_argument("--batch_size", type=int, default=None)
    p.add_argument("--enable_logit_lens", default=True, type=lambda x: (str(x).lower() == "true"))
    p.add_argument("--logit_lens_layers", type=str, nargs="+",
                   default=["encoder.down_blocks.0.resnets.0.norm1", "encoder.down_blocks.1.resnets.0.conv_shortcut"])
    p.add_argument("--logit_lens_num_samples", type=int, default=1)
    p.add_argument("--logit_lens_projection_type", type=str, default="mini_decoder_single_channel",
                   choices=["mini_decoder_single_channel", "mini_decoder_full_map"])
    p.add_argument("--logit_lens_mini_decoder_input_channels", type=int, default=None)
    # not a flag of the reference: first_batch_activations.pt is the one thing left that brings whole captured tensors to the host
    p.add_argument("--save_first_batch_activations", default=True, type=lambda x: (str(x).lower() == "true"))
    # not a flag of the reference: evaluate <checkpoint_path>/vae_ema, the averaged weights train.py saves with training.use_ema
    # (`--use_ema` or `--use_ema true`; `--use_ema false` evaluates the raw weights and says so in eval_metrics.txt)
    p.add_argument("--use_ema", nargs="?", const=True, default=None, type=lambda x: (str(x).lower() == "true"))
    return p.parse_args()


def model_directory(checkpoint_path: str, use_ema) -> str:
    """<checkpoint_path>/vae, or vae_ema when asked for; a missing directory ends the program with status 1"""
    model_path = os.path.join(checkpoint_path, "vae_ema" if use_ema else "vae")
    if not os.path.isdir(model_path):
        logger.error(f"{'EMA ' if use_ema else ''}VAE model directory not found at: {model_path}")
        sys.exit(1)
    return model_path


def to_unit(t: torch.Tensor) -> torch.Tensor:
    return torch.clamp((t + 1.0) / 2.0, 0.0, 1.0)


def psnr_sums(pred: torch.Tensor, target: torch.Tensor):
    """torchmetrics PeakSignalNoiseRatio(data_range=1.0) accumulates sum of squared error and count."""
    return torch.sum((pred - target) ** 2).double(), pred.numel()


def ssim_per_image(pred: torch.Tensor, target: torch.Tensor, sigma: float = 1.5, ksize: int = 11) -> torch.Tensor:
    """SSIM with a gaussian window (data_range 1.0, k1=0.01, k2=0.03), reflect-padded and border-cropped like torchmetrics.
    The window statistics are taken in float64: var = E[x^2] - mu^2 cancels catastrophically in fp32 on flat regions
    (errors of 1e-4 in the index against the 9e-4 stabiliser c2); torchmetrics itself works in the input dtype."""
    out_dtype = pred.dtype
    pred, target = pred.double(), target.double()
    c = pred.shape[1]
    ax = torch.arange(ksize, dtype=pred.dtype, device=pred.device) - (ksize - 1) / 2
    g = torch.exp(-(ax / sigma) ** 2 / 2)
    g = (g / g.sum()).unsqueeze(0)
    win = (g.t() @ g).expand(c, 1, ksize, ksize).contiguous()
    pad = (ksize - 1) // 2
    p = F.pad(pred, (pad, pad, pad, pad), mode="reflect")
    t = F.pad(target, (pad, pad, pad, pad), mode="reflect")
    stack = torch.cat([p, t, p * p, t * t, p * t])
    out = F.conv2d(stack, win, groups=c)
    mu_p, mu_t, e_pp, e_tt, e_pt = out.split(pred.shape[0])
    s_pp, s_tt, s_pt = e_pp - mu_p ** 2, e_tt - mu_t ** 2, e_pt - mu_p * mu_t
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p ** 2 + mu_t ** 2 + c1) * (s_pp + s_tt + c2))
    return ssim[..., pad:-pad, pad:-pad].reshape(pred.shape[0], -1).mean(-1).to(out_dtype)


def save_png(t: torch.Tensor, path: str):
    from PIL import Image
    a = (to_unit(t.float().cpu()) * 255.0).round().byte().permute(1, 2, 0).numpy()
    Image.fromarray(a).save(path)


def lens_settings(args, config) -> dict:
    """the analyzer's config as the reference builds it (evaluate.py:108-134); full-map projection without the decoder's
    channel count ends the program with status 1"""
    cin = args.logit_lens_mini_decoder_input_channels
    if cin is None:
        if args.logit_lens_projection_type == "mini_decoder_full_map":
            logger.error("For 'mini_decoder_full_map', --logit_lens_mini_decoder_input_channels must be specified.")
            sys.exit(1)
        cin = 1
    section = config.get("logit_lens", {}) or {}
    return {"visualization_output_subdir": section.get("visualization_output_subdir", "logit_lens_visualizations_eval"),
            "default_num_channels_to_viz": section.get("num_channels_to_viz", 4),
            "default_num_batch_samples_to_viz": args.logit_lens_num_samples,
            "mini_decoder_input_channels": cin,
            "colormap": section.get("colormap", "viridis"),
            "run_mini_decoder_projection": section.get("run_mini_decoder_projection", True)}


def run_logit_lens(lens, args, acts: dict):
    """channel maps and projections of the captured first batch (global step 0)"""
    for layer in args.logit_lens_layers:
        if layer in acts:
            lens.visualize_channel_activation_maps(acts[layer], layer, 0, num_batch_samples_to_viz=args.logit_lens_num_samples,
                                                   colormap=lens.config.get("colormap", "viridis"))
    lens.run_logit_lens_with_activations(global_step=0, layers_to_analyze=args.logit_lens_layers,
                                         num_batch_samples_to_viz=args.logit_lens_num_samples,
                                         projection_type=args.logit_lens_projection_type, activations_to_process=acts)


def host_activations(acts: dict) -> dict:
    """captured activations as the hook path hands them out: logical (B, C, H, W) fp32 CPU tensors"""
    return {k: (v.float().cpu().permute(0, 3, 1, 2) if v.is_cuda else v) for k, v in acts.items()}


def main():
    args = parse_args()
    config = load_config(args.config_path)
    lens_cfg = lens_settings(args, config) if args.enable_logit_lens else None  # (a bad flag combination ends here, before the GPU)
    if args.use_ema:  # a wrong checkpoint path is reported before anything else is touched
        model_directory(args.checkpoint_path, True)
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: evaluation runs on the HIP engine (no CPU fallback)")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    if args.output_dir is None:
        args.output_dir = os.path.join(args.checkpoint_path, f"eval_results_{args.eval_split}")
    os.makedirs(args.output_dir, exist_ok=True)
    model_path = model_directory(args.checkpoint_path, args.use_ema)
    w = SDXLVAEWrapper(pretrained_model_name_or_path=model_path, device=device)
    w.vae.eval()
    lens = None
    if lens_cfg is not None:
        from analysis.logit_lens import VAELogitLens
        logger.info("Logit Lens analysis enabled.")
        lens = VAELogitLens(model_for_lens=w.vae, logit_lens_config=lens_cfg, main_experiment_output_dir=args.output_dir)
    data_cfg = config.get("data", {})
    bs = args.batch_size or data_cfg.get("validation_batch_size", data_cfg.get("batch_size", 4))
    ds = load_and_preprocess_dataset(
        dataset_name=data_cfg.get("validation_dataset_name", data_cfg.get("dataset_name")),
        dataset_config_name=data_cfg.get("validation_dataset_config_name", data_cfg.get("dataset_config_name", None)),
        image_column=data_cfg.get("image_column", "image"), resolution=data_cfg.get("resolution", 256),
        max_samples=data_cfg.get("validation_max_samples", None), split=args.eval_split)
    dl = create_dataloader(ds, batch_size=bs, num_workers=data_cfg.get("num_workers", 0), shuffle=False)

    metrics = ImageMetrics()
    kl_sum = torch.zeros((), dtype=torch.float64, device=device)
    n = saved = 0
    with torch.no_grad():
        for step, batch in enumerate(dl):
            if step == 0 and lens is not None:
                w.add_device_captures(args.logit_lens_layers)
            pv = batch.get("pixel_values") if batch else None
            if pv is None:
                continue
            pv = pv.to(device, dtype=torch.float32)
            out = w(pv, sample_posterior=False)
            rec = out["reconstruction"]
            kl = out["latent_dist"].kl()
            b = pv.shape[0]
            metrics.update(rec.float(), pv)
            kl_sum += kl.double().sum()
            n += b
            while saved < args.num_samples_to_save and saved - (n - b) < b:
                i = saved - (n - b)
                save_png(pv[i], os.path.join(args.output_dir, f"sample_{saved}_orig.png"))
                save_png(rec[i], os.path.join(args.output_dir, f"sample_{saved}_recon.png"))
                saved += 1
            if step == 0 and lens is not None:
                acts = w.get_captured_activations()
                logger.info("Running LogitLens on first batch activations...")
                run_logit_lens(lens, args, acts)
                if args.save_first_batch_activations:
                    torch.save(host_activations(acts), os.path.join(args.output_dir, "first_batch_activations.pt"))
                w.remove_hooks()
                logger.info("LogitLens hooks removed.")
    m = metrics.compute()
    avg_mse, psnr, ssim = m["avg_mse"], m["psnr"], m["ssim"]
    avg_kl = float(kl_sum) / n if n else 0
    logger.info("***** Evaluation Results *****")
    logger.info(f"  Dataset split: {args.eval_split}; samples: {n}")
    logger.info(f"  Average MSE Loss: {avg_mse:.6f}  Average KL Divergence: {avg_kl:.6f}  PSNR: {psnr:.4f} dB  SSIM: {ssim:.4f}")
    with open(os.path.join(args.output_dir, "eval_metrics.txt"), "w") as f:
        f.write(f"Evaluation Split: {args.eval_split}\n")
        f.write(f"Checkpoint Path: {args.checkpoint_path}\n")
        f.write(f"Number of Samples Processed: {n}\n")
        f.write(f"Average MSE: {avg_mse}\n")
        f.write(f"Average KL: {avg_kl}\n")
        f.write(f"Average PSNR: {psnr}\n")
        f.write(f"Average SSIM: {ssim}\n")
        if args.use_ema is not None:
            f.write(f"Weights: {'ema' if args.use_ema else 'raw'}\n")


if __name__ == "__main__":
    try:
        main()
    except Exception as e:
        logging.getLogger(__name__).error(f"Unhandled exception in main: {e}", exc_info=True)
        sys.exit(1)
