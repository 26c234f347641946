"""Logit lens for VAE activations: per-channel activation maps and "mini-decoder" projections of an intermediate layer,
saved as pictures (the reference's src/analysis/logit_lens.py: same constructor, config keys, methods, directory layout,
file names, log and skip behaviour).

The arithmetic runs on the HIP engine (vaehip.ops.lens_planes / lens_project, csrc/lens.hip): min/max normalisation of the
selected planes, and Sigmoid(ConvT(ReLU(ConvT(x)))) with the hidden image kept on chip.  There is one compute path and no
torch convolution in it; `mini_decoder` is an ordinary nn.Sequential that only holds the weights (same modules, same
construction order as the reference, so a torch seed draws the same weights, and a state dict can be loaded into it).

Activations are accepted in two forms:
  * a device tensor, fp32 or bf16, in the engine's NHWC layout (B, H, W, C): what SDXLVAEWrapper.add_device_captures stores;
    it is read in place, only the results come to the host;
  * a CPU tensor (B, C, H, W), the reference's contract and what ActivityMonitor hands out: only the samples and channels
    that are drawn are sliced and uploaded.
Compute (`channel_maps`, `project`: tensors in, device tensors out) and rendering (`render_*`: host arrays in, files out)
are separate; matplotlib is imported when the first figure is rendered.
"""
import logging
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

logger = logging.getLogger(__name__)

SINGLE_CHANNEL, FULL_MAP = "mini_decoder_single_channel", "mini_decoder_full_map"


def _pyplot():
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError as e:
        raise RuntimeError("the logit lens renders its figures with matplotlib, which is not installed "
                           "(the tensors are available without it: VAELogitLens.channel_maps / project)") from e
    return plt


def render_image_row(images: Sequence[np.ndarray], titles: Sequence[str], save_path: str, colormap: Optional[str] = None) -> int:
    """one figure with a subplot per image ((H, W) maps drawn with `colormap`, (H, W, 3) images as they are), axes hidden,
    saved to save_path -> the number of subplots"""
    plt = _pyplot()
    n = len(images)
    fig, axes = plt.subplots(1, n, figsize=(n * 4, 4))
    axes = [axes] if n == 1 else list(axes)  # a single subplot comes back bare
    for ax, img, title in zip(axes, images, titles):
        ax.imshow(img, cmap=colormap) if np.ndim(img) == 2 else ax.imshow(img)
        ax.set_title(title)
        ax.axis("off")
    plt.tight_layout()
    plt.savefig(save_path)
    n_axes = len(fig.axes)
    plt.close(fig)
    return n_axes


def render_channel_maps(normalized: np.ndarray, save_path: str, colormap: str = "viridis") -> int:
    """normalized: (K, H, W) maps in [0, 1] -> sample_<i>_all_channels.png"""
    return render_image_row(list(normalized), [f"Channel {c}" for c in range(len(normalized))], save_path, colormap)


def render_single_channel_projections(projected: np.ndarray, save_path: str) -> int:
    """projected: (K, H', W', 3) images in [0, 1] -> lens_sample_<i>_single_channel_projections_combined.png"""
    return render_image_row(list(projected), [f"Proj. Ch. {c}" for c in range(len(projected))], save_path)


def save_projection_png(image: np.ndarray, save_path: str):
    """image: (H', W', 3) in [0, 1] -> an 8-bit RGB PNG, (x * 255).round() as evaluate.save_png"""
    from PIL import Image
    a = np.clip(np.round(np.asarray(image, dtype=np.float32) * 255.0), 0, 255).astype(np.uint8)
    Image.fromarray(a).save(save_path)


def logical_shape(t: torch.Tensor) -> Tuple[int, int, int, int]:
    """(B, C, H, W) of an accepted activation: a device tensor is NHWC, a CPU tensor (B, C, H, W)"""
    if t.is_cuda:
        B, H, W, C = t.shape
        return B, C, H, W
    return tuple(t.shape)


class VAELogitLens:
    def __init__(self, model_for_lens: Optional[nn.Module] = None, logit_lens_config: Optional[Dict[str, Any]] = None,
                 main_experiment_output_dir: str = "./experiment_outputs"):
        self.model = model_for_lens
        self.config = logit_lens_config if logit_lens_config is not None else {}
        self.default_num_channels = self.config.get("default_num_channels_to_viz", 4)
        self.default_batch_samples = self.config.get("default_num_batch_samples_to_viz", 1)
        self.visualization_base_dir = os.path.join(main_experiment_output_dir,
                                                   self.config.get("visualization_output_subdir", "logit_lens_visualizations"))
        os.makedirs(self.visualization_base_dir, exist_ok=True)
        logger.info(f"VAELogitLens initialized. Visualizations will be saved in: {self.visualization_base_dir}")
        # holds the weights only (the kernels compute); built on the CPU, no GPU is needed here
        cin = int(self.config.get("mini_decoder_input_channels", 1))
        up2x = dict(kernel_size=3, stride=2, padding=1, output_padding=1)
        self.mini_decoder = nn.Sequential(nn.ConvTranspose2d(cin, 16, **up2x), nn.ReLU(), nn.ConvTranspose2d(16, 3, **up2x), nn.Sigmoid())
        self._device_weights = None  # (key, device, [w1, b1, w2, b2])
        logger.info("Placeholder mini-decoder initialized.")

    # ------------------------------------------------------------------ helpers
    def _get_safe_layer_name(self, layer_identifier: str) -> str:
        return layer_identifier.replace(".", "_").replace("/", "_")

    def get_layer_logit_length(self, activation_map_tensor: torch.Tensor, layer_identifier: str) -> Optional[int]:
        """the number of channels of a 4-D activation (logged), None for anything else"""
        if not isinstance(activation_map_tensor, torch.Tensor) or activation_map_tensor.ndim != 4:
            shape = activation_map_tensor.shape if hasattr(activation_map_tensor, "shape") else "N/A"
            logger.warning(f"Cannot compute logit length for {layer_identifier}: activation map is not a 4D tensor. Shape: {shape}")
            return None
        num_channels = logical_shape(activation_map_tensor)[1]
        logger.info(f"Logit length (number of channels) for layer '{layer_identifier}': {num_channels}")
        return num_channels

    def _device(self) -> torch.device:
        if self.model is not None:
            p = next(iter(self.model.parameters()), None)
            if p is not None and p.is_cuda:
                return p.device
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the logit lens computes on the HIP engine (no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device())

    def _weights(self, device: torch.device) -> List[torch.Tensor]:
        """fp32 device copies of the mini-decoder's parameters, refreshed when the module's parameters change"""
        params = [self.mini_decoder[0].weight, self.mini_decoder[0].bias, self.mini_decoder[2].weight, self.mini_decoder[2].bias]
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self._device_weights is None or self._device_weights[0] != key or self._device_weights[1] != device:
            self._device_weights = (key, device, [p.detach().to(device=device, dtype=torch.float32).contiguous() for p in params])
        return self._device_weights[2]

    def _operand(self, act, samples: int, channels: Sequence[int]):
        """-> (NHWC device tensor, device int32 channel list, host channel list, samples) for the kernels.  A device tensor is
        used in place; of a CPU (B, C, H, W) tensor only the `samples` x `channels` planes are uploaded, as a fresh NHWC tensor
        whose channels are the listed ones in order."""
        if not isinstance(act, torch.Tensor) or act.ndim != 4:
            raise ValueError(f"expected a 4-D activation tensor, got {type(act).__name__} of shape {getattr(act, 'shape', 'N/A')}")
        channels = [int(c) for c in channels]
        B, C, H, W = logical_shape(act)
        if not 1 <= samples <= B or not channels or any(not 0 <= c < C for c in channels):
            raise ValueError(f"samples={samples}, channels={channels} do not fit an activation of logical shape {(B, C, H, W)}")
        if act.is_cuda:
            x = act if act.dtype in (torch.float32, torch.bfloat16) else act.float()
        else:
            dev = self._device()
            planes = act[:samples][:, channels]  # (S, K, H, W): all that leaves the host
            if planes.dtype not in (torch.float32, torch.bfloat16):
                planes = planes.float()
            x = planes.permute(0, 2, 3, 1).contiguous().to(dev)
            channels = list(range(len(channels)))
        idx = torch.tensor(channels, dtype=torch.int32, device=x.device)
        return x, idx, channels, samples

    # ------------------------------------------------------------------ compute (device tensors out, nothing rendered)
    def channel_maps(self, act, samples: int, channels: Sequence[int]):
        """-> (maps [S, K, H, W], ranges [S, K, 2] = per-plane (min, max), normalized [S, K, H, W]) as fp32 device tensors:
        the raw planes of the first `samples` samples and the listed channels, and (x - min) / (max - min) per plane,
        0 where max - min <= 1e-6"""
        from vaehip import ops
        x, idx, host, S = self._operand(act, samples, channels)
        return ops.lens_planes(x, S, idx, host)

    def project(self, act, samples: int, channels: Sequence[int], projection_type: str = SINGLE_CHANNEL) -> torch.Tensor:
        """the mini-decoder's output as an fp32 HWC device tensor: [S, K, 4H, 4W, 3] (each listed channel on its own,
        mini_decoder_single_channel) or [S, 4H, 4W, 3] (the listed channels as the input, mini_decoder_full_map)"""
        from vaehip import ops
        if projection_type not in (SINGLE_CHANNEL, FULL_MAP):
            raise ValueError(f"Unknown projection_type: {projection_type}")
        full = projection_type == FULL_MAP
        cin = self.mini_decoder[0].in_channels
        if cin != (len(channels) if full else 1):
            raise ValueError(f"the mini-decoder expects {cin} input channels, {projection_type} of {len(channels)} channels gives it "
                             f"{len(channels) if full else 1}")
        x, idx, host, S = self._operand(act, samples, channels)
        return ops.lens_project(x, S, idx, *self._weights(x.device), full, host)

    # ------------------------------------------------------------------ pictures
    def visualize_channel_activation_maps(self, activation_map_tensor: torch.Tensor, layer_identifier: str, global_step: int,
                                          num_channels_to_viz: Optional[int] = None, num_batch_samples_to_viz: Optional[int] = None,
                                          colormap: str = "viridis"):
        if not isinstance(activation_map_tensor, torch.Tensor) or activation_map_tensor.ndim != 4:
            shape = activation_map_tensor.shape if hasattr(activation_map_tensor, "shape") else "N/A"
            logger.warning(f"Activation map for {layer_identifier} is not a 4D tensor. Shape: {shape}. Skipping visualization.")
            return
        n_ch = num_channels_to_viz if num_channels_to_viz is not None else self.default_num_channels
        n_s = num_batch_samples_to_viz if num_batch_samples_to_viz is not None else self.default_batch_samples
        batch_size, total_channels, _, _ = logical_shape(activation_map_tensor)
        self.get_layer_logit_length(activation_map_tensor, layer_identifier)
        samples, channels = min(n_s, batch_size), min(n_ch, total_channels)
        output_subdir = os.path.join(self.visualization_base_dir, f"step_{global_step}", self._get_safe_layer_name(layer_identifier))
        os.makedirs(output_subdir, exist_ok=True)
        if samples < 1 or channels < 1:
            return
        try:
            normalized = self.channel_maps(activation_map_tensor, samples, range(channels))[2].cpu().numpy()
        except Exception as e:
            logger.error(f"Error computing channel maps for {layer_identifier}: {e}", exc_info=True)
            return
        for sample_idx in range(samples):
            save_path = os.path.join(output_subdir, f"sample_{sample_idx}_all_channels.png")
            try:
                render_channel_maps(normalized[sample_idx], save_path, colormap)
            except Exception as e:
                logger.error(f"Error visualizing maps for {layer_identifier}, sample {sample_idx}: {e}", exc_info=True)
                continue
            logger.info(f"Saved combined activation map visualization for {layer_identifier}, sample {sample_idx} to {save_path}")

    def run_logit_lens_with_activations(self, global_step: int, layers_to_analyze: List[str], num_batch_samples_to_viz: Optional[int],
                                        projection_type: str, activations_to_process: Dict[str, torch.Tensor]):
        n_s = num_batch_samples_to_viz if num_batch_samples_to_viz is not None else self.default_batch_samples
        logger.info(f"\n--- Running Logit Lens for step {global_step} ---")
        if not activations_to_process:
            logger.warning("No activations provided to run_logit_lens_with_activations. Skipping.")
            return
        for layer_name in layers_to_analyze:
            if layer_name not in activations_to_process:
                logger.warning(f"No activation found for layer '{layer_name}' in provided dict. Skipping.")
                continue
            activation_map = activations_to_process[layer_name]
            batch_size, total_channels, height, width = logical_shape(activation_map)
            samples = min(n_s, batch_size)
            output_subdir = os.path.join(self.visualization_base_dir, f"step_{global_step}", self._get_safe_layer_name(layer_name),
                                         "logit_lens_projections")
            os.makedirs(output_subdir, exist_ok=True)
            logger.info(f"Processing Logit Lens for layer '{layer_name}' with shape {(batch_size, total_channels, height, width)}")
            if samples < 1:
                continue
            if projection_type == FULL_MAP and total_channels != self.mini_decoder[0].in_channels:
                for _ in range(samples):
                    logger.warning(f"Mismatch: Mini-decoder expects {self.mini_decoder[0].in_channels} input channels, "
                                   f"but layer '{layer_name}' has {total_channels} channels. Skipping full map projection.")
                continue
            if projection_type not in (SINGLE_CHANNEL, FULL_MAP):
                for _ in range(samples):
                    logger.warning(f"Unknown projection_type: {projection_type}. Skipping.")
                continue
            channels = total_channels if projection_type == FULL_MAP else min(self.default_num_channels, total_channels)
            try:
                projected = self.project(activation_map, samples, range(channels), projection_type).cpu().numpy()
            except Exception as e:
                logger.error(f"Error during Logit Lens projection for layer '{layer_name}': {e}", exc_info=True)
                continue
            for sample_idx in range(samples):
                try:
                    if projection_type == SINGLE_CHANNEL:
                        render_single_channel_projections(
                            projected[sample_idx], os.path.join(output_subdir, f"lens_sample_{sample_idx}_single_channel_projections_combined.png"))
                        logger.debug(f"Saved combined single-channel projections for {layer_name}, sample {sample_idx}")
                    else:
                        save_projection_png(projected[sample_idx], os.path.join(output_subdir, f"lens_sample_{sample_idx}_full_map.png"))
                        logger.debug(f"Saved full map projection for {layer_name}, sample {sample_idx}")
                except Exception as e:
                    logger.error(f"Error during Logit Lens projection for layer '{layer_name}', sample {sample_idx}: {e}", exc_info=True)
        logger.info(f"Logit Lens analysis completed for step {global_step}.")

    def project_with_mini_decoder(self, activation_map_tensor: torch.Tensor, layer_identifier: str, global_step: int,
                                  channel_idx: int = 0, sample_idx: int = 0):
        """one channel of one sample through the mini-decoder -> mini_decoded/sample_<i>_channel_<c>_projected.png"""
        batch_size, total_channels, _, _ = logical_shape(activation_map_tensor)
        if not (0 <= sample_idx < batch_size and 0 <= channel_idx < total_channels):
            logger.warning("Invalid sample_idx or channel_idx for mini-decoder projection. Skipping.")
            return
        try:
            one = activation_map_tensor[sample_idx:sample_idx + 1]
            image = self.project(one, 1, [channel_idx], SINGLE_CHANNEL)[0, 0].cpu().numpy()
            output_subdir = os.path.join(self.visualization_base_dir, f"step_{global_step}", self._get_safe_layer_name(layer_identifier),
                                         "mini_decoded")
            os.makedirs(output_subdir, exist_ok=True)
            save_path = os.path.join(output_subdir, f"sample_{sample_idx}_channel_{channel_idx}_projected.png")
            save_projection_png(image, save_path)
            logger.info(f"Saved mini-decoder projection for {layer_identifier}, sample {sample_idx}, channel {channel_idx} to {save_path}")
        except Exception as e:
            logger.error(f"Error during mini-decoder projection for {layer_identifier}: {e}", exc_info=True)
