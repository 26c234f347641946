"""Accumulation of evaluate.py's image metrics over batches (what torchmetrics' update / compute do for the reference,
src/evaluate.py:172-183,216-240): the per-image values come from the device kernel (ops.image_metrics), the running sums
stay on the device, and only compute() transfers anything."""
from __future__ import annotations

import math
from typing import Dict

import torch

from . import ops


class ImageMetrics:
    """Average MSE, PSNR (data range 1 on the [0,1]-mapped images) and SSIM of reconstructions against their targets."""

    def __init__(self):
        self._sums = None  # float64 [3]: sum of sse_raw, of sse_unit, of the per-image SSIM; on the device of the first update
        self.n = 0         # images
        self.numel = 0     # elements (C * H * W per image), the PSNR's count

    def update(self, rec: torch.Tensor, target: torch.Tensor) -> None:
        """one batch: (B, C, H, W) fp32 device tensors in [-1, 1], any strides"""
        self.update_from(ops.image_metrics(rec, target), rec[0].numel())

    def update_from(self, triples: torch.Tensor, numel_per_image: int) -> None:
        """the same accumulation from [B, 3] values (sse_raw, sse_unit, ssim per image) already computed; any device"""
        if triples.dim() != 2 or triples.shape[1] != 3:
            raise ValueError(f"ImageMetrics: expected [B, 3] per-image values, got {tuple(triples.shape)}")
        s = triples.double().sum(0)
        self._sums = s if self._sums is None else self._sums + s
        self.n += triples.shape[0]
        self.numel += triples.shape[0] * int(numel_per_image)

    def compute(self) -> Dict[str, float]:
        """evaluate's aggregation: avg_mse = sum sse_raw / elements (the mean of per-image MSEs: images of one size), psnr from
        the summed squared error over the summed element count, ssim = mean over images.  One device-to-host transfer."""
        if not self.n:
            return {"n": 0, "avg_mse": 0, "psnr": float("nan"), "ssim": float("nan")}
        sse_raw, sse_unit, ssim = self._sums.tolist()
        mse_unit = sse_unit / self.numel
        return {"n": self.n, "avg_mse": sse_raw / self.numel,
                "psnr": 10.0 * math.log10(1.0 / mse_unit) if mse_unit > 0 else float("inf"),
                "ssim": ssim / self.n}
