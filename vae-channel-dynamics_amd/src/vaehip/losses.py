"""What the fused train step minimises beside the KL term (not in the reference, whose loss is plain MSE):

    rec = pixel + ssim_weight * (1 - ssim),   total = rec + kl_weight * kl

pixel is the mean of d^2 (`mse`), of |d| (`l1`) or of Huber's term (`huber`: |d| <= delta ? d^2 / 2 : delta (|d| - delta / 2),
torch.nn.functional.huber_loss) of d = recon - target; ssim is the mean SSIM index of (recon + 1) / 2 against (target + 1) / 2
(11 x 11 gaussian window, sigma 1.5, window positions wholly inside the image) WITHOUT evaluate.py's clamp to [0, 1]: a clamp
would zero the gradient exactly where a reconstruction has left [-1, 1].  The kernels are in csrc/recon_loss.hip
(ops.recon_loss); the default spec, `ReconLoss()`, is the MSE of the reference and takes the step's original two calls."""
from __future__ import annotations

from dataclasses import dataclass

KINDS = ("mse", "l1", "huber")   # index = VAE_LOSS_* of include/vaehip.h
SSIM_WINDOW = 11


@dataclass(frozen=True)
class ReconLoss:
    kind: str = "mse"
    huber_delta: float = 1.0
    ssim_weight: float = 0.0

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"reconstruction loss kind {self.kind!r}: expected one of {', '.join(KINDS)}")
        for name in ("huber_delta", "ssim_weight"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
                raise ValueError(f"{name}={v!r}: expected a finite number")
            object.__setattr__(self, name, float(v))
        if not self.huber_delta > 0.0:
            raise ValueError(f"huber_delta={self.huber_delta!r}: must be > 0")
        if not self.ssim_weight >= 0.0:
            raise ValueError(f"ssim_weight={self.ssim_weight!r}: must be >= 0")

    @property
    def kind_id(self) -> int:
        return KINDS.index(self.kind)

    @property
    def is_default(self) -> bool:
        """plain MSE: the step makes the calls it always made (ops.mse_kl_loss, ops.mse_bwd)"""
        return self.kind == "mse" and self.ssim_weight == 0.0


def as_spec(recon_loss) -> ReconLoss:
    """None -> the default spec; anything but a ReconLoss is refused"""
    if recon_loss is None:
        return ReconLoss()
    if not isinstance(recon_loss, ReconLoss):
        raise TypeError(f"recon_loss: expected a vaehip.losses.ReconLoss or None, got {type(recon_loss).__name__}")
    return recon_loss

