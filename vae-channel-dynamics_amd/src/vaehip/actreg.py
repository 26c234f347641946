"""Activation penalties of the fused train step (not in the reference, whose only cure for a fading channel is the GroupNorm
gamma nudge): a loss term on a module's output a of shape [B, H, W, C], N = B H W, w_c the 0 / 1 channel mask (all ones, or
ones on `channels`):

    ceiling, threshold t:  P = weight / (N C) sum_c w_c sum_{b,p} relu(|a| - t)^2
    floor,   threshold t:  P = weight / C sum_c w_c relu(t - m_c)^2,  m_c = (1 / N) sum_{b,p} |a|

The ceiling holds down the outliers that fp16 cannot carry (the last bin of log2_histogram_per_channel), the floor lifts the
channels whose mean |A| the classifier calls inactive.  The step's loss becomes rec + kl_weight kl + sum over targets of P.
Engine.add_activation_penalty registers a spec on a module; the kernels are in csrc/actreg.hip (ops.actreg_stats,
ops.actreg_inject)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

KINDS = ("ceiling", "floor")   # index = the kind of vae_actreg_final / vae_actreg_inject


def _finite(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
        raise ValueError(f"{name}={v!r}: expected a finite number")
    return float(v)


@dataclass(frozen=True)
class ActivationPenalty:
    kind: str
    threshold: float
    weight: float = 1.0
    channels: Optional[Tuple[int, ...]] = None

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"activation penalty kind {self.kind!r}: expected one of {', '.join(KINDS)}")
        object.__setattr__(self, "threshold", _finite("threshold", self.threshold))
        object.__setattr__(self, "weight", _finite("weight", self.weight))
        if not self.threshold > 0.0:
            raise ValueError(f"threshold={self.threshold!r}: must be > 0")
        if not self.weight >= 0.0:
            raise ValueError(f"weight={self.weight!r}: must be >= 0")
        if self.channels is not None:
            ch = self.channels
            if isinstance(ch, (str, bytes)) or not hasattr(ch, "__iter__"):
                raise ValueError(f"channels={ch!r}: expected a list of channel indices")
            ch = tuple(ch)
            if not ch or any(isinstance(c, bool) or not isinstance(c, int) for c in ch):
                raise ValueError(f"channels={list(ch)!r}: expected a non-empty list of ints")
            if any(c < 0 for c in ch):
                raise ValueError(f"channels={list(ch)!r}: a channel index is negative")
            if len(set(ch)) != len(ch):
                raise ValueError(f"channels={list(ch)!r}: a channel is listed twice")
            object.__setattr__(self, "channels", ch)

    @property
    def kind_id(self) -> int:
        return KINDS.index(self.kind)

    def check_channels(self, C: int) -> None:
        """the listed channels against the width of the target (known at registration)"""
        if self.channels is not None:
            bad = [c for c in self.channels if c >= C]
            if bad:
                raise ValueError(f"channels={list(self.channels)!r}: {bad} out of range for a module with {C} output channels")


def from_mapping(entry) -> ActivationPenalty:
    """one `targets:` entry of the YAML section (without its name): kind, threshold, weight (default 1.0), channels (optional)"""
    known = {"kind", "threshold", "weight", "channels"}
    extra = sorted(set(entry) - known)
    if extra:
        raise ValueError(f"unknown keys {extra} (known: {sorted(known)})")
    for k in ("kind", "threshold"):
        if k not in entry:
            raise ValueError(f"`{k}` is missing")
    return ActivationPenalty(entry["kind"], entry["threshold"], entry.get("weight", 1.0), entry.get("channels"))
