"""Fused clip + AdamW over the flat parameter arena (replaces clip_grad_norm_ + torch.optim.AdamW,
reference src/train.py:184-187,301-302).  One grad-norm reduction and one update kernel per step,
no host synchronisation: the clip coefficient is read from device memory by the update kernel.
"""
from __future__ import annotations

import logging
from typing import Optional

import torch

from . import ops
from .trainable import RangeTable

logger = logging.getLogger(__name__)


def ema_decay_at(t: int, ema_decay: float) -> float:
    """decay of the t-th optimizer update (t from 1): diffusers' EMAModel defaults (use_ema_warmup=False, update_after_step=0).
    The first update copies the weights (0); afterwards min(ema_decay, t / (9 + t)), diffusers' (1 + s) / (10 + s) at s = t - 1."""
    if t <= 1:
        return 0.0
    return min(float(ema_decay), t / (9.0 + t))


class FusedAdamW(torch.optim.Optimizer):
    """A torch.optim.Optimizer (so LambdaLR / accelerate can drive `param_groups[0]['lr']`)
    whose step() is two HIP kernels over `vae.arena.flat` / `.grad`."""

    def __init__(self, vae, lr: float = 1e-5, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: float = 0.0, use_ema: bool = False, ema_decay: float = 0.9999):
        if not 0.0 < float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must lie in (0, 1), got {ema_decay!r}")
        self._vae = vae
        params = list(vae.parameters())
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = float(max_grad_norm)
        self._arena_id = None
        self.exp_avg: Optional[torch.Tensor] = None
        self.exp_avg_sq: Optional[torch.Tensor] = None
        self.sqnorm: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None
        self.step_count = 0
        self.last_lr: Optional[float] = None
        # fp32 average of the weights, moved by the update kernel itself (vae_adamw_ema); None when use_ema is off
        self.use_ema = bool(use_ema)
        self.ema_decay = float(ema_decay)
        self.ema: Optional[torch.Tensor] = None
        # the trainable set as merged arena ranges (refresh_trainable); _table is None when every parameter trains: the step
        # is then vae_sqnorm + vae_adamw(_ema) over the whole arena, else the two *_ranges calls over the device table
        self.ranges: Optional[list] = None
        self._table: Optional[RangeTable] = None

    def refresh_trainable(self):
        """read requires_grad of the arena's parameters again (HipTrainer does when it is built and in set_trainable; a bare
        optimizer reads it at its first step): the merged ranges, and their device table unless they are the whole arena"""
        a = self._vae.arena
        ranges = a.trainable_ranges()
        if not ranges:
            raise ValueError("no parameter of the VAE has requires_grad: the trainable set is empty")
        if ranges != self.ranges or (self._table is not None and self._table.seg_off.device != a.flat.device):
            self.ranges = ranges
            whole = ranges == [(0, a.total)]
            self._table = None if whole or a.flat.device.type != "cuda" else RangeTable(ranges, a.flat.device, a.total)
        return self.ranges

    @property
    def all_trainable(self) -> bool:
        return self.ranges is None or self.ranges == [(0, self._vae.arena.total)]

    def _ensure(self):
        a = self._vae.arena
        if self._arena_id != id(a) or self.exp_avg is None or self.exp_avg.device != a.flat.device:
            old_m, old_v, old_e = self.exp_avg, self.exp_avg_sq, self.ema
            self.exp_avg = torch.zeros_like(a.flat)
            self.exp_avg_sq = torch.zeros_like(a.flat)
            if old_m is not None and old_m.numel() == a.flat.numel():
                self.exp_avg.copy_(old_m)
                self.exp_avg_sq.copy_(old_v)
            if self.use_ema:
                # starts as the weights themselves (in data-parallel runs: after broadcast_params, the same on every rank)
                self.ema = a.flat.detach().clone()
                if old_e is not None and old_e.numel() == a.flat.numel():
                    self.ema.copy_(old_e)
            self.sqnorm = torch.zeros(1, device=a.flat.device, dtype=torch.float32)
            self._ws = torch.empty(2048, device=a.flat.device, dtype=torch.float32)
            self._arena_id = id(a)
            self.ranges = self._table = None
        if self.ranges is None:
            self.refresh_trainable()
        return a

    def clip_grad_norm_(self, max_norm: float):
        """accelerate-style entry: just arms the fused clip for the next step()."""
        self.max_grad_norm = float(max_norm)

    @torch.no_grad()
    def step(self, closure=None):
        a = self._ensure()
        if a.flat.device.type != "cuda":
            raise RuntimeError("FusedAdamW needs the parameter arena on the GPU (no CPU fallback)")
        g = self.param_groups[0]
        self.step_count += 1
        self.last_lr = g["lr"]  # of the update this call applies (WeightDynamicsTracker's update ratio)
        hp = (self.sqnorm, self.max_grad_norm, g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.step_count)
        if self._table is not None:  # part of the model is frozen: norm and update over the trainable ranges only
            ops.sqnorm_ranges(a.grad, self._table, self.sqnorm)
            ops.adamw_ranges(a.flat, a.grad, self.exp_avg, self.exp_avg_sq, self.ema if self.use_ema else None, self._table, *hp,
                             ema_decay_at(self.step_count, self.ema_decay) if self.use_ema else 0.0)
            return
        ops.sqnorm(a.grad, self.sqnorm, self._ws)
        if self.use_ema:
            ops.adamw_ema(a.flat, a.grad, self.exp_avg, self.exp_avg_sq, self.ema, self.sqnorm, self.max_grad_norm, g["lr"],
                          g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.step_count,
                          ema_decay_at(self.step_count, self.ema_decay))
        else:
            ops.adamw(a.flat, a.grad, self.exp_avg, self.exp_avg_sq, self.sqnorm, self.max_grad_norm, g["lr"],
                      g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.step_count)

    def zero_grad(self, set_to_none: bool = True):
        # gradients are overwritten (not accumulated) by engine.forward_backward: nothing to clear
        return None

    def grad_norm(self) -> torch.Tensor:
        """device scalar: global L2 norm of the last step's (unclipped) gradients, over the trainable parameters only (what
        clip_grad_norm_ over the parameters with a gradient gives in the reference)."""
        return torch.sqrt(self.sqnorm[0])

    def state_dict(self):
        self._ensure()
        sd = {"step": self.step_count, "exp_avg": self.exp_avg.detach().cpu(), "exp_avg_sq": self.exp_avg_sq.detach().cpu(),
              "param_groups": [{k: v for k, v in self.param_groups[0].items() if k != "params"}],
              "max_grad_norm": self.max_grad_norm}
        if self.use_ema:  # without it the file is what it was before the average existed
            sd.update(ema=self.ema.detach().cpu(), use_ema=True, ema_decay=self.ema_decay)
        return sd

    def load_state_dict(self, sd):
        self._ensure()
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        for k, v in sd["param_groups"][0].items():
            self.param_groups[0][k] = v
        self.max_grad_norm = float(sd.get("max_grad_norm", self.max_grad_norm))
        if self.use_ema:
            if sd.get("ema") is not None:
                self.ema.copy_(sd["ema"])
            else:  # call this after the weights are in the arena
                self.ema.copy_(self._vae.arena.flat)
                logger.info("optimizer state holds no weight average: the EMA starts from the loaded weights")
