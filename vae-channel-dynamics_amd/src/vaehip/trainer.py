"""One optimizer step of the reference's hot loop (src/train.py:283-306) on the HIP engine:
fwd + loss + bwd (+ bucketed RCCL gradient mean) + fused clip/AdamW + LambdaLR, no host sync."""
from __future__ import annotations

import contextlib
from typing import Callable, Optional

import torch
import torch.distributed as dist

from . import ops
from .dp import GradBucketReducer, allreduce_mean_, broadcast_params
from .losses import as_spec
from .optim import FusedAdamW
from .trainable import apply_trainable, span_of


def lr_lambda_factory(warmup: int, max_steps: int) -> Callable[[int], float]:
    """train.py:197-200 (note: gives lr = 0 on the very first optimizer step)."""
    def fn(step: int) -> float:
        if step < warmup:
            return float(step) / float(max(1, warmup))
        progress = float(step - warmup) / float(max(1, max_steps - warmup))
        return max(0.0, 1.0 - min(1.0, progress))
    return fn


def _show(ranges, most: int = 6) -> str:
    n = sum(e - b for b, e in ranges)
    head = ", ".join(f"[{b}, {e})" for b, e in ranges[:most])
    return f"{head}{', ...' if len(ranges) > most else ''} ({len(ranges)} range(s), {n} elements)"


class HipTrainer:
    def __init__(self, wrapper, *, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=1.0,
                 kl_weight=1e-6, lr_warmup_steps=100, max_train_steps=1000, scheduler_steps_per_update: int = 1,
                 bucket_mb: float = 64.0, generator: Optional[torch.Generator] = None, mixed_precision: str = "no",
                 gradient_accumulation_steps: int = 1, checkpoint_decoder: bool = False, time_comm: bool = False,
                 one_rank_exchange: bool = False, use_ema: bool = False, ema_decay: float = 0.9999, trainable=None,
                 recon_loss=None, activation_penalties=None):
        """recon_loss: a vaehip.losses.ReconLoss (None: the reference's MSE), the reconstruction term of every train_step;
        eval_step keeps the reference's MSE.
        activation_penalties: a list of (module name, vaehip.actreg.ActivationPenalty): loss terms on module outputs, registered
        on the engine (Engine.add_activation_penalty) under names that resolve as tracking.target_layers names do (from the
        wrapper, `vae.decoder...`; the wrapper's `vae.` may be left out).  eval_step ignores them.
        trainable: None (requires_grad as the user left it, read now), 'all', 'decoder', 'encoder' or a list of module-name
        prefixes (vaehip.trainable); change it later with set_trainable()."""
        self.wrapper = wrapper
        self.vae = wrapper.vae
        apply_trainable(self.vae, trainable)
        self.kl_weight = float(kl_weight)
        self.recon_loss = as_spec(recon_loss)
        # the default spec makes the call the step always made
        self._loss_kw = {} if self.recon_loss.is_default else {"recon_loss": self.recon_loss}
        self.generator = generator
        self.vae.engine.set_precision(mixed_precision)
        self.vae.engine.checkpoint_decoder = bool(checkpoint_decoder)
        # accelerator.accumulate (train.py:286): the loss of every micro-batch is divided by N, gradients add up over N
        # micro-batches, ranks exchange only on the N-th, and clip / AdamW / LR schedule run once per N micro-batches
        self.accum_steps = int(gradient_accumulation_steps)
        if self.accum_steps < 1:
            raise ValueError("gradient_accumulation_steps must be >= 1")
        self.micro_step = 0
        self._accum: Optional[torch.Tensor] = None
        self.bucket_mb = float(bucket_mb)
        self.time_comm = bool(time_comm)
        self.optimizer = FusedAdamW(self.vae, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                    max_grad_norm=max_grad_norm, use_ema=use_ema, ema_decay=ema_decay)
        self.optimizer.refresh_trainable()
        self.lr_scheduler = torch.optim.lr_scheduler.LambdaLR(self.optimizer, lr_lambda_factory(lr_warmup_steps, max_train_steps))
        # accelerate steps the scheduler num_processes times per optimizer step (accelerate/scheduler.py:72-82)
        self.scheduler_steps_per_update = int(scheduler_steps_per_update)
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        # the gradient exchange runs when there is someone to exchange with -- or, as a self-test of the RCCL path on a one-GPU
        # box (dp.GradBucketReducer.one_rank_exchange), on a one-rank process group
        self.one_rank_exchange = bool(one_rank_exchange) and dist.is_initialized()
        self.exchanging = self.world > 1 or self.one_rank_exchange
        self.reducer: Optional[GradBucketReducer] = None   # made on first use (arena.grad exists after the first backward)
        self._accum_reducer: Optional[GradBucketReducer] = None
        if self.exchanging:
            broadcast_params(self.vae.arena.flat, 0, one_rank_exchange=self.one_rank_exchange)
        self.global_step = 0
        self.last = None
        self.activation_penalties = []  # (name, handle) in the order given
        for i, entry in enumerate(activation_penalties or []):
            try:
                name, spec = entry
                handle = self.vae.engine.add_activation_penalty(self._resolve_module(name), spec)
            except (TypeError, ValueError, AttributeError) as e:
                for _, h in self.activation_penalties:  # a refused list leaves nothing registered
                    h.remove()
                which = entry[0] if isinstance(entry, (tuple, list)) and entry else entry
                raise ValueError(f"activation_penalties[{i}] ({which!r}): {e}") from None
            self.activation_penalties.append((name, handle))

    def _resolve_module(self, dotted: str):
        """a module by its name from the wrapper (`vae.decoder.mid_block`) or from the VAE (`decoder.mid_block`), through the
        resolver of tracking.target_layers names (one rule for both)"""
        from tracking.monitor import _resolve
        if not isinstance(dotted, str) or not dotted:
            raise ValueError(f"module name {dotted!r}: expected a dotted name")
        root = self.wrapper if hasattr(self.wrapper, dotted.split(".")[0]) else self.vae
        cur = _resolve(root, dotted)
        if not isinstance(cur, torch.nn.Module):
            raise ValueError(f"'{dotted}' is not a module")
        return cur

    def activation_penalty_report(self) -> Optional[torch.Tensor]:
        """float64 [targets, 3] on the device, no host sync: per registered penalty, in order, its value in the last
        train_step, the elements over its threshold and the channels whose mean |A| is under it (both over the channels the
        penalty covers); NaN for a target whose module has not run.  None when no penalty is registered."""
        if not self.activation_penalties:
            return None
        dev = self.vae.arena.flat.device
        rows = []
        for _, h in self.activation_penalties:
            if h.last is None:
                rows.append(torch.full((3,), float("nan"), device=dev, dtype=torch.float64))
                continue
            sums, value = h.last
            m = h.mask(sums.device)
            over = sums[2] if m is None else sums[2] * m
            under = sums[1] < h.spec.threshold * h.rows
            if m is not None:
                under = under & (m > 0)
            rows.append(torch.stack([value, over.sum(), under.sum().to(torch.float64)]))
        return torch.stack(rows)

    @property
    def sync_gradients(self) -> bool:
        """True when the LAST train_step call ended with an optimizer update (accelerator.sync_gradients)."""
        return self.micro_step == 0

    def set_trainable(self, value):
        """change the trainable set (the values of the constructor's `trainable`; None reads requires_grad again).  The moments
        of a parameter that freezes stay as they are and are picked up again if it thaws.  Refused inside an accumulation window."""
        if self.micro_step:
            raise RuntimeError(f"set_trainable(): {self.micro_step} micro-batch(es) are pending; call it after an optimizer "
                               "update or after flush()")
        apply_trainable(self.vae, value)
        self.optimizer.refresh_trainable()
        self.vae.arena.attach_grads()   # a parameter that froze loses its .grad now, not at the next step
        self.reducer = self._accum_reducer = None

    @property
    def trainable_ranges(self):
        """merged [begin, end) arena ranges of the trainable parameters"""
        return list(self.optimizer.ranges if self.optimizer.ranges is not None else self.optimizer.refresh_trainable())

    def _make_reducer(self, flat: torch.Tensor) -> GradBucketReducer:
        return GradBucketReducer(flat, bucket_mb=self.bucket_mb, time_finish=self.time_comm, one_rank_exchange=self.one_rank_exchange,
                                 span=span_of(self.trainable_ranges))

    def _accumulating_step(self, pixel_values, eps, end_of_dataloader: bool):
        """one micro-batch of an N-micro-batch update; returns (result, update_due).  The update is due on the N-th
        micro-batch, or on the LAST batch of a dataloader pass whatever the count (accelerate's `accumulate` forces
        sync_gradients there, accelerator.py:_do_sync; the 1/N loss scale stays, as in accelerate).
        Exchange (world > 1): the mean over ranks is linear, so the sum of the earlier micro-batches (`_accum`) is
        all-reduced in buckets from the START of the due micro-batch -- under its whole forward + backward -- and that
        micro-batch's own gradient goes through the watermark-driven reducer under its backward; the two means are then
        added.  Nothing is exchanged on the other micro-batches (DDP no_sync)."""
        eng = self.vae.engine
        grad = self.vae.arena.grad
        due = (self.micro_step + 1 == self.accum_steps) or bool(end_of_dataloader)
        first = self.micro_step == 0
        exchange = due and self.exchanging
        acc_red = None
        if exchange:
            if not first:
                if self._accum_reducer is None or self._accum_reducer.flat.data_ptr() != self._accum.data_ptr():
                    self._accum_reducer = self._make_reducer(self._accum)
                acc_red = self._accum_reducer
                acc_red.begin()
                acc_red.ready(0)  # every bucket of the earlier micro-batches' sum is final: all in flight now
            if self.reducer is None or self.reducer.flat.data_ptr() != grad.data_ptr():
                self.reducer = self._make_reducer(grad)
            self.reducer.begin()
            eng.reducer = self.reducer
        try:
            res = eng.forward_backward(pixel_values, eps, self.kl_weight, True, self.generator, grad_scale=1.0 / self.accum_steps,
                                       **self._loss_kw)
        finally:
            eng.reducer = None
        grad = self.vae.arena.grad
        if exchange:
            self.reducer.finish()
            if acc_red is not None:
                acc_red.finish()
        self.micro_step += 1
        if first:
            if not due:
                if self._accum is None or self._accum.shape != grad.shape:
                    self._accum = torch.empty_like(grad)
                self._accum.copy_(grad)
            return res, due            # a one-micro-batch update (flush right after an update): grad is already the sum
        dst = grad if due else self._accum   # the sum ends up in arena.grad, where the optimizer reads it
        self._add(self._accum, grad, dst)
        return res, due

    @staticmethod
    def _add(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor):
        ops.lib.call("vae_add", ops._p(a), ops._p(b), a.numel(), ops._p(out), ops._stream())

    def train_step(self, pixel_values: torch.Tensor, eps: Optional[torch.Tensor] = None, end_of_dataloader: bool = False):
        """one micro-batch; returns the engine result dict, result['scalars'] = device tensor [mse, kl, total] of THIS
        rank.  With gradient_accumulation_steps = N the optimizer / scheduler / global_step advance on every N-th call
        and on a call with end_of_dataloader=True (`sync_gradients` tells which)."""
        eng = self.vae.engine
        if self.accum_steps > 1:
            res, due = self._accumulating_step(pixel_values, eps, end_of_dataloader)
            self.last = res
            if not due:
                return res
            self.micro_step = 0
        else:
            if self.exchanging:
                if self.reducer is None or self.reducer.flat.data_ptr() != self.vae.arena.grad.data_ptr():
                    self.reducer = self._make_reducer(self.vae.arena.grad)
                self.reducer.begin()
                eng.reducer = self.reducer
            try:
                res = eng.forward_backward(pixel_values, eps, self.kl_weight, True, self.generator, **self._loss_kw)
            finally:
                eng.reducer = None
            if self.exchanging:
                self.reducer.finish()
        self._update()
        self.last = res
        return res

    @property
    def pending_micro_batches(self) -> int:
        """micro-batches accumulated since the last optimizer update"""
        return self.micro_step

    def flush(self):
        """optimizer update from the micro-batches accumulated so far, without a new one (a dataloader pass that ends
        on a batch every rank skipped).  No-op when nothing is pending."""
        if self.micro_step == 0:
            return
        grad = self.vae.arena.grad
        grad.copy_(self._accum)
        if self.exchanging:
            lo, hi = span_of(self.trainable_ranges)
            allreduce_mean_(grad[lo:hi], one_rank_exchange=self.one_rank_exchange)
        self.micro_step = 0
        self._update()

    def _update(self):
        self.optimizer.step()
        for _ in range(self.scheduler_steps_per_update):
            self.lr_scheduler.step()
        self.global_step += 1

    @contextlib.contextmanager
    def ema_weights(self):
        """inside, the arena holds the averaged weights (and optimizer.ema the raw ones): eval_step, save_pretrained and
        state_dict read the average, and in bf16 mode the next forward repacks the bf16 image from it.  The two buffers are
        exchanged back on exit, bit for bit.  Not for use between the micro-batches of one update's backward passes."""
        opt = self.optimizer
        if not opt.use_ema:
            raise RuntimeError("ema_weights(): this trainer was built with use_ema=False")
        flat = opt._ensure().flat
        # a frozen element is its own average: only the trainable ranges change places, so a frozen weight that was nudged or
        # re-loaded is seen as it is now
        ranges = [(0, flat.numel())] if opt.all_trainable else opt.ranges

        def exchange():
            with torch.no_grad():
                for b, e in ranges:
                    tmp = flat[b:e].clone()
                    flat[b:e].copy_(opt.ema[b:e])
                    opt.ema[b:e].copy_(tmp)
        exchange()
        try:
            yield
        finally:
            exchange()

    def state_dict(self) -> dict:
        """everything a restart needs beside the weights: optimizer (with the weight average), scheduler, step counters,
        the gradient sum of a pending accumulation window, the generator."""
        sd = {"optimizer": self.optimizer.state_dict(), "lr_scheduler": self.lr_scheduler.state_dict(),
              "global_step": self.global_step, "micro_step": self.micro_step,
              "accum": self._accum.detach().cpu() if (self.micro_step > 0 and self._accum is not None) else None,
              "generator": self.generator.get_state() if self.generator is not None else None,
              "trainable_ranges": [list(r) for r in self.trainable_ranges]}
        return sd

    def load_state_dict(self, sd: dict):
        """the weights must be in the arena already (an optimizer state without an average starts it from them)"""
        mine = [list(r) for r in self.trainable_ranges]
        theirs = sd.get("trainable_ranges")  # a state from before parameters could be frozen trained them all
        theirs = [[0, self.vae.arena.total]] if theirs is None else [list(map(int, r)) for r in theirs]
        if theirs != mine:
            raise ValueError(f"trainer state was saved with the trainable arena ranges {_show(theirs)}, this trainer trains "
                             f"{_show(mine)}: build it with the same trainable set")
        self.optimizer.load_state_dict(sd["optimizer"])
        self.lr_scheduler.load_state_dict(sd["lr_scheduler"])
        self.global_step = int(sd["global_step"])
        self.micro_step = int(sd.get("micro_step", 0))
        acc = sd.get("accum")
        if acc is not None:
            self._accum = acc.to(self.vae.arena.flat.device, dtype=torch.float32).clone()
        elif self.micro_step:
            raise ValueError("trainer state has pending micro-batches but no accumulated gradient")
        if sd.get("generator") is not None:
            if self.generator is None:
                raise ValueError("trainer state holds a generator state, but this trainer has no generator")
            self.generator.set_state(sd["generator"])

    def exposed_comm_ms(self) -> float:
        """time the compute stream waited in reducer.finish() since the last call (0 when the exchange was hidden under
        the backward pass or the world is 1); needs time_comm=True; synchronises the device"""
        return sum(r.exposed_ms() for r in (self.reducer, self._accum_reducer) if r is not None)

    @torch.no_grad()
    def eval_step(self, pixel_values: torch.Tensor):
        """validation forward (train.py:75-78): deterministic latents, sum-reduced MSE and KL."""
        res = self.vae.engine.forward_eval(pixel_values, None, False, self.kl_weight)
        n = pixel_values.numel()
        b = pixel_values.shape[0]
        sc = res["scalars"]
        return {"rec_sum": sc[0] * n, "kl_sum": sc[1] * b, **res}
