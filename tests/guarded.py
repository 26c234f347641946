"""Guarded, poisoned memory for kernel tests (a helper module, not a test).

GuardedPool hands out tensors that are views into private uint8 buffers filled with byte 0xFF: an all-ones word is a NaN
as fp32, bf16 and fp64 and -1 as an integer, so one pattern serves every dtype and guards are compared as bytes.

    [ front guard ............ | payload | back guard ............ ]
                                ^ 256-byte boundary (+ offset_bytes); the back guard starts at the payload's last byte + 1

* a store outside a tensor changes a guard byte                      -> pool.violations()
* an element a kernel never wrote still holds the poison             -> pool.unwritten(t) / pool.unwritten_report()
* a load outside an operand meets NaN instead of finite garbage      -> the result is poisoned and fails its value check
  (a load whose value never reaches a result stays invisible)

guarded(pool, *modules) swaps the module-global name `torch` of the given modules for a proxy whose allocation functions
(ROUTED) draw from the pool, so that every result and workspace a wrapper allocates is such a tensor.
"""
from __future__ import annotations

import contextlib
import sys
from typing import List, NamedTuple, Optional

import torch

POISON = 0xFF
ALIGN = 256                 # payload alignment: what torch's own device allocations have (the dispatcher looks at it)
MIN_GUARD = 256 * 1024      # one full output tile of the widest layer: 128 rows x 512 channels x 4 B
GUARD_ROWS = 128            # ... and at least this many rows of the tensor's own last dimension,
MAX_GUARD = 4 * 1024 * 1024  # up to this size: a 1-D buffer or a split-K slab has "rows" of many MiB (the parameter arena: 320 MiB),
#                              and 128 of them on either side of every such tensor do not fit the device.  A store is still seen
#                              unless it lands more than 4 MiB away from the tensor without touching anything nearer.

# the allocation functions the proxy routes to the pool (tests/test_guarded_host.py holds the sources against this list)
ROUTED = ("empty", "empty_like", "zeros", "zeros_like", "full", "full_like", "ones", "randn")


class Violation(NamedTuple):
    label: str
    side: str     # "front" | "back"
    offset: int   # first changed byte relative to the payload edge: back 0 = the byte after the payload, front -1 = the byte before it
    count: int    # changed guard bytes on that side


class Unwritten(NamedTuple):
    label: str
    count: int    # elements that still hold the poison pattern
    first: int    # flat index of the first of them
    last: int     # ... and of the last
    numel: int


class _Block:
    __slots__ = ("label", "buf", "start", "nbytes", "tensor", "poisoned", "before")

    def __init__(self, label, buf, start, nbytes, tensor, poisoned):
        self.label, self.buf, self.start, self.nbytes, self.tensor, self.poisoned = label, buf, start, nbytes, tensor, poisoned
        self.before = None  # payload bytes at snapshot() time

    @property
    def payload(self):
        return self.buf[self.start:self.start + self.nbytes]


def _shape(args) -> tuple:
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


class GuardedPool:
    def __init__(self, device):
        self.device = torch.device(device)
        self.blocks: List[_Block] = []

    # ------------------------------------------------------------------ allocation
    def alloc(self, shape, dtype=torch.float32, fill=None, offset_bytes: int = 0, label: Optional[str] = None) -> torch.Tensor:
        """a contiguous tensor between two guards; fill=None leaves the payload poisoned (this is torch.empty)"""
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * item
        row = (shape[-1] if shape else 1) * item
        guard = max(MIN_GUARD, min(GUARD_ROWS * row, MAX_GUARD))
        guard = (guard + ALIGN - 1) // ALIGN * ALIGN
        buf = torch.full((guard + ALIGN + offset_bytes + nbytes + guard,), POISON, dtype=torch.uint8, device=self.device)
        start = guard + (-(buf.data_ptr() + guard)) % ALIGN + offset_bytes
        buf = buf[:start + nbytes + guard]
        t = buf[start:start + nbytes].view(dtype).view(shape)
        assert t.data_ptr() % ALIGN == offset_bytes % ALIGN and t.is_contiguous()
        if fill is not None:
            t.fill_(fill)
        if label is None:
            label = f"#{len(self.blocks)}"
        label = f"{label} {list(shape)} {str(dtype).replace('torch.', '')}"
        self.blocks.append(_Block(label, buf, start, nbytes, t, fill is None))
        return t

    def put(self, src: torch.Tensor, label: str, offset_bytes: int = 0) -> torch.Tensor:
        """an operand: a pool tensor holding a copy of `src` (any device), with the guards around it"""
        t = self.alloc(src.shape, src.dtype, fill=0, offset_bytes=offset_bytes, label=label)
        t.copy_(src)
        return t

    def block_of(self, t: torch.Tensor) -> _Block:
        for b in self.blocks:
            if b.tensor is t:
                return b
        for b in self.blocks:  # a view of the whole payload
            if b.nbytes and b.tensor.data_ptr() == t.data_ptr() and b.nbytes == t.numel() * t.element_size():
                return b
        raise KeyError("not a tensor of this pool")

    def shrink(self, t: torch.Tensor, nbytes: int):
        """bookkeeping only, no byte is touched: treat the last `nbytes` of t's payload as the start of its back guard.  (For
        trying that the checks bite: what a correct kernel wrote there then counts as an overrun.)"""
        self.block_of(t).nbytes -= nbytes

    # ------------------------------------------------------------------ checks
    def violations(self) -> List[Violation]:
        """every guard byte that is no longer 0xFF, per block and side"""
        if not self.blocks:
            return []
        counts = torch.stack([torch.stack(((b.buf[:b.start] != POISON).sum(), (b.buf[b.start + b.nbytes:] != POISON).sum()))
                              for b in self.blocks]).cpu()
        out = []
        for b, (nf, nb) in zip(self.blocks, counts.tolist()):
            if nf:
                bad = (b.buf[:b.start] != POISON).nonzero()
                out.append(Violation(b.label, "front", int(bad[0]) - b.start, int(nf)))
            if nb:
                bad = (b.buf[b.start + b.nbytes:] != POISON).nonzero()
                out.append(Violation(b.label, "back", int(bad[0]), int(nb)))
        return out

    def _poison_mask(self, b: _Block) -> torch.Tensor:
        item = b.tensor.element_size()
        return (b.payload.view(-1, item) == POISON).all(dim=1)

    def unwritten(self, t: torch.Tensor) -> int:
        """elements of a handed-out tensor that still hold the poison pattern (bytewise, not isnan)"""
        b = self.block_of(t)
        return int(self._poison_mask(b).sum()) if b.nbytes else 0

    def unwritten_report(self, skip=()) -> List[Unwritten]:
        """over every tensor handed out poisoned (fill=None), except the blocks in `skip`"""
        todo = [b for b in self.blocks if b.poisoned and b.nbytes and b not in skip]
        if not todo:
            return []
        counts = torch.stack([self._poison_mask(b).sum() for b in todo]).cpu().tolist()
        out = []
        for b, n in zip(todo, counts):
            if n:
                idx = self._poison_mask(b).nonzero().flatten()
                out.append(Unwritten(b.label, int(n), int(idx[0]), int(idx[-1]), b.tensor.numel()))
        return out

    def snapshot(self):
        """remember the payload of every block handed out so far (the operands, before the launch)"""
        for b in self.blocks:
            b.before = b.payload.clone()

    def changed(self) -> List[str]:
        """labels of the snapshotted blocks whose payload is no longer bytewise what it was"""
        todo = [b for b in self.blocks if b.before is not None]
        if not todo:
            return []
        flags = torch.stack([(b.payload != b.before).any() for b in todo]).cpu().tolist()
        return [b.label for b, f in zip(todo, flags) if f]


class TorchProxy:
    """stands in for the name `torch` in a module: every attribute is torch's own, except the functions of ROUTED, which
    allocate from the pool when the tensor is for the pool's device"""

    def __init__(self, pool: GuardedPool, module_name: str = ""):
        self._pool = pool
        self._module = module_name

    def __getattr__(self, name):
        return getattr(torch, name)

    # -- helpers
    def _mine(self, device) -> bool:
        if device is None:
            return self._pool.device.type == "cpu"
        return torch.device(device).type == self._pool.device.type

    def _label(self) -> str:
        f = sys._getframe(1)
        while f.f_back is not None and f.f_globals.get("__name__") == __name__:
            f = f.f_back
        short = self._module.rsplit(".", 1)[-1]
        return f"{short}.{f.f_code.co_name}:{f.f_lineno}"

    @staticmethod
    def _plain(kw):
        # arguments that do not change what the pool has to provide (contiguous, dense, no autograd)
        for k in ("memory_format", "requires_grad", "layout", "pin_memory"):
            kw.pop(k, None)
        return kw

    def _new(self, shape, dtype, fill, kw):
        kw = self._plain(dict(kw))
        kw.pop("device", None)
        if kw:
            raise TypeError(f"guarded torch proxy: unsupported arguments {sorted(kw)}")
        return self._pool.alloc(shape, dtype or torch.get_default_dtype(), fill=fill, label=self._label())

    # -- routed functions
    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._new(_shape(size), dtype, None, kw)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._new(_shape(size), dtype, 0, kw)

    def ones(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.ones(*size, dtype=dtype, device=device, **kw)
        return self._new(_shape(size), dtype, 1, kw)

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        if dtype is None:
            dtype = torch.tensor(fill_value).dtype if not isinstance(fill_value, float) else torch.get_default_dtype()
        return self._new(_shape((size,)), dtype, fill_value, kw)

    def randn(self, *size, dtype=None, device=None, generator=None, **kw):
        if not self._mine(device):
            return torch.randn(*size, dtype=dtype, device=device, generator=generator, **kw)
        return self._new(_shape(size), dtype, 0, kw).normal_(generator=generator)

    def _like(self, t, fill, dtype, device, kw):
        return self._new(tuple(t.shape), dtype or t.dtype, fill, kw)

    def empty_like(self, t, dtype=None, device=None, **kw):
        if not self._mine(device if device is not None else t.device):
            return torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._like(t, None, dtype, device, kw)

    def zeros_like(self, t, dtype=None, device=None, **kw):
        if not self._mine(device if device is not None else t.device):
            return torch.zeros_like(t, dtype=dtype, device=device, **kw)
        return self._like(t, 0, dtype, device, kw)

    def full_like(self, t, fill_value, dtype=None, device=None, **kw):
        if not self._mine(device if device is not None else t.device):
            return torch.full_like(t, fill_value, dtype=dtype, device=device, **kw)
        return self._like(t, fill_value, dtype, device, kw)


@contextlib.contextmanager
def guarded(pool: GuardedPool, *modules):
    """inside the block the given modules allocate from the pool; their `torch` is restored on exit, also on an exception.
    The torch package itself is not touched."""
    saved = []
    try:
        for m in modules:
            saved.append((m, m.__dict__["torch"]))
            m.torch = TorchProxy(pool, m.__name__)
        yield pool
    finally:
        for m, t in saved:
            m.torch = t
