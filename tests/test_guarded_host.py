"""The guarded-memory harness (tests/guarded.py) must be able to fail: fake ops with each kind of fault, as torch indexing on
CPU tensors inside the pool's own buffers.  Nothing here touches a device."""
import ast
import os

import pytest
import torch

from guarded import ALIGN, MAX_GUARD, MIN_GUARD, ROUTED, GuardedPool, TorchProxy, guarded

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vae-channel-dynamics_amd", "src", "vaehip")
DTYPES = [torch.float32, torch.bfloat16, torch.float64, torch.int32]
N = 1000


def _wide(pool, t, before, after):
    """flat typed view of t's payload with `before` / `after` extra elements of its guards: what a kernel's raw pointer sees"""
    b = pool.block_of(t)
    item = t.element_size()
    return b.buf[b.start - before * item:b.start + b.nbytes + after * item].view(t.dtype)


def _operand(pool, dtype):
    src = (torch.arange(N) % 7 + 1).to(dtype)
    return pool.put(src, "x"), src


def _setup(dtype):
    pool = GuardedPool("cpu")
    x, src = _operand(pool, dtype)
    pool.snapshot()
    out = pool.alloc((N,), dtype, label="out")
    return pool, x, src, out


@pytest.mark.parametrize("dtype", DTYPES)
def test_correct_op_reports_nothing(dtype):
    pool, x, src, out = _setup(dtype)
    out.copy_(x * 2)
    assert pool.violations() == [] and pool.unwritten_report() == [] and pool.unwritten(out) == 0 and pool.changed() == []
    assert torch.equal(out, src * 2)
    assert x.data_ptr() % ALIGN == 0 and out.data_ptr() % ALIGN == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_skipped_tail_is_unwritten(dtype):
    pool, x, src, out = _setup(dtype)
    out[:N - 3] = x[:N - 3] * 2
    assert pool.unwritten(out) == 3 and pool.unwritten(x) == 0
    (rep,) = pool.unwritten_report()
    assert rep.label.startswith("out") and (rep.count, rep.first, rep.last, rep.numel) == (3, N - 3, N - 1, N)
    assert pool.violations() == []


@pytest.mark.parametrize("dtype", DTYPES)
def test_store_one_past_the_end(dtype):
    pool, x, src, out = _setup(dtype)
    _wide(pool, out, 0, 1)[:] = torch.cat([x * 2, x[:1]])
    (v,) = pool.violations()
    assert v.label.startswith("out") and (v.side, v.offset, v.count) == ("back", 0, out.element_size())
    assert pool.unwritten_report() == []


@pytest.mark.parametrize("dtype", DTYPES)
def test_store_before_the_start(dtype):
    pool, x, src, out = _setup(dtype)
    out.copy_(x * 2)
    _wide(pool, out, 2, 0)[:2] = x[:2]
    (v,) = pool.violations()
    item = out.element_size()
    assert v.label.startswith("out") and (v.side, v.offset, v.count) == ("front", -2 * item, 2 * item)


@pytest.mark.parametrize("dtype", DTYPES)
def test_store_far_past_the_end(dtype):
    """200 KiB past the end: still inside the guard (MIN_GUARD), so it is seen rather than lost in foreign memory"""
    pool, x, src, out = _setup(dtype)
    out.copy_(x * 2)
    item = out.element_size()
    far = 200 * 1024
    assert far + item <= MIN_GUARD
    _wide(pool, out, 0, far // item + 1)[N + far // item] = 3
    (v,) = pool.violations()
    assert v.label.startswith("out") and (v.side, v.offset, v.count) == ("back", far, item)  # no byte of 3 is 0xFF in any of the formats


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_into_an_input(dtype):
    pool, x, src, out = _setup(dtype)
    out.copy_(x * 2)
    x[5] = 0
    assert pool.changed() == [pool.block_of(x).label] and pool.violations() == []


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_load_past_an_operand_poisons_the_result(dtype):
    """0.0 * x[numel]: with finite garbage behind x this is invisible, with the guard's NaN it is not"""
    pool, x, src, out = _setup(dtype)
    out.copy_(x * 2)
    out[N - 1] += 0.0 * _wide(pool, x, 0, 1)[N]
    assert int((~torch.isfinite(out)).sum()) == 1 and not torch.isfinite(out[N - 1])
    assert pool.violations() == [] and pool.changed() == []


def test_guard_sizes_offsets_and_fill():
    pool = GuardedPool("cpu")
    t = pool.alloc((3, 4096), torch.float32, fill=0, offset_bytes=4)
    b = pool.block_of(t)
    assert t.data_ptr() % ALIGN == 4 and float(t.abs().sum()) == 0.0
    assert b.start >= 128 * 4096 * 4 and b.buf.numel() - b.start - b.nbytes >= 128 * 4096 * 4  # 128 rows of the last dimension
    s = pool.alloc((5,), torch.bfloat16)
    bs = pool.block_of(s)
    assert bs.start >= MIN_GUARD and bs.buf.numel() - bs.start - bs.nbytes >= MIN_GUARD and bs.nbytes == 10
    assert pool.unwritten(s) == 5 and bool(torch.isnan(s).all())
    assert bool(torch.isnan(pool.alloc((2,), torch.float32)).all()) and bool(torch.isnan(pool.alloc((2,), torch.float64)).all())
    assert pool.alloc((2,), torch.int32).tolist() == [-1, -1]
    big = pool.alloc((2, 3_000_000), torch.float32, fill=0)  # a slab with rows of 12 MB: the guards stop growing at MAX_GUARD
    bb = pool.block_of(big)
    assert MAX_GUARD <= bb.start < MAX_GUARD + 2 * ALIGN and bb.buf.numel() - bb.start - bb.nbytes == MAX_GUARD
    e = pool.alloc((0, 7), torch.float32)
    assert e.numel() == 0 and pool.unwritten(e) == 0 and pool.violations() == []


# ------------------------------------------------------------------ the proxy
class _FakeModule:
    """a module-like namespace whose functions say `torch.<name>` the way vaehip's modules do"""

    def __init__(self):
        self.__name__ = "fake.module"
        self.torch = torch

    def work(self, dev="cpu"):
        t = self.torch
        return dict(empty=t.empty((2, 3), device=dev, dtype=t.bfloat16), empty_v=t.empty(2, 3, device=dev), zeros=t.zeros(4, device=dev),
                    ones=t.ones((2, 2), device=dev), full=t.full((3,), float("nan"), device=dev), full_i=t.full((3,), 7, device=dev),
                    empty_like=t.empty_like(t.zeros(5, device=dev)), zeros_like=t.zeros_like(t.ones(5, device=dev), dtype=t.float64),
                    full_like=t.full_like(t.ones(2, device=dev), 3.0), randn=t.randn((4, 4), device=dev, generator=t.Generator().manual_seed(1)))


def test_proxy_routes_allocations_and_forwards_the_rest():
    pool = GuardedPool("cpu")
    m = _FakeModule()
    with guarded(pool, m):
        assert isinstance(m.torch, TorchProxy)
        assert m.torch.float32 is torch.float32 and m.torch.cuda is torch.cuda and m.torch.Tensor is torch.Tensor
        assert m.torch.cat is torch.cat and m.torch.bfloat16 is torch.bfloat16
        got = m.work()
        meta = m.torch.empty((2,), device="meta")  # another device: torch's own allocation
    assert m.torch is torch and meta.device.type == "meta"
    ref = _FakeModule().work()
    for k, t in got.items():
        assert pool.block_of(t) is not None, k
        assert t.shape == ref[k].shape and t.dtype == ref[k].dtype and t.is_contiguous(), k
        if "empty" not in k:
            assert torch.equal(t, ref[k], ) or (k == "full" and bool(torch.isnan(t).all())), k
    assert pool.unwritten(got["empty"]) == 6 and pool.unwritten(got["empty_like"]) == 5 and pool.unwritten(got["zeros"]) == 0
    assert any("work" in b.label for b in pool.blocks)  # labels name the allocation site
    assert pool.violations() == []


def test_guarded_restores_the_modules_after_an_exception():
    pool = GuardedPool("cpu")
    m1, m2 = _FakeModule(), _FakeModule()
    with pytest.raises(RuntimeError):
        with guarded(pool, m1, m2):
            assert isinstance(m1.torch, TorchProxy) and isinstance(m2.torch, TorchProxy)
            raise RuntimeError("boom")
    assert m1.torch is torch and m2.torch is torch
    with pytest.raises(KeyError):  # a module without the name: nothing is left swapped
        with guarded(pool, m1, object.__new__(type("Bare", (), {}))):
            pass
    assert m1.torch is torch


# every torch factory function: a call of one of these in the guarded modules must be one the proxy routes
FACTORIES = {"empty", "empty_like", "empty_strided", "empty_permuted", "zeros", "zeros_like", "ones", "ones_like", "full", "full_like",
             "rand", "rand_like", "randn", "randn_like", "randint", "randint_like", "randperm", "normal", "arange", "range",
             "linspace", "logspace", "eye", "tensor", "as_tensor", "asarray", "scalar_tensor", "from_numpy", "frombuffer",
             "tril_indices", "triu_indices", "sparse_coo_tensor", "hann_window", "hamming_window", "complex", "polar"}
NEW_METHODS = {"new_empty", "new_zeros", "new_ones", "new_full", "new_tensor", "new_empty_strided"}
GUARDED_SOURCES = ["ops.py", "engine.py", "trainer.py", "optim.py"]


def _allocation_calls(path):
    tree = ast.parse(open(path).read(), path)
    found = []
    for node in ast.walk(tree):
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            names = [a.name for a in node.names]
            if isinstance(node, ast.ImportFrom) and node.module == "torch":
                found += [(node.lineno, f"from torch import {n}") for n in names if n in FACTORIES]
            if isinstance(node, ast.Import):
                found += [(node.lineno, f"import {a.name} as {a.asname}") for a in node.names if a.name == "torch" and a.asname]
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
            continue
        f = node.func
        if isinstance(f.value, ast.Name) and f.value.id == "torch" and f.attr in FACTORIES:
            found.append((node.lineno, f.attr))
        elif f.attr in NEW_METHODS:
            found.append((node.lineno, "." + f.attr))
    return found


@pytest.mark.parametrize("name", GUARDED_SOURCES)
def test_every_allocation_in_the_guarded_modules_goes_through_the_proxy(name):
    routed = {n for n in ROUTED if callable(TorchProxy.__dict__.get(n))}
    assert routed == set(ROUTED)
    calls = _allocation_calls(os.path.join(SRC, name))
    escaped = [(line, what) for line, what in calls if what not in routed]
    assert not escaped, f"{name}: allocations the guarded proxy does not route (line, call): {escaped}"
    if name == "ops.py":
        assert len(calls) >= 40  # the parser does see them


def test_the_ast_check_sees_an_escape(tmp_path):
    p = tmp_path / "m.py"
    p.write_text("import torch\ndef f(x):\n    a = torch.arange(3)\n    b = x.new_empty(3)\n    return torch.empty(2), a, b\n")
    assert [w for _, w in sorted(_allocation_calls(str(p)))] == ["arange", ".new_empty", "empty"]
