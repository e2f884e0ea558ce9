"""What the poisoned-buffer tests (test_gpu_poisoned_buffers.py, test_poisoned_buffers_cpu.py) share.

Every byte of device memory the library touches is allocated in Python by `torch.empty`, `torch.empty_like` or
`Tensor.new_empty`.  `poisoned(byte)` makes those three return memory whose every byte is `byte`, so a call's result can be
compared, bit for bit, across three different contents of everything it allocated but has not yet written: the library
is deterministic (no float atomics, fixed summation orders), hence no tolerance.  Nothing looks outside a buffer, pads an
allocation or touches the allocator; only what a fresh allocation holds changes.

FILLS: 0x00 is zero; 0xFF an all-ones NaN in fp32 and fp64; 0x7F7F.. a large finite number (3.39e38 in fp32, 1.38e306 in
fp64).  Two non-zero fills because each can be swallowed: a NaN by `fmaxf` or a masking select, a huge finite value by
`exp(-x)` or by a softmax under its running max.  An integer tensor gets 0, 1 or 2 instead: an unwritten integer that is
read then changes the result without indexing far from its buffer."""
import contextlib
import random

import pytest
import torch

FILLS = (0x00, 0xFF, 0x7F)
_INT_FILL = {0x00: 0, 0xFF: 1, 0x7F: 2}
_WORD = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


@contextlib.contextmanager
def device_errors_end_the_session():
    """A kernel form that faults leaves the device unusable: nothing more is launched on it, the session ends there"""
    try:
        yield
    except RuntimeError as err:
        if any(s in str(err) for s in ("HIP error", "CUDA error", "hipError", "illegal memory access")):
            pytest.exit(f"device error, no further test is run: {err}", returncode=3)
        raise


def _fill(t, byte):
    """Sets every byte of the fresh tensor `t` (floating point, complex, uint8), or every element (other integers: 0, 1 or
    2; bool), without touching autograd; -> t"""
    if not isinstance(t, torch.Tensor) or t.layout != torch.strided or t.is_meta or t.numel() == 0:
        return t
    d = t.detach()
    if t.dtype == torch.bool:
        d.fill_(bool(byte))
    elif t.dtype == torch.uint8:
        d.fill_(byte)
    elif t.is_floating_point() or t.is_complex():
        try:
            (d.view(1) if d.dim() == 0 else d).view(torch.uint8).fill_(byte)
        except RuntimeError:      # a layout whose last stride is not 1 (empty_like of a transposed tensor): one element's pattern
            d.copy_(torch.full((t.element_size(),), byte, dtype=torch.uint8).view(t.dtype)[0].to(t.device))
    else:
        d.fill_(_INT_FILL.get(byte, byte % 3))
    return t


@contextlib.contextmanager
def poisoned(byte):
    """For its duration `torch.empty`, `torch.empty_like` and `torch.Tensor.new_empty` return their normal result with
    every byte set to `byte` (integers: see the module's docstring); the originals are put back whatever happens inside."""
    byte = int(byte) & 0xFF
    originals = (torch.empty, torch.empty_like, torch.Tensor.new_empty)

    def empty(*args, **kwargs):
        return _fill(originals[0](*args, **kwargs), byte)

    def empty_like(*args, **kwargs):
        return _fill(originals[1](*args, **kwargs), byte)

    def new_empty(self, *args, **kwargs):
        return _fill(originals[2](self, *args, **kwargs), byte)

    try:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
        yield
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = originals


def words(t):
    """The elements of a tensor as integer words of their size: NaNs compare by their bits"""
    t = t.detach()
    if t.layout != torch.strided:
        t = t.to_dense()
    if t.dtype == torch.bool:
        return t.contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(_WORD[t.element_size()])


def same_bits(a, b):
    """Whether two results hold the same bits: tensors by shape, dtype and integer words; tuples, lists and dicts
    elementwise; None equals None; anything else by =="""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype
                and bool(torch.equal(words(a), words(b))))
    if isinstance(a, dict) or isinstance(b, dict):
        return (isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys()
                and all(same_bits(a[k], b[k]) for k in a))
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        return (isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b)
                and all(same_bits(x, y) for x, y in zip(a, b)))
    return a == b


def differences(a, b, path="result"):
    """The paths at which two results differ in their bits, each with how many elements do: what an assert message names"""
    if isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys():
        return [d for k in a for d in differences(a[k], b[k], f"{path}[{k!r}]")]
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b):
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, f"{path}[{i}]")]
    if same_bits(a, b):
        return []
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype:
        ne = words(a) != words(b)
        where = torch.nonzero(ne)[0].tolist()
        return [f"{path}: {int(ne.sum())} of {ne.numel()} words differ, the first at {where}"]
    return [f"{path}: {a!r} vs {b!r}"]


def nonfinite_where_finite(base, other, path="result"):
    """The paths at which `other` is not finite although `base` (the 0x00 run) is"""
    if isinstance(base, dict):
        return [d for k in base for d in nonfinite_where_finite(base[k], other[k], f"{path}[{k!r}]")]
    if isinstance(base, (tuple, list)):
        return [d for i, (x, y) in enumerate(zip(base, other)) for d in nonfinite_where_finite(x, y, f"{path}[{i}]")]
    if isinstance(base, torch.Tensor) and isinstance(other, torch.Tensor) and base.is_floating_point() \
            and base.shape == other.shape:
        if base.layout != torch.strided:
            base, other = base.to_dense(), other.to_dense()
        bad = torch.isfinite(base) & ~torch.isfinite(other)
        if bool(bad.any()):
            return [f"{path}: {int(bad.sum())} entries not finite where the 0x00 run is finite"]
    return []


def _synchronize():
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()


def run_under_fills(fn, order=None, seed=20260101):
    """`order` None: runs `fn()` once per fill and synchronises after each; -> the three results.

    `order` a sequence of keys: runs `fn(key)` for every key under each fill -- under the first fill in the order given,
    under the second and third in a seeded shuffle of it, so that a result cannot depend on which key ran before it --
    and -> {key: the three results}.  An exception of one key (other than a device error) takes the place of its result:
    the caller raises it for that key alone.  A HIP error ends the session and nothing more is launched."""
    if order is None:
        out = []
        for byte in FILLS:
            with device_errors_end_the_session(), poisoned(byte):
                out.append(fn())
                _synchronize()
        return out
    order = list(order)
    results = {key: [] for key in order}
    rng = random.Random(seed)
    for i, byte in enumerate(FILLS):
        walk = list(order)
        if i:
            rng.shuffle(walk)
        for key in walk:
            with device_errors_end_the_session(), poisoned(byte):
                try:
                    results[key].append(fn(key))
                    _synchronize()
                except Exception as err:          # noqa: BLE001 -- kept for the key's own test to raise
                    if isinstance(err, RuntimeError) and any(s in str(err) for s in ("HIP error", "CUDA error", "hipError",
                                                                                        "illegal memory access")):
                        raise
                    results[key].append(err)
    return results


def check_fills(results, what=""):
    """Asserts that the three results of `run_under_fills` hold the same bits, and are finite wherever the 0x00 run is"""
    for r in results:
        if isinstance(r, BaseException):
            raise r
    failures = []
    for byte, r in zip(FILLS[1:], results[1:]):
        failures += [f"{what} fill 0x{byte:02X} vs 0x00: {d}" for d in differences(results[0], r)]
        failures += [f"{what} fill 0x{byte:02X}: {d}" for d in nonfinite_where_finite(results[0], r)]
    assert not failures, "\n".join(failures[:40])
