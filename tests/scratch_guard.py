"""Guarded, pattern-filled allocations for the package's own modules.  TEST INFRASTRUCTURE ONLY.

The library works out of memory that nobody initialised: one torch.empty workspace per batch size, torch.empty scratch of
exactly pl_*_scratch_bytes(...) bytes, torch.empty outputs.  The contract (include/poselift.h):

    every word a kernel reads from workspace, scratch or an output buffer was written earlier in the same call sequence,
    and nothing is written outside the bytes that were asked for.

guarded(pkg, pattern, monkeypatch) makes both halves observable.  While it is active every torch.empty / torch.empty_like
(and torch.empty_strided; the package calls no Tensor.new_empty, which a module-level proxy could not reach) issued BY THE
PACKAGE'S OWN MODULES returns the interior of a larger uint8 buffer:

    [ GUARD bytes | pad to a 256-byte boundary | the tensor's bytes | GUARD bytes ]

and the whole buffer is filled with one byte value, `pattern`.  The same call sequence run under PATTERNS must give
torch.equal results (a difference is a read of a word nobody wrote, or an output element nobody stored), and check()
-- after torch.cuda.synchronize() -- asserts that both guards of every buffer still hold the pattern (a change is a write
outside the bytes asked for), naming the allocation site, the offset of the first changed byte and the buffer's size.

THE GUARD SIZE IS A CONDITION, NOT A MEASUREMENT: a write further than GUARD = 4096 bytes outside an allocation is outside
what this harness claims to see.

Confined to the package: each module of the package gets a thin proxy in place of its `torch` global (monkeypatch.setattr,
undone by pytest); the proxy forwards every attribute but the allocation functions.  The torch module itself is never
patched, so the test's own allocations, torch's internals and every other library are untouched.  Calls under graph capture
are out of scope: capture nothing inside guarded().  Works for device="cpu" as for a GPU."""
import contextlib
import os
import sys
import types

import torch as _torch

GUARD = 4096
ALIGN = 256
PATTERNS = (0x00, 0xFF, 0x7F)


class GuardError(AssertionError):
    pass


def _site(depth):
    f = sys._getframe(depth)
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno}"


class Guard:
    """The bookkeeping of one guarded() block: every buffer handed out stays alive here until the block ends.  empty(),
    empty_like() and empty_strided() are torch's signatures; a test that calls the C ABI itself allocates through them."""

    def __init__(self, pattern):
        assert 0 <= int(pattern) <= 0xFF
        self.pattern = int(pattern)
        self.buffers = []                      # (whole uint8 buffer, interior offset, interior bytes, site)

    # ------------------------------------------------------------------------------------------------ allocation
    def alloc(self, shape, dtype, device, site, strides=None):
        dtype = _torch.get_default_dtype() if dtype is None else dtype
        device = _torch.device("cpu" if device is None else device)
        if device.type == "cuda" and device.index is None:
            device = _torch.device("cuda", _torch.cuda.current_device())
        shape = tuple(int(s) for s in shape)
        item = _torch.empty((), dtype=dtype).element_size()
        if strides is None:
            n = 1
            for s in shape:
                n *= s
        else:
            n = 0 if any(s == 0 for s in shape) else 1 + sum((s - 1) * st for s, st in zip(shape, strides))
        nbytes = n * item
        whole = _torch.full((GUARD + ALIGN + nbytes + GUARD,), self.pattern, dtype=_torch.uint8, device=device)
        off = GUARD + (-(whole.data_ptr() + GUARD)) % ALIGN
        self.buffers.append((whole, off, nbytes, site))
        if strides is None:
            strides = _torch.empty(shape, dtype=dtype, device="meta").stride()
        assert off % item == 0
        # a tensor of its own on the buffer's storage (not an autograd view of it: an autograd node may return it)
        out = _torch.empty(0, dtype=dtype, device=device).set_(whole.untyped_storage(), whole.storage_offset() + off // item,
                                                                 shape, tuple(int(s) for s in strides))
        assert out.data_ptr() % ALIGN == 0 or nbytes == 0
        return out

    def empty(self, *size, dtype=None, device=None, requires_grad=False, pin_memory=False, layout=None,
              memory_format=None, out=None, names=None, _depth=2):
        assert out is None and names is None and layout in (None, _torch.strided), "not supported under the guard"
        assert not pin_memory, "pinned allocations are not guarded"
        if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
            size = tuple(size[0])
        t = self.alloc(size, dtype, device, _site(_depth), strides=self._strides(size, memory_format))
        return t.requires_grad_(True) if requires_grad else t

    def empty_like(self, src, *, dtype=None, device=None, requires_grad=False, pin_memory=False, layout=None,
                   memory_format=None, _depth=2):
        assert layout in (None, _torch.strided) and not pin_memory, "not supported under the guard"
        dtype = src.dtype if dtype is None else dtype
        device = src.device if device is None else device
        mf = _torch.preserve_format if memory_format is None else memory_format
        dense = src.numel() == 0 or 1 + sum((s - 1) * st for s, st in zip(src.shape, src.stride())) == src.numel()
        if mf == _torch.preserve_format and dense and not src.is_contiguous():
            t = self.alloc(src.shape, dtype, device, _site(_depth), strides=src.stride())  # as torch: the source's strides
        else:
            t = self.alloc(src.shape, dtype, device, _site(_depth), strides=self._strides(src.shape, mf))
        return t.requires_grad_(True) if requires_grad else t

    def empty_strided(self, size, stride, *, dtype=None, device=None, requires_grad=False, pin_memory=False, layout=None,
                      _depth=2):
        assert layout in (None, _torch.strided) and not pin_memory, "not supported under the guard"
        t = self.alloc(size, dtype, device, _site(_depth), strides=tuple(stride))
        return t.requires_grad_(True) if requires_grad else t

    @staticmethod
    def _strides(shape, memory_format):
        if memory_format in (_torch.channels_last, _torch.channels_last_3d):
            return _torch.empty(tuple(shape), device="meta", memory_format=memory_format).stride()
        return None

    # ------------------------------------------------------------------------------------------------ the check
    def check(self):
        """Both guards of every buffer still hold the pattern (after a device synchronisation)."""
        if _torch.cuda.is_available() and any(w.is_cuda for w, _, _, _ in self.buffers):
            _torch.cuda.synchronize()
        for whole, off, nbytes, site in self.buffers:
            for name, lo, hi in (("front", 0, off), ("back", off + nbytes, whole.numel())):
                bad = whole[lo:hi] != self.pattern
                if bool(bad.any()):
                    first = int(bad.nonzero()[0, 0]) + lo - off          # relative to the interior's first byte
                    where = f"{-first} bytes in front of" if first < 0 else f"{first - nbytes} bytes past the end of"
                    raise GuardError(
                        f"write outside an allocation made at {site}: first changed byte at offset {first} "
                        f"({where} a buffer of {nbytes} bytes; {int(bad.sum())} guard bytes changed, pattern "
                        f"0x{self.pattern:02X}, {name} guard)")
        return len(self.buffers)


class _TorchProxy(types.ModuleType):
    """Stands where a module's `torch` global stood: everything but the allocation functions is torch's own."""

    def __init__(self, guard):
        super().__init__("torch")
        object.__setattr__(self, "_guard", guard)

    def __getattr__(self, name):                                   # (only what the instance itself does not have)
        return getattr(_torch, name)

    def empty(self, *a, **k):                                      # (_depth: the site is the module's line, not this one)
        return self._guard.empty(*a, _depth=3, **k)

    def empty_like(self, *a, **k):
        return self._guard.empty_like(*a, _depth=3, **k)

    def empty_strided(self, *a, **k):
        return self._guard.empty_strided(*a, _depth=3, **k)


def package_modules(pkg):
    """The package's own loaded modules that hold torch as a global named `torch`."""
    name = pkg.__name__
    mods = [m for n, m in list(sys.modules.items())
            if m is not None and (n == name or n.startswith(name + ".")) and getattr(m, "__dict__", {}).get("torch") is _torch]
    return mods


@contextlib.contextmanager
def guarded(pkg, pattern, monkeypatch, modules=None):
    """with guarded(pkg, 0xFF, monkeypatch) as g: ...; g.check() runs on a clean exit as well.
    pkg: the package (or any module, or a list through `modules`) whose `torch` globals get the proxy."""
    g = Guard(pattern)
    proxy = _TorchProxy(g)
    mods = package_modules(pkg) if modules is None else list(modules)
    assert mods, "no module to guard"
    with monkeypatch.context() as mp:
        for m in mods:
            mp.setattr(m, "torch", proxy)
        yield g
        g.check()
    g.buffers.clear()
