"""Buffer contracts made executable: every buffer the package hands the library is guarded and poisoned.

include/codenerf.h words a contract for every pointer: outputs are WRITTEN or ACCUMULATED, accumulators
are zeroed by the caller, a workspace's contents on entry are ignored.  ``contracts(fill)`` checks the two
properties of that contract that no value comparison sees:

  * reading memory nobody wrote.  While the context is active the package modules that allocate for the
    library (``codenerf.ops``, ``codenerf.autograd``, ``codenerf.nerf`` and its render modules,
    ``codenerf.optim``, ``codenerf.train``, ``codenerf.evaluate``) see a stand-in
    for the name ``torch``.  It forwards every attribute to the real module, but ``empty`` / ``empty_like``
    return a tensor whose interior is filled per ``fill``: ``"zero"`` (what fresh device memory usually
    holds) or ``"poison"``: NaN for floating types, the *value* 1 for integer types (``fill_(1)``, not a
    byte pattern: a stale integer used as an offset or a count stays inside every buffer, so the poison
    itself cannot cause an out-of-range access).  A result that differs between the two fills, or holds a
    NaN, read something the kernels never wrote.
  * storing past the end.  Every such tensor (and those of ``zeros`` / ``zeros_like`` / ``full``) sits at
    offset 0 of a larger flat allocation with a trailing guard of 128 KiB (one 128-row tile of 256-float
    rows) that starts right after the interior's last byte and holds a canary.  On exit every guard must equal the
    canary bit for bit; the failure names shape, dtype, call site and the first damaged byte.

Guards are trailing only: interiors keep ``storage_offset() == 0`` and a 256-byte aligned ``data_ptr()``,
which the package asserts in places.  The global ``torch.empty`` is never patched.

The context is also an arena: ``arena.empty(shape, dtype, device)`` gives a test the same guarded,
filled tensor for buffers it owns.  ``n_allocations`` counts what went through the stand-in or the arena,
so a test can assert its calls did not bypass the harness.  ``returns`` logs what every public function of
``codenerf.ops`` returned while the context was active (name, labelled tensors, keyword arguments) in call order,
and after each call a copy of the caller-owned buffers it accumulated into (ACCUMULATED_ARGUMENTS), so two
runs of one case under different fills can be compared output by output (``compare_fills``) without touching
the case's code.
"""
import contextlib
import ctypes
import functools
import importlib
import inspect
import os
import sys
import types

import torch

GUARD_BYTES = 128 * 1024
ALIGN = 256
CANARY = 0xA5
FILLS = ("zero", "poison")
PATCHED_MODULES = ("codenerf.ops", "codenerf.autograd", "codenerf.nerf", "codenerf.optim", "codenerf.train",
                   "codenerf.evaluate") + tuple(
    "codenerf.nerf." + m for m in ("fields", "density", "mesh", "occupancy", "render", "scene", "distributed"))


class GuardError(AssertionError):
    pass


def poison_(t: torch.Tensor) -> torch.Tensor:
    """NaN for floating (and complex) tensors, the value 1 for every other type."""
    if t.numel():
        t.fill_(float("nan") if (t.is_floating_point() or t.is_complex()) else 1)
    return t


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _shape_of(args, kwargs):
    if "size" in kwargs:
        return tuple(int(s) for s in kwargs.pop("size"))
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


def _flat_bytes(total: int, device: torch.device) -> torch.Tensor:
    """``total`` uint8 at offset 0 of their own storage, ``data_ptr()`` a multiple of ALIGN."""
    if device.type != "cpu":
        flat = torch.empty(total, dtype=torch.uint8, device=device)     # the caching allocator aligns to 512
        assert flat.data_ptr() % ALIGN == 0 and flat.storage_offset() == 0
        return flat
    buf = bytearray(total + ALIGN)
    base = ctypes.addressof((ctypes.c_char * len(buf)).from_buffer(buf))
    flat = torch.frombuffer(buf, dtype=torch.uint8, count=total, offset=(-base) % ALIGN)
    assert flat.data_ptr() % ALIGN == 0 and flat.storage_offset() == 0
    return flat


class _Allocation:
    __slots__ = ("flat", "nbytes", "shape", "dtype", "site", "kind")

    def __init__(self, flat, nbytes, shape, dtype, site, kind):
        self.flat, self.nbytes, self.shape, self.dtype, self.site, self.kind = flat, nbytes, shape, dtype, site, kind

    def describe(self):
        return f"{self.kind}{self.shape} {self.dtype} allocated at {self.site}"


class _TorchStandIn(types.ModuleType):
    """Forwards every attribute to the real ``torch`` except the allocating factories."""

    def __init__(self, arena):
        super().__init__("torch")
        self.__dict__["_arena"] = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, dtype=None, device=None, **kw):
        _plain(kw)
        return self._arena._allocate(_shape_of(args, kw), dtype, device, "empty", self._arena.fill)

    def empty_like(self, t, dtype=None, device=None, **kw):
        _plain(kw)
        return self._arena._allocate(tuple(t.shape), dtype or t.dtype, device or t.device, "empty_like",
                                     self._arena.fill)

    def zeros(self, *args, dtype=None, device=None, **kw):
        _plain(kw)
        return self._arena._allocate(_shape_of(args, kw), dtype, device, "zeros", 0)

    def zeros_like(self, t, dtype=None, device=None, **kw):
        _plain(kw)
        return self._arena._allocate(tuple(t.shape), dtype or t.dtype, device or t.device, "zeros_like", 0)

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        _plain(kw)
        if dtype is None:                 # torch.full's inference: the fill value's own type
            dtype = fill_value.dtype if isinstance(fill_value, torch.Tensor) else torch.tensor(fill_value).dtype
        return self._arena._allocate(tuple(int(s) for s in size), dtype, device, "full", fill_value)


def _plain(kw):
    """The stand-in builds contiguous, strided tensors that do not require grad; anything else is a call the
    harness does not model and must not silently mis-serve."""
    for k, v in kw.items():
        ok = (k == "requires_grad" and not v) or (k == "pin_memory" and not v) or \
             (k == "memory_format" and v in (torch.contiguous_format, torch.preserve_format)) or \
             (k == "layout" and v == torch.strided)
        if not ok:
            raise TypeError(f"tests/buffers.py: unsupported factory argument {k}={v!r}")


def _tensors(value, out, path=""):
    """The tensors of a (nested) return value as (label, tensor) pairs: the label is the path of dict keys and
    sequence positions to the tensor ("0.d_ro", "param_grads.3"), so a comparison picks outputs by name."""
    if isinstance(value, torch.Tensor):
        out.append((path, value))
    elif isinstance(value, dict):
        for k in value:
            _tensors(value[k], out, f"{path}.{k}" if path else str(k))
    elif isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            _tensors(v, out, f"{path}.{i}" if path else str(i))
    return out


class Arena:
    def __init__(self, fill: str, inside=()):
        assert fill in FILLS, fill
        self.fill = fill
        self.n_allocations = 0
        self.returns = []                     # (ops function name, [(label, tensor)], kwargs) in call order
        self._inside = set(inside)          # module (or top-level package) names whose frames are call sites
        self._allocations = []

    # ---- allocation
    def _site(self) -> str:
        """file:line of the innermost frame inside the package (else of the arena's caller)."""
        outside = None
        fr = sys._getframe(1)
        while fr is not None:
            name = fr.f_globals.get("__name__", "")
            if name != __name__:
                where = f"{os.path.basename(fr.f_code.co_filename)}:{fr.f_lineno}"
                if name in self._inside or name.split(".")[0] in self._inside:
                    return where
                outside = outside or where
            fr = fr.f_back
        return outside or "?"

    def _allocate(self, shape, dtype, device, kind, value):
        dtype = dtype or torch.get_default_dtype()
        device = torch.device(device) if device is not None else torch.device("cpu")
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        nbytes = _numel(shape) * torch.empty(0, dtype=dtype).element_size()
        total = (nbytes + ALIGN - 1) // ALIGN * ALIGN + GUARD_BYTES
        flat = _flat_bytes(total, device)
        flat.fill_(CANARY)
        t = flat[:nbytes].view(dtype).view(shape)
        if value == "poison":
            poison_(t)
        elif t.numel():
            t.fill_(0 if value == "zero" else value)
        assert t.storage_offset() == 0 and (t.numel() == 0 or t.data_ptr() == flat.data_ptr())
        self._allocations.append(_Allocation(flat, nbytes, tuple(shape), dtype, self._site(), kind))
        self.n_allocations += 1
        return t

    def empty(self, shape, dtype=torch.float32, device="cpu"):
        """A guarded tensor filled per the arena's ``fill``, for a buffer the test owns."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        return self._allocate(shape, dtype, device, "arena.empty", self.fill)

    # ---- checking
    def check_guards(self):
        """Every guard equals its canary bit for bit (the bytes from the interior's end to the allocation's)."""
        damaged = []
        for a in self._allocations:
            guard = a.flat[a.nbytes:]
            bad = guard != CANARY
            if bool(bad.any()):
                first = int(bad.nonzero()[0])
                damaged.append(f"{a.describe()}: guard damaged, first at byte {a.nbytes + first} "
                               f"({first} past the end of the {a.nbytes}-byte interior), "
                               f"{int(bad.sum())} bytes in all")
        if damaged:
            raise GuardError("store past the end of a buffer:\n  " + "\n  ".join(damaged))


# Caller-owned buffers the package's functions ADD into: logged (as copies, taken when the call returns)
# beside what the call returned.  ``fields`` is field_backward_train_multi's list of per-field dicts.
ACCUMULATED_ARGUMENTS = ("param_grads", "g_code", "ray_into", "dz_into", "d_rd_into")


def _accumulated(fn, args, kwargs):
    try:
        given = inspect.signature(fn).bind_partial(*args, **kwargs).arguments
    except TypeError:
        return []
    out = []
    for name in ACCUMULATED_ARGUMENTS:
        _tensors(given.get(name), out, name)
    for i, f in enumerate(given.get("fields") or ()):
        if isinstance(f, dict):
            for name in ACCUMULATED_ARGUMENTS:
                _tensors(f.get(name), out, f"{i}.{name}")
    return [(label, t.detach().clone()) for label, t in out]


def _logged(arena, name, fn):
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        out = fn(*args, **kwargs)
        arena.returns.append((name, _tensors(out, []), dict(kwargs)))
        acc = _accumulated(fn, args, kwargs)
        if acc:
            arena.returns.append((name + " (accumulated)", acc, dict(kwargs)))
        return out
    return wrapper


@contextlib.contextmanager
def contracts(fill: str, modules=PATCHED_MODULES, log_returns_of="codenerf.ops"):
    """See the module docstring.  ``modules``: importable names or module objects whose global ``torch`` is
    replaced for the duration; ``log_returns_of``: the module whose public functions' returns are logged."""
    mods = [importlib.import_module(m) if isinstance(m, str) else m for m in modules]
    arena = Arena(fill, inside={m.__name__.split(".")[0] for m in mods})
    stand_in = _TorchStandIn(arena)
    undo = []
    for m in mods:
        if m.__dict__.get("torch") is not torch:
            raise AssertionError(f"{m.__name__} holds no plain `torch` global to stand in for")
        undo.append((m, "torch", torch))
        m.torch = stand_in
    logged = None
    if log_returns_of is not None:
        logged = importlib.import_module(log_returns_of) if isinstance(log_returns_of, str) else log_returns_of
        if logged in mods:
            for name, fn in list(vars(logged).items()):
                if isinstance(fn, types.FunctionType) and not name.startswith("_") and fn.__module__ == logged.__name__:
                    undo.append((logged, name, fn))
                    setattr(logged, name, _logged(arena, name, fn))
    try:
        yield arena
        if any(a.flat.is_cuda for a in arena._allocations):
            torch.cuda.synchronize()
        arena.check_guards()
    finally:
        for m, name, orig in reversed(undo):
            setattr(m, name, orig)
        arena._allocations = []               # the checks end with the context; the tensors live on


# ---------------------------------------------------------------- comparing two runs' logs


def tensor_bytes(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bytes, flat."""
    t = t.detach().contiguous().reshape(-1)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.view(torch.uint8) if t.numel() else t


def compare_fills(zero, poison, outputs_of=None, exception_for=None, bounds=None, close=None):
    """``zero`` and ``poison``: the ``returns`` logs of one case under the two fills.  The same calls in the same
    order, and every logged tensor bitwise equal between them (NaNs included), except where
    ``exception_for(name, label, kwargs)`` names a key of ``bounds``: then the NaN positions must still agree
    and, with ``bounds[key]`` a number, ``close(poison, zero, bound, what)`` must hold; with None the values
    are not compared.  ``outputs_of(name, pairs, kwargs)`` reduces a call's logged (label, tensor) pairs to
    what of them is documented output.  Returns the set of keys used."""
    assert [r[0] for r in zero] == [r[0] for r in poison], "the two runs made different calls"
    used = set()
    for (name, za, kw), (_, pa, _) in zip(zero, poison):
        if outputs_of is not None:
            za, pa = outputs_of(name, za, kw), outputs_of(name, pa, kw)
        assert [label for label, _ in za] == [label for label, _ in pa], (name, "different outputs")
        for (label, a), (_, b) in zip(za, pa):
            assert a.shape == b.shape and a.dtype == b.dtype, (name, label)
            if torch.equal(tensor_bytes(a), tensor_bytes(b)):
                continue
            key = exception_for(name, label, kw) if exception_for is not None else None
            if key is None:
                fa, fb = a.reshape(-1), b.reshape(-1)
                diff = fa != fb
                if a.is_floating_point():
                    diff = diff | (torch.isnan(fa) != torch.isnan(fb))
                nan = int(torch.isnan(fb).sum()) if b.is_floating_point() else 0
                first = int(diff.nonzero()[0]) if bool(diff.any()) else 0
                raise AssertionError(
                    f"{name}: {label} {tuple(a.shape)} {a.dtype} depends on what its buffers held: "
                    f"{int(diff.sum())} of {a.numel()} elements differ, first at flat index {first} "
                    f"(zero fill {fa[first].item()!r}, poison {fb[first].item()!r}), {nan} NaN under poison")
            used.add(key)
            if a.is_floating_point():
                assert torch.equal(torch.isnan(a), torch.isnan(b)), (name, label, "NaN under one fill only")
            if bounds[key] is not None:
                close(b, a.double(), bounds[key], f"{name} {label} between fills ({key})")
    return used
