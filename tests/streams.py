"""Where the work is enqueued, made checkable: every ``codenerf.ops`` call under a side stream, and every call
captured in a graph and replayed.

The wrappers promise to launch "on the current stream" (codenerf/ops.py, include/codenerf.h).  A launch with a
forgotten stream argument, a helper that synchronises or allocates, a wrapper that reads a device value on
the host: none of them changes a value while everything runs on the default stream.  Two checks, both built
like tests/buffers.py (the public functions of ``codenerf.ops`` are wrapped for the duration of a context,
``buffers._tensors`` labels what they return, ``buffers.ACCUMULATED_ARGUMENTS`` names the caller-owned buffers
they add into, ``buffers.compare_fills`` compares two logs); the global ``torch`` is never patched.

(a) ``side_stream()``: the case runs under a side stream (``concurrent_streams``: one shown to run while the
    default stream is busy).  Before every ops call a bounded
    spin (``torch.cuda._sleep``, a single-thread kernel that counts cycles; nothing waits on a flag) is enqueued on
    the DEFAULT stream; right after the call returns, what it returned and what it accumulated into is copied on
    the current stream.  A launch that strayed onto the default stream sits behind the spin, so the copy misses
    its writes; nested in ``buffers.contracts("poison")`` an output no side-stream kernel wrote holds NaN.
    ``compare_logs`` then holds the log against the same case's log from ``plain()`` (the default stream), bit
    for bit.  Per call the check is conclusive only if the spin ended after the copies had finished: read from
    event timestamps, retried once with a spin four times longer, else ``Inconclusive``.  Only outermost calls
    are spun and checked (a wrapper's own calls of other wrappers are logged in place: waiting for a spin of
    theirs would outlast the outer one).

(b) ``capture_replay()``: each distinct call ``plain(record=True)`` recorded (name, arguments as they were
    before the call, what the call gave) is captured alone in a ``torch.cuda.CUDAGraph`` on one stream in global
    error mode -- a launch on another stream, a hidden synchronisation or a hidden allocation raise there
    (``Refused``) -- then twice: every output poisoned, every argument put back, replay, and the eager bits
    required.  Work that ran at capture time but never entered the graph leaves the poison in place.
"""
import contextlib
import functools
import gc
import importlib
import inspect
import time
import types

import torch

import buffers as B

SPIN_MS = 2.0                 # per call at least; a case's kernels mostly take microseconds
SPIN_PER_WALL = 4.0           # and this many times what the same call took, host and device, in the plain run
RETRY_FACTOR = 4
WHOLE_STORAGE_LIMIT = 2 << 30     # (the fp32 training forward's (M, 5 x 256 + 64) save buffer at M = 67584: 363 MB)


class Inconclusive(AssertionError):
    """The spin on the default stream ended before the side stream's copies had finished: nothing was shown."""


class Refused(RuntimeError):
    """A call raised while it was being captured."""


# ---------------------------------------------------------------- the spin

_CYCLES_PER_MS = {}


def cycles_per_ms(device=None) -> float:
    """``torch.cuda._sleep`` cycles per millisecond, measured once per process and device against events."""
    key = torch.cuda.current_device() if device is None else torch.device(device).index
    if key not in _CYCLES_PER_MS:
        with torch.cuda.device(key):
            torch.cuda._sleep(100_000)            # the kernel's first launch
            torch.cuda.synchronize()
            best = None
            for n in (2_000_000, 20_000_000):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                torch.cuda._sleep(n)
                b.record()
                b.synchronize()
                best = n / max(a.elapsed_time(b), 1e-3)
            _CYCLES_PER_MS[key] = best
    return _CYCLES_PER_MS[key]


def spin(stream, ms: float):
    """A spin of about ``ms`` on ``stream`` -> the timed event recorded right behind it."""
    end = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * cycles_per_ms(stream.device)))
        end.record(stream)
    return end


# ---------------------------------------------------------------- streams that do run beside one another
#
# A process has a few hardware queues (HIP's default is four) for all its streams.  Were two streams to share
# one, a spin on one would hold the other back and no check built on the spin could be conclusive.  The checks
# therefore take their streams from here: streams shown, by the spin itself, to finish work while the default
# stream and while each other are busy.

_CONCURRENT = []


def runs_beside(busy, other, ms=1.0) -> bool:
    """Does work on ``other`` finish while ``busy`` still spins?"""
    torch.cuda.synchronize()
    end = spin(busy, ms)
    with torch.cuda.stream(other):
        done = torch.cuda.Event()
        torch.zeros(8, device=busy.device).add_(1.0)
        done.record()
    done.synchronize()
    beside = not end.query()
    torch.cuda.synchronize()
    return beside


def concurrent_streams(n: int):
    """``n`` streams, the same ones every time, each of which runs beside the default stream and beside the
    others.  Fails if the pool's streams do not hold that many."""
    default = torch.cuda.default_stream()
    tried = 0
    while len(_CONCURRENT) < n and tried < 32:
        tried += 1
        s = torch.cuda.Stream()
        if any(s == t for t in _CONCURRENT):
            continue
        with torch.cuda.stream(s):                       # the stream's first launch, outside the measurement
            torch.zeros(8, device=s.device).add_(1.0)
        if all(runs_beside(b, s) and runs_beside(s, b) for b in [default] + _CONCURRENT):
            _CONCURRENT.append(s)
    assert len(_CONCURRENT) >= n, f"found {len(_CONCURRENT)} streams that run beside the default stream, need {n}"
    return _CONCURRENT[:n]


# ---------------------------------------------------------------- copies that keep storage and aliasing


def _storage_bytes(t):
    st = t.untyped_storage()
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(st, 0, (st.nbytes(),), (1,))


class Snapshot:
    """Copies of tensors, one per storage: the whole storage is copied (so a view keeps what lies beside it --
    the fp32 training forward's encoding plane behind ``saved``, a guard) and views of one storage stay views
    of one copy.  ``map`` copies every tensor of a nested value; ``restore`` writes the copies back into the
    originals; ``refresh`` copies the originals again."""

    def __init__(self):
        self._by_storage = {}            # storage pointer -> (live bytes, copied bytes)
        self._views = []                 # (live tensor, clone): storages too large to copy whole

    def of(self, t: torch.Tensor) -> torch.Tensor:
        t = t.detach()
        st = t.untyped_storage()
        if st.nbytes() == 0 or st.nbytes() > WHOLE_STORAGE_LIMIT:
            c = t.clone()
            self._views.append((t, c))
            return c
        key = (t.device, st.data_ptr())
        if key not in self._by_storage:
            live = _storage_bytes(t)
            self._by_storage[key] = (live, live.clone())
        copy = self._by_storage[key][1]
        return torch.empty(0, dtype=t.dtype, device=t.device).set_(copy.untyped_storage(), t.storage_offset(),
                                                                   t.shape, t.stride())

    def map(self, value):
        if isinstance(value, torch.Tensor):
            return self.of(value)
        if isinstance(value, dict):
            return {k: self.map(v) for k, v in value.items()}
        if isinstance(value, tuple) and hasattr(value, "_fields"):
            return type(value)(*[self.map(v) for v in value])
        if isinstance(value, (list, tuple)):
            return type(value)(self.map(v) for v in value)
        return value

    def pairs(self, pairs):
        return [(label, self.of(t)) for label, t in pairs]

    def restore(self):
        for live, copy in self._by_storage.values():
            live.copy_(copy)
        for live, copy in self._views:
            live.copy_(copy)

    def refresh(self):
        for live, copy in self._by_storage.values():
            copy.copy_(live)
        for live, copy in self._views:
            copy.copy_(live)


def accumulated(fn, args, kwargs):
    """The caller-owned buffers ``fn`` adds into, as (label, tensor) pairs of the tensors themselves
    (buffers._accumulated gives copies of the same)."""
    try:
        given = inspect.signature(fn).bind_partial(*args, **kwargs).arguments
    except TypeError:
        return []
    out = []
    for name in B.ACCUMULATED_ARGUMENTS:
        B._tensors(given.get(name), out, name)
    fields = given.get("fields")
    for i, f in enumerate(fields if isinstance(fields, (list, tuple)) else ()):
        if isinstance(f, dict):
            for name in B.ACCUMULATED_ARGUMENTS:
                B._tensors(f.get(name), out, f"{i}.{name}")
    return out


# ---------------------------------------------------------------- wrapping the public functions


class Record:
    """One outermost call of an eager run: the function, its arguments as they were before the call (copies),
    and copies of what it returned and accumulated into."""
    __slots__ = ("name", "fn", "args", "kwargs", "out", "acc")

    def __init__(self, name, fn, args, kwargs, out, acc):
        self.name, self.fn, self.args, self.kwargs, self.out, self.acc = name, fn, args, kwargs, out, acc

    def key(self):
        """What makes two calls the same call: name, tensor shapes and types, everything else by value."""
        return (self.name, _describe(self.args), _describe(self.kwargs))


def _describe(v):
    if isinstance(v, torch.Tensor):
        return ("tensor", tuple(v.shape), str(v.dtype), v.device.type)
    if isinstance(v, dict):
        return tuple((str(k), _describe(v[k])) for k in sorted(v, key=str))
    if isinstance(v, (list, tuple)):
        return (type(v).__name__,) + tuple(_describe(x) for x in v)
    if isinstance(v, (bool, int, float, str, type(None))):
        return repr(v)
    shape = getattr(v, "shape", None)
    return (type(v).__name__, tuple(shape) if shape is not None else None)


class Log:
    def __init__(self):
        self.returns = []          # (name, [(label, copy)], kwargs), the layout of buffers.Arena.returns
        self.records = []          # Record per outermost call (plain(record=True))
        self.slack_ms = []         # side_stream: per call, how long the spin outlasted the copies
        self.wall_ms = []          # plain: per outermost call, host time from the call to its copies' completion
        self.retries = 0
        self.depth = 0
        self.stream = None         # side_stream: the stream the case runs under


def _public(module):
    return [(name, fn) for name, fn in list(vars(module).items())
            if isinstance(fn, types.FunctionType) and not name.startswith("_") and fn.__module__ == module.__name__]


@contextlib.contextmanager
def _wrapped(module, make):
    module = importlib.import_module(module) if isinstance(module, str) else module
    undo = []
    try:
        for name, fn in _public(module):
            undo.append((name, fn))
            setattr(module, name, make(name, fn))
        yield
    finally:
        for name, fn in reversed(undo):
            setattr(module, name, fn)


def _log_call(log, name, fn, args, kwargs, out):
    snap = Snapshot()
    pairs = snap.pairs(B._tensors(out, []))
    acc = snap.pairs(accumulated(fn, args, kwargs))
    log.returns.append((name, pairs, dict(kwargs)))
    if acc:
        log.returns.append((name + " (accumulated)", acc, dict(kwargs)))
    return pairs, acc


@contextlib.contextmanager
def plain(module="codenerf.ops", record=False):
    """Log every call of ``module``'s public functions on whatever stream is current (the default one)."""
    log = Log()

    def make(name, fn):
        @functools.wraps(fn)
        def wrapper(*args, **kwargs):
            log.depth += 1
            try:
                before = None
                if record and log.depth == 1:
                    before = Snapshot().map((args, dict(kwargs)))
                t0 = time.perf_counter()
                out = fn(*args, **kwargs)
                pairs, acc = _log_call(log, name, fn, args, kwargs, out)
                if log.depth == 1:
                    torch.cuda.current_stream().synchronize()
                    log.wall_ms.append(1e3 * (time.perf_counter() - t0))
                if before is not None:
                    log.records.append(Record(name, fn, before[0], before[1], pairs, acc))
                return out
            finally:
                log.depth -= 1
        return wrapper

    with _wrapped(module, make):
        yield log
    torch.cuda.synchronize()


@contextlib.contextmanager
def side_stream(module="codenerf.ops", spin_ms=SPIN_MS, stream=None, wall_ms=()):
    """See the module docstring, (a).  The body runs with ``stream`` (else concurrent_streams(1)'s) current.
    ``wall_ms``: the plain run's ``Log.wall_ms``; outermost call i spins for max(spin_ms, SPIN_PER_WALL x
    wall_ms[i]), so a call whose own work takes milliseconds (a training backward over 10^5 rows) is not
    inconclusive by construction.  Python's collector is held off inside a call's window: a pass over a long
    session's heap takes longer than a spin."""
    calls = [0]
    log = Log()
    log.stream = concurrent_streams(1)[0] if stream is None else stream
    default = torch.cuda.default_stream()

    def make(name, fn):
        @functools.wraps(fn)
        def wrapper(*args, **kwargs):
            assert torch.cuda.current_stream() == log.stream, "the case left the side stream"
            if log.depth:                 # a call made by a wrapped call: inside its spin, logged in its place
                out = fn(*args, **kwargs)
                _log_call(log, name, fn, args, kwargs, out)
                return out
            before = Snapshot()
            before.map((args, kwargs))
            base = spin_ms
            if calls[0] < len(wall_ms):
                base = max(base, SPIN_PER_WALL * wall_ms[calls[0]])
            calls[0] += 1
            log.depth += 1
            collecting = gc.isenabled()
            gc.disable()
            try:
                mark = len(log.returns)
                out = None
                for factor in (1, RETRY_FACTOR):
                    if factor != 1:
                        out = None                    # (its blocks go back to the stream's cache)
                        del log.returns[mark:]        # the first attempt's log, the calls it made itself included
                        before.restore()              # on the current stream: the call runs again from the same state
                        log.retries += 1
                    spin_end = spin(default, base * factor)
                    out = fn(*args, **kwargs)
                    _log_call(log, name, fn, args, kwargs, out)
                    copied = torch.cuda.Event(enable_timing=True)
                    copied.record()                   # the current stream: behind the copies
                    copied.synchronize()
                    spin_end.synchronize()
                    slack = copied.elapsed_time(spin_end)
                    if slack > 0:
                        log.slack_ms.append(slack)
                        return out
                raise Inconclusive(f"{name}: the default stream's {base * RETRY_FACTOR:.1f} ms spin ended "
                                   f"{-slack:.3f} ms before the copies had finished")
            finally:
                log.depth -= 1
                if collecting:
                    gc.enable()
        return wrapper

    cycles_per_ms()
    torch.cuda.synchronize()
    with _wrapped(module, make):
        with torch.cuda.stream(log.stream):
            yield log
    torch.cuda.synchronize()


def compare_logs(plain_log, other_log, what, outputs_of=None, exception_for=None, bounds=None, close=None):
    """buffers.compare_fills on two logs (the same calls, every logged tensor bitwise equal but for the named
    exceptions), the failure worded for this harness."""
    try:
        return B.compare_fills(plain_log, other_log, outputs_of, exception_for, bounds, close)
    except AssertionError as e:
        raise AssertionError(f"{what} differs from the default-stream run (left: default stream, right: {what}; "
                             f"NaN: nothing on that stream wrote it before the copy): {e}") from None


# ---------------------------------------------------------------- (b) capture and replay


def distinct(records):
    seen, out = set(), []
    for r in records:
        k = r.key()
        if k not in seen:
            seen.add(k)
            out.append(r)
    return out


def capture(call):
    """``call()`` captured alone on a fresh stream in global error mode -> (graph, what it returned).  Anything
    the call raises (and whatever ending the broken capture raises) becomes ``Refused``."""
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        graph.capture_begin(capture_error_mode="global")
        try:
            out = call()
        except Exception as e:
            try:
                graph.capture_end()
            except Exception:
                pass
            raise Refused(f"{type(e).__name__}: {e}") from None
        try:
            graph.capture_end()
        except Exception as e:
            raise Refused(f"{type(e).__name__}: {e}") from None
    torch.cuda.synchronize()
    return graph, out


def capture_replay(rec, outputs_of=None, exception_for=None, bounds=None, close=None, replays=2):
    """See the module docstring, (b): ``rec`` (a Record) captured and replayed ``replays`` times."""
    work = Snapshot()                                 # the recorded arguments stay as they were
    args, kwargs = work.map((rec.args, rec.kwargs))
    graph, out = capture(lambda: rec.fn(*args, **kwargs))
    produced = B._tensors(out, [])
    eager = [(rec.name, rec.out, rec.kwargs)]
    if rec.acc:
        eager.append((rec.name + " (accumulated)", rec.acc, rec.kwargs))
    for i in range(replays):
        for _, t in produced:
            B.poison_(t)
        work.refresh()                                # every argument as before the call (an output may be one)
        graph.replay()
        torch.cuda.synchronize()
        got = [(rec.name, produced, rec.kwargs)]
        acc = accumulated(rec.fn, args, kwargs)
        if acc:
            got.append((rec.name + " (accumulated)", acc, rec.kwargs))
        compare_logs(eager, got, f"replay {i + 1} of the captured {rec.name}", outputs_of, exception_for, bounds, close)
    return graph
