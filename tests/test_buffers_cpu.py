"""The buffer-contract harness of tests/buffers.py fails when it should: toy "ops" in plain torch that
allocate through a module patched the same way as the package's.

``stale_sum`` sums a workspace in which it wrote all rows but one, ``overrun`` stores one element past its
view, ``unwritten`` leaves an output element unwritten, ``correct`` does none of that.  The first three fail
under ``poison``; the first two pass under ``zero``, which is why zero-filled (fresh) memory hides them."""
import sys
import types

import pytest
import torch

import buffers as B

TOY_SOURCE = '''
import torch


def stale_sum(x):
    """Row sums of x (n, k) through an (n + 1)-row workspace whose last row no one writes."""
    ws = torch.empty(x.shape[0] + 1, x.shape[1], dtype=x.dtype)
    ws[:-1] = x
    return ws.sum(dim=0)


def overrun(x):
    """A copy of x (n,) whose store runs one element past the end of the output."""
    out = torch.empty(x.shape[0], dtype=x.dtype)
    wide = out.as_strided((x.shape[0] + 1,), (1,))
    wide[:-1] = x
    wide[-1] = 7
    return out


def unwritten(x):
    """A copy of x (n,) that never writes its last element."""
    out = torch.empty_like(x)
    out[:-1] = x[:-1]
    return out


def correct(x):
    """Row sums of x through a fully written workspace, plus a zeroed accumulator and a full()."""
    ws = torch.empty(x.shape[0], x.shape[1], dtype=x.dtype)
    ws.copy_(x)
    acc = torch.zeros(x.shape[1], dtype=x.dtype)
    acc += ws.sum(dim=0)
    return acc + torch.full((x.shape[1],), 0.0, dtype=x.dtype) + torch.zeros_like(acc)


def raw(shape, dtype):
    return torch.empty(shape, dtype=dtype)


def noisy(x, d_rd_into=None):
    """A dict of outputs: "exact" is x, "sum" is x plus an unwritten tail element; adds x into ``d_rd_into``."""
    out = torch.empty(x.shape[0] + 1, dtype=x.dtype)
    out[:-1] = x
    if d_rd_into is not None:
        d_rd_into += x
    return {"exact": x.clone(), "sum": out}
'''


@pytest.fixture()
def toy():
    mod = types.ModuleType("buffers_toy_ops")
    sys.modules[mod.__name__] = mod
    exec(compile(TOY_SOURCE, "buffers_toy_ops.py", "exec"), mod.__dict__)
    yield mod
    del sys.modules[mod.__name__]


def ctx(toy, fill):
    return B.contracts(fill, modules=(toy,), log_returns_of=toy)


X = torch.arange(1.0, 13.0).reshape(4, 3)
V = torch.arange(1.0, 6.0)


def test_stale_workspace_read_fails_only_under_poison(toy):
    with ctx(toy, "zero") as arena:
        got = toy.stale_sum(X)
    assert arena.n_allocations > 0
    assert torch.equal(got, X.sum(dim=0))                 # zero-filled memory hides the stale row
    with ctx(toy, "poison") as arena:
        got = toy.stale_sum(X)
    assert arena.n_allocations > 0
    assert bool(torch.isnan(got).all())
    assert not torch.equal(got, X.sum(dim=0))


@pytest.mark.parametrize("fill", B.FILLS)
def test_store_past_the_end_trips_the_guard(toy, fill):
    with pytest.raises(B.GuardError) as info:
        with ctx(toy, fill) as arena:
            got = toy.overrun(V)
            assert torch.equal(got, V)                    # the values themselves are right
            assert arena.n_allocations > 0
    msg = str(info.value)
    assert "(5,)" in msg and "torch.float32" in msg and "buffers_toy_ops.py:" in msg
    assert "first at byte 20 " in msg                     # 5 floats, then the first damaged byte


def test_unwritten_output_fails_under_poison(toy):
    with ctx(toy, "zero") as arena:
        zero = toy.unwritten(V)
    assert arena.n_allocations > 0
    with ctx(toy, "poison") as arena:
        poison = toy.unwritten(V)
    assert arena.n_allocations > 0
    assert torch.equal(zero[:-1], V[:-1]) and torch.equal(poison[:-1], V[:-1])
    assert bool(torch.isnan(poison[-1])) and not bool(torch.isnan(zero[-1]))
    assert not torch.equal(zero, poison)


@pytest.mark.parametrize("fill", B.FILLS)
def test_correct_op_passes(toy, fill):
    with ctx(toy, fill) as arena:
        got = toy.correct(X)
    assert arena.n_allocations == 4
    assert torch.equal(got, X.sum(dim=0))
    assert [r[0] for r in arena.returns] == ["correct"]
    assert arena.returns[0][1][0][0] == "" and torch.equal(arena.returns[0][1][0][1], got)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(0,), (1,), (7, 3), (129, 257)])
def test_fill_values_alignment_and_offset(toy, dtype, shape):
    for fill in B.FILLS:
        with ctx(toy, fill) as arena:
            t = toy.raw(shape, dtype)
            own = arena.empty(shape, dtype)
        assert arena.n_allocations == 2
        for u in (t, own):
            assert u.shape == shape and u.dtype == dtype and u.is_contiguous()
            assert u.data_ptr() % 256 == 0
            assert u.storage_offset() == 0
            if fill == "zero":
                assert not bool(u.any())
            elif dtype.is_floating_point:
                assert bool(torch.isnan(u).all())
            else:
                assert bool((u == 1).all())               # the value 1, not a byte pattern


def test_guard_is_128_kib_of_canary_right_behind_the_interior(toy):
    with ctx(toy, "poison") as arena:
        t = toy.raw((5,), torch.float32)
        a = arena._allocations[0]
        assert a.nbytes == 20 and a.flat.data_ptr() == t.data_ptr()
        assert a.flat.numel() - a.nbytes >= B.GUARD_BYTES
        assert bool((a.flat[20:] == B.CANARY).all())
        assert a.site.startswith("buffers_toy_ops.py:")


def test_stand_in_forwards_and_is_removed(toy):
    real_empty = torch.empty
    with ctx(toy, "poison"):
        assert toy.torch is not torch
        assert toy.torch.float32 is torch.float32 and toy.torch.Tensor is torch.Tensor
        assert torch.empty is real_empty                  # the global factory is never patched
    assert toy.torch is torch
    with pytest.raises(RuntimeError):
        with ctx(toy, "poison"):
            raise RuntimeError("body failed")
    assert toy.torch is torch and toy.correct.__name__ == "correct"


# ---------------------------------------------------------------- compare_fills


def _close(got, ref, rtol, what):
    """test_gpu_grad.close's measure."""
    err, scale = (got.double() - ref.double()).abs().max().item(), ref.double().abs().max().item()
    assert err <= rtol * scale + 1e-7, what


def _logs(toy, op, *args, **kw):
    """The ``returns`` logs of toy.<op>(*args) under both fills (looked up inside the context: the logged one)."""
    logs = {}
    for fill in B.FILLS:
        with ctx(toy, fill) as arena:
            getattr(toy, op)(*args, **kw)
        assert arena.returns
        logs[fill] = arena.returns
    return logs


def test_compare_fills_passes_a_correct_op_and_labels_outputs(toy):
    logs = _logs(toy, "correct", X)
    assert B.compare_fills(logs["zero"], logs["poison"]) == set()
    base = torch.ones(5)
    logs = {}
    for fill in B.FILLS:
        with ctx(toy, fill) as arena:
            toy.noisy(V, d_rd_into=base.clone())
        logs[fill] = arena.returns
    assert [r[0] for r in logs["zero"]] == ["noisy", "noisy (accumulated)"]
    assert [label for label, _ in logs["zero"][0][1]] == ["exact", "sum"]
    assert [label for label, _ in logs["zero"][1][1]] == ["d_rd_into"]
    assert torch.equal(logs["zero"][1][1][0][1], base + V)


def test_compare_fills_fails_on_an_unwritten_output(toy):
    logs = _logs(toy, "unwritten", V)
    with pytest.raises(AssertionError, match="depends on what its buffers held.*first at flat index 4.*1 NaN"):
        B.compare_fills(logs["zero"], logs["poison"])


def test_compare_fills_exceptions_cover_only_what_they_name(toy):
    """An exception excuses a difference within its bound on the output it names, never a NaN one fill lacks,
    never another output, and a bound of None still wants the NaNs to agree."""
    logs = _logs(toy, "noisy", V)

    def only(label):
        return lambda name, lab, kw: "k" if (name, lab) == ("noisy", label) else None
    for bounds in ({"k": 1.0}, {"k": None}):          # "sum"'s tail is NaN under poison only
        with pytest.raises(AssertionError, match="NaN under one fill only"):
            B.compare_fills(logs["zero"], logs["poison"], exception_for=only("sum"), bounds=bounds, close=_close)
    with pytest.raises(AssertionError, match="depends on what its buffers held"):
        B.compare_fills(logs["zero"], logs["poison"], exception_for=only("exact"), bounds={"k": 1.0}, close=_close)
    # outputs_of drops the open tail: nothing differs, no exception is used
    trim = lambda name, pairs, kw: [(lab, t[:5]) for lab, t in pairs]          # noqa: E731
    assert B.compare_fills(logs["zero"], logs["poison"], outputs_of=trim) == set()
    # a finite difference: inside the bound passes and reports its key, outside fails, unnamed fails
    moved = [("noisy", [("exact", V + 1e-3), ("sum", V.clone())], {})]
    plain = [("noisy", [("exact", V.clone()), ("sum", V.clone())], {})]
    assert B.compare_fills(plain, moved, exception_for=only("exact"), bounds={"k": 1e-3}, close=_close) == {"k"}
    assert B.compare_fills(plain, moved, exception_for=only("exact"), bounds={"k": None}, close=_close) == {"k"}
    with pytest.raises(AssertionError):
        B.compare_fills(plain, moved, exception_for=only("exact"), bounds={"k": 1e-5}, close=_close)
    with pytest.raises(AssertionError, match="depends on what its buffers held"):
        B.compare_fills(plain, moved, exception_for=only("sum"), bounds={"k": 1.0}, close=_close)


def test_compare_fills_wants_the_same_calls(toy):
    a = _logs(toy, "correct", X)["zero"]
    b = _logs(toy, "unwritten", V)["zero"]
    with pytest.raises(AssertionError, match="different calls"):
        B.compare_fills(a, b)
    with pytest.raises(AssertionError, match="different outputs"):
        B.compare_fills([("f", [("x", V)], {})], [("f", [("y", V)], {})])


def test_full_infers_the_fill_values_type(toy):
    with ctx(toy, "poison"):
        assert toy.torch.full((3,), -1).dtype == torch.int64 and toy.torch.full((3,), 0.5).dtype == torch.float32
        assert toy.torch.empty(()).shape == () and toy.torch.empty((), dtype=torch.float64).dtype == torch.float64
