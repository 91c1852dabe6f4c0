"""Every op honours the caller's stream and survives graph capture (tests/streams.py).

The rest of the suite runs every kernel on the default stream, where a launch with a forgotten stream argument,
a hidden synchronisation or a host read of a device value changes no value.  Here the same runners run

  (a) under a side stream, with a spin on the default stream before every ``codenerf.ops`` call and a copy of
      the call's results right behind it: bit for bit the default-stream run's log, conclusive per call;
  (b) call by call, captured alone in a graph in global error mode and replayed twice over poisoned outputs:
      the eager bits both times;

and whole steps (the eval step and the training step of tests/pair_path_cases.py, train_minibatch) run under a
side stream, and with the forward under one stream and ``backward()`` under another.

Both comparisons are bitwise, with test_gpu_buffer_contracts.EXCEPTIONS for the float-atomic routes and no bound
of their own.  NOT_CAPTURABLE is the only list of calls (b) leaves out, and those must refuse capture.
"""
import contextlib
import gc
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest
import torch

import buffers as B
import pair_path_cases as C
import streams as S
import test_gpu_buffer_contracts as BC
import test_gpu_density as DEN
import test_gpu_density_grad as DG
import test_gpu_occupancy as OCC
import test_gpu_pair_paths as PP
import test_gpu_pose_data as PD
import test_gpu_scene as SCN
import test_gpu_train as T
import test_gpu_view_rows as VR
import test_gpu_weight_cull as WCT
from test_gpu_density import field as density_field  # noqa: F401
from test_gpu_density_grad import field as gradient_field  # noqa: F401
from test_gpu_grad import close, dev, embedders  # noqa: F401
from test_gpu_occupancy import scene as occupancy_scene  # noqa: F401
from test_gpu_pair_paths import eval_models  # noqa: F401
from test_gpu_scene import scene as compose_scene  # noqa: F401
from test_gpu_weight_cull import scene as cull_scene  # noqa: F401

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- what is documented to synchronise the host
#
# name -> the sentence of its docstring that says so.  (b) leaves these out and nothing else; each must refuse
# capture (test_the_table_refuses_capture_and_the_toys_are_told_apart), the captured form of the optimiser
# step -- graph_scalars() + graph_step() -- must not.
NOT_CAPTURABLE = {
    "occupancy_cull": "This is the one place that reads ``count`` back (``.item()``): a HOST SYNCHRONISATION",
    "weight_cull": "Like occupancy_cull, this reads ``count`` back once (``.item()``): a HOST SYNCHRONISATION",
    "isosurface": "The two totals are read back once (``.item()``) between the count and the emit: a HOST "
                  "SYNCHRONISATION",
    "AdamW.step": "Not graph-capturable: the step counts live on the host and are folded into the launch's "
                  "arguments, so a replay would repeat this step's; under capture it raises (use graph_scalars() "
                  "+ graph_step()).",
}
WHOLE_STEPS = ("train-step-f32", "train-step-bf16x3", "eval-step")     # (b): their host logic is not capturable

TALLY = {"cases": 0, "side_calls": 0, "retries": 0, "min_slack_ms": float("inf"), "logged": 0, "duplicate": 0,
         "captured": 0, "table": 0, "side_only_cases": 0}
_SEEN = set()


def _documented(name):
    if name == "AdamW.step":
        from codenerf.optim import AdamW
        return AdamW.step.__doc__
    from codenerf import ops
    return getattr(ops, name).__doc__


def test_the_table_cites_the_docstrings():
    for name, sentence in NOT_CAPTURABLE.items():
        assert " ".join(sentence.split()) in " ".join(_documented(name).split()), name


# ---------------------------------------------------------------- sensitivity: toy ops in plain torch

TOY_SOURCE = '''
import torch


def correct(x):
    """2 x + 1 on the current stream."""
    out = torch.empty_like(x)
    torch.mul(x, 2.0, out=out)
    return out.add_(1.0)


def on_default(x):
    """The same, with its work under the default stream whatever stream is current."""
    out = torch.empty_like(x)
    with torch.cuda.stream(torch.cuda.default_stream()):
        torch.mul(x, 2.0, out=out)
        out.add_(1.0)
    return out


def reads_back(x):
    """The same, sized by a device value read on the host."""
    n = int((x == x).sum().item())
    out = torch.empty(n, dtype=x.dtype, device=x.device)
    torch.mul(x.reshape(-1), 2.0, out=out)
    return out.add_(1.0).reshape(x.shape)
'''


def make_toy():
    mod = types.ModuleType("streams_toy_ops")
    sys.modules[mod.__name__] = mod
    exec(compile(TOY_SOURCE, "streams_toy_ops.py", "exec"), mod.__dict__)
    return mod


@pytest.fixture()
def toy():
    mod = make_toy()
    yield mod
    del sys.modules[mod.__name__]


def _toy_logs(toy, name, x):
    with B.contracts("poison", modules=(toy,), log_returns_of=None), S.plain(module=toy) as base:
        want = getattr(toy, name)(x)
    with B.contracts("poison", modules=(toy,), log_returns_of=None), S.side_stream(module=toy) as side:
        getattr(toy, name)(x)
    assert torch.equal(want, 2 * x + 1)
    return base, side


def test_side_stream_check_tells_the_toys_apart(dev, toy):
    """(a) passes the toy that works on the current stream and the one that reads a value back (a host
    synchronisation moves no work to another stream: that class is (b)'s), and flags the one that works under
    the default stream: its output still holds the poison when it is copied."""
    x = torch.arange(1.0, 1025.0, device=dev)
    torch.cuda.synchronize()
    for name in ("correct", "reads_back"):
        base, side = _toy_logs(toy, name, x)
        S.compare_logs(base.returns, side.returns, name)
        assert len(side.slack_ms) == 1 and side.slack_ms[0] > 0
    base, side = _toy_logs(toy, "on_default", x)
    assert side.slack_ms[0] > 0
    with pytest.raises(AssertionError, match="differs from the default-stream run"):
        S.compare_logs(base.returns, side.returns, "on_default")
    assert bool(torch.isnan(side.returns[0][1][0][1]).all())


def test_spin_is_calibrated(dev):
    """The spin the checks rest on lasts what it is asked to, within a factor of two."""
    a = torch.cuda.Event(enable_timing=True)
    a.record()
    b = S.spin(torch.cuda.current_stream(), S.SPIN_MS)
    b.synchronize()
    ms = a.elapsed_time(b)
    print("STREAMS_SPIN", json.dumps({"cycles_per_ms": S.cycles_per_ms(), "asked_ms": S.SPIN_MS, "took_ms": ms}))
    assert 0.5 * S.SPIN_MS <= ms <= 2.0 * S.SPIN_MS + 0.5


def test_two_streams_run_beside_the_default_stream(dev):
    """The streams the checks run under: two, each of which finishes work while the default stream or the
    other one spins (streams that share a hardware queue do not)."""
    a, b = S.concurrent_streams(2)
    default = torch.cuda.default_stream()
    assert a != b and a != default and b != default
    for busy, other in ((default, a), (default, b), (a, b), (b, a)):
        assert S.runs_beside(busy, other)


# ---------------------------------------------------------------- every case under (a) and (b)


def check_case(dev, run, allowed, capture=True, warm=False):
    """``warm``: the runner is called once beforehand, for runners whose first call fills a cache a later one
    reads (a model's packs): both logged runs then make the same calls."""
    allowed = set(allowed)
    if warm:
        run(dev, None)

    def exception_for(name, label, kw):
        return BC.exception_for(name, label, kw, allowed)

    BC.fresh_caches()
    with B.contracts("poison", log_returns_of=None) as arena, S.plain(record=capture) as base:
        run(dev, arena)
    BC.fresh_caches()
    with B.contracts("poison", log_returns_of=None) as arena, S.side_stream(wall_ms=base.wall_ms) as side:
        run(dev, arena)
    BC.fresh_caches()
    assert base.returns, "no codenerf.ops call was logged"
    assert [r[0] for r in base.returns] == [r[0] for r in side.returns], "the two runs made different calls"
    assert side.slack_ms and min(side.slack_ms) > 0
    if "eval_step" not in allowed:
        S.compare_logs(base.returns, side.returns, "the side-stream run", BC.outputs_of, exception_for, BC.BOUNDS,
                       close)
    TALLY["cases"] += 1
    TALLY["side_calls"] += len(side.slack_ms)
    TALLY["retries"] += side.retries
    TALLY["min_slack_ms"] = min(TALLY["min_slack_ms"], min(side.slack_ms))
    if not capture:
        TALLY["side_only_cases"] += 1
        return
    TALLY["logged"] += len(base.wall_ms)          # the outermost calls (a)'s plain run logged
    for rec in base.records:
        key = rec.key()
        if key in _SEEN:
            TALLY["duplicate"] += 1
        elif rec.name in NOT_CAPTURABLE:
            _SEEN.add(key)
            TALLY["table"] += 1
        else:
            _SEEN.add(key)
            S.capture_replay(rec, BC.outputs_of, exception_for, BC.BOUNDS, close)
            TALLY["captured"] += 1


def added_cases():
    """The ops test_gpu_buffer_contracts.case_list() lacks, each at the smallest parameters its own file states."""
    out = []

    def add(name, fn, *args, allowed=()):
        out.append(pytest.param(lambda dev, arena: fn(dev, *args), tuple(allowed), id=name))

    add("object-rays-1x1", SCN.test_object_rays_bit_exact, 1, 1)
    add("compose-exclusive-2x17", SCN.test_exclusive_activity, 2, 17)
    add("compose-overlap-2x64", SCN.test_overlap_against_the_rule, 2, 64)
    small = [c for c in VR.ONE_CODE_GEOMETRY if (c["r"], c["s"], c["chunk"]) in ((1, 1, 1), (7, 5, 3))]
    for c in small or VR.ONE_CODE_GEOMETRY[:2]:
        add(f"view-rows-{VR.ident(c)}", VR.run_exact, c)
    return out


CASES = BC.case_list() + added_cases()


@pytest.mark.parametrize("run,allowed", CASES)
def test_side_stream_and_capture(dev, request, run, allowed):
    check_case(dev, run, allowed, capture=request.node.callspec.id not in WHOLE_STEPS)


@pytest.mark.parametrize("mode", ["pts", "rayz"])
@pytest.mark.parametrize("r,s", [(1, 1), (50, 8)])
def test_density_field(dev, density_field, r, s, mode):
    """cn_density_field at m = 1 and at 400 rows (three tiles and a ragged one), from points and from rays."""
    check_case(dev, lambda dev, arena: DEN.test_density_bitwise_vs_full_field(dev, density_field, r, s, mode, "one"),
               ())


@pytest.mark.parametrize("m", [1, 127])
def test_density_gradient_points(dev, gradient_field, m):
    check_case(dev, lambda dev, arena: DG.test_gradient_and_sigma_bits_small(dev, gradient_field, m), ())


@pytest.mark.parametrize("r,s", [(7, 16), (50, 3)])
def test_density_gradient_rays(dev, gradient_field, r, s):
    check_case(dev, lambda dev, arena: DG.test_gradient_and_sigma_bits_ray_mode(dev, gradient_field, r, s), ())


def test_srn_unpack(dev, tmp_path):
    def run(dev, arena):
        tree = tmp_path / f"tree{len(os.listdir(tmp_path))}"
        tree.mkdir()
        PD.test_srn_resident_batches(dev, tree, "train")
    check_case(dev, run, ())


def test_culled_renders_side_stream_only(dev, occupancy_scene, cull_scene):
    """The inference render_rays with an occupancy grid and with weight culling: they synchronise the host
    (NOT_CAPTURABLE), so (a) only."""
    check_case(dev, lambda dev, arena: OCC.test_render_sphere_grid_composed(dev, occupancy_scene, 64, 64, True), (),
               capture=False, warm=True)
    nc, nf = WCT.SAMPLERS[0]
    check_case(dev, lambda dev, arena: WCT.test_render_tolerance_composed(dev, cull_scene, nc, nf, True), (),
               capture=False, warm=True)


def test_render_scene_side_stream_only(dev, compose_scene):
    """render_scene with two overlapping objects (its culls synchronise the host): (a) only."""
    check_case(dev, lambda dev, arena: SCN.test_two_overlapping_objects(compose_scene), (), capture=False,
               warm=True)


def test_run_cap():
    """(b) left out nothing but duplicates and the table: every outermost call (a)'s plain run logged was
    captured, was the same call as one captured before, or is in NOT_CAPTURABLE."""
    print("STREAMS_TALLY", json.dumps(TALLY))
    assert TALLY["logged"] == TALLY["captured"] + TALLY["duplicate"] + TALLY["table"]
    assert TALLY["logged"] == 0 or TALLY["captured"] > 0
    # (a) only: the two whole steps of the contracts list (test_forward_and_backward_... covers them), the two
    # culled renders and render_scene
    assert TALLY["side_only_cases"] <= 6
    assert TALLY["retries"] <= TALLY["side_calls"]


# ---------------------------------------------------------------- whole steps across streams


@contextlib.contextmanager
def no_collection():
    """Python's collector held off while a spin is being outrun: a pass over a long session's heap takes longer
    than the spins here."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class Backward:
    """``backward_from`` as the steps call it (codenerf.autograd / codenerf.train), with what the cases need
    around it.  Every mode times the call on the host, then copies the loss, every parameter's ``.grad`` (the
    optimiser's, found through its zero_grad) on the stream then current, and with ``step_after`` runs one
    optimiser step there and copies the parameters.

    ``mode``: "plain"; "watch": ``arm()`` enqueues a spin of ``watch_ms`` on the default stream before a step
    (train_minibatch calls it itself), and right after the copies are enqueued its end is asked whether it is
    still pending; "split": the forward ran under the current stream X -- the other stream Y waits for X (as a
    caller must), a spin is enqueued on X (ten times this call's host time in the default-stream run before,
    20 ms to 1 s), and the backward, the copies and everything after run under Y."""

    def __init__(self, monkeypatch, step_after):
        from codenerf import autograd as A, optim, train as TR
        self.real, self.step_after = A.backward_from, step_after
        self.mode, self.event, self.streams, self.warm, self.watch_ms = "plain", None, None, None, None
        self.opt = None
        self.reset()
        real_zero = optim.AdamW.zero_grad

        def zero_grad(opt, *a, **k):
            self.opt = opt
            return real_zero(opt, *a, **k)
        monkeypatch.setattr(optim.AdamW, "zero_grad", zero_grad)
        monkeypatch.setattr(A, "backward_from", self)
        monkeypatch.setattr(TR, "backward_from", self)
        real_minibatch = TR.train_minibatch

        def train_minibatch(*a, **k):
            self.arm()
            t0 = time.perf_counter()
            try:
                return real_minibatch(*a, **k)
            finally:
                self.step_wall.append(time.perf_counter() - t0)
        monkeypatch.setattr(TR, "train_minibatch", train_minibatch)

    def reset(self):
        self.wall, self.loss, self.grads, self.params = [], [], [], []
        self.held, self.spins, self.step_wall = [], [], []

    def arm(self):
        if self.mode == "watch":
            self.event = S.spin(torch.cuda.default_stream(), self.watch_ms)

    def leaves(self):
        return [p for g in self.opt.param_groups for p in g["params"]]

    def __call__(self, loss):
        event = self.event
        if self.mode == "split":
            here = torch.cuda.current_stream()
            there = self.streams[1] if here == self.streams[0] else self.streams[0]
            there.wait_stream(here)
            ms = min(1000.0, max(20.0, 10e3 * self.warm[len(self.wall)]))
            event = S.spin(here, ms)
            self.spins.append(ms)
            torch.cuda.set_stream(there)
        t0 = time.perf_counter()
        self.real(loss)
        self.wall.append(time.perf_counter() - t0)
        grads = [None if p.grad is None else p.grad.detach().clone() for p in self.leaves()]
        if event is not None:
            self.held.append(not event.query())       # the spin was still running when the copies were enqueued
        self.grads.append(grads)
        self.loss.append(loss.detach().clone())
        if self.step_after:
            self.opt.step()
            self.params.append([p.detach().clone() for p in self.leaves()])


def same_tensors(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (what, i)
        if a is not None:
            assert a.shape == b.shape and torch.equal(B.tensor_bytes(a), B.tensor_bytes(b)), \
                (what, i, (a - b).abs().max().item(), int(torch.isnan(a).sum()))


NC, NF = C.SAMPLES[0]


def eval_step(dev, models, seen):
    """pair_path_cases' eval step (16 x 16 view, 100 rays, 16 + 16 samples, loss on both images): the shared
    launch of both fields must have run."""
    PP._reset(seen)
    out = PP._eval_step(dev, C.eval_inputs(NC, NF), NC, NF, "both", models)
    assert (seen["multi"], seen["x3"], seen["flush"]) == C.EXPECTED_CALLS[((NC, NF), "both")]
    return [torch.tensor(out[0])] + [out[1][k] for k in C.LEAVES]


def train_step(dev, models, seen):
    """Its training counterpart (64 rays, 16 + 16 samples, weights trained, on_grads given): one shared call
    for both fields, on_grads once."""
    PP._reset(seen)
    called = []
    got = PP._train_step(dev, "both", None, lambda: called.append(1))
    _, _, n_on_grads, multi_calls = PP.TRAIN_CASES["both"]
    assert len(called) == n_on_grads and seen["train_multi"] == multi_calls
    return [got[k] for k in sorted(got)]


def minibatch_step(dev, models, seen, bw):
    """test_train_minibatch_deterministic's steps in f32 (two model sets, three chunks each, its own assertion)
    -> the second set's flat parameters after the last step."""
    T.test_train_minibatch_deterministic(dev, "f32")
    return [bw.opt.flat_buffers()["param"].detach().clone()]


STEPS = {"eval": eval_step, "train": train_step}


@pytest.mark.parametrize("step", ["eval", "train", "minibatch"])
def test_whole_step_under_a_side_stream(dev, monkeypatch, eval_models, step):
    """Case (i): the whole step under a side stream, the default stream held by a spin from before each step
    until after its backward's results are copied (else inconclusive: a failure): the loss, every gradient
    (minibatch: every parameter after three optimiser steps) and what the step returns, bit for bit the
    default-stream step's."""
    seen, _ = PP._spies(monkeypatch)
    bw = Backward(monkeypatch, step_after=False)

    def run():
        if step == "minibatch":
            return minibatch_step(dev, eval_models, seen, bw)
        return STEPS[step](dev, eval_models, seen)
    t0 = time.perf_counter()
    want = run()
    ref = (bw.loss, bw.grads)
    # a spin covers one step, from before its forward until its backward's results are copied: three times the
    # longest step of the run above on the host, 20 ms to 1 s
    spans = bw.step_wall or [time.perf_counter() - t0]
    ms = min(1000.0, max(20.0, 3e3 * max(spans)))
    bw.reset()
    bw.mode, bw.watch_ms = "watch", ms
    torch.cuda.synchronize()
    with no_collection(), torch.cuda.stream(S.concurrent_streams(1)[0]):
        if step != "minibatch":
            bw.arm()
        got = run()
    torch.cuda.synchronize()
    print("STREAMS_SIDE_STEP", json.dumps({"step": step, "spans_ms": [1e3 * x for x in spans], "spin_ms": ms,
                                           "held": bw.held}))
    assert bw.held and all(bw.held), ("inconclusive: the spin ended before the copies were enqueued", bw.held, ms)
    same_tensors(bw.loss, ref[0], "loss")
    for i, (a, b) in enumerate(zip(bw.grads, ref[1])):
        same_tensors(a, b, f"gradients of backward {i}")
    same_tensors(got, want, "what the step returned")


@pytest.mark.parametrize("step", ["eval", "train", "minibatch"])
def test_forward_and_backward_under_different_streams(dev, monkeypatch, eval_models, step):
    """Cases (ii) and (iii).  The forward runs under stream A; B waits for A, a spin is enqueued on A, and
    under B ``backward()`` runs and every ``.grad`` is copied at once, then one optimiser step runs under B and
    the parameters are copied (minibatch: train_minibatch's own step, and the next chunk swaps the streams'
    roles).  The spin was still running when the copies were enqueued (else inconclusive: a failure), so
    only a wait B itself was made to do orders the copies after the backward's kernels.  Loss, gradients
    and updated parameters bit for bit the default-stream step's."""
    seen, _ = PP._spies(monkeypatch)
    bw = Backward(monkeypatch, step_after=step != "minibatch")

    def run():
        if step == "minibatch":
            return minibatch_step(dev, eval_models, seen, bw)
        return STEPS[step](dev, eval_models, seen)
    want = run()
    ref = (bw.loss, bw.grads, bw.params)
    bw.warm = list(bw.wall)
    bw.reset()
    bw.mode, bw.streams = "split", tuple(S.concurrent_streams(2))
    torch.cuda.synchronize()
    with no_collection(), torch.cuda.stream(bw.streams[0]):
        got = run()
    torch.cuda.synchronize()
    print("STREAMS_SPLIT", json.dumps({"step": step, "backward_wall_ms": [1e3 * w for w in bw.warm],
                                       "spin_ms": bw.spins, "held": bw.held}))
    assert bw.held and all(bw.held), ("inconclusive: the spin ended before the copies were enqueued", bw.held)
    same_tensors(bw.loss, ref[0], "loss")
    for i, (a, b) in enumerate(zip(bw.grads, ref[1])):
        same_tensors(a, b, f"gradients right after backward {i}")
    for i, (a, b) in enumerate(zip(bw.params, ref[2])):
        same_tensors(a, b, f"parameters right after optimiser step {i}")
    same_tensors(got, want, "what the step returned")


def test_graphed_eval_step_on_a_side_stream(dev, eval_models):
    """GraphedEvalStep built and stepped with a non-default stream current: over two replays the loss and every
    gradient are the eager step's on the default stream, bit for bit (test_graphed_eval_step_matches_eager's
    assertion, at pair_path_cases' size)."""
    from codenerf.evaluate import GraphedEvalStep, eval_step_loss
    from codenerf.nerf import PointSampler, RaySampler
    from codenerf.optim import AdamW
    inp = {k: v.to(dev) for k, v in C.eval_inputs(NC, NF).items()}
    rs = RaySampler(C.SIZE, C.SIZE, C.intrinsics(), sample_size=C.N_RAYS, device=dev, datatype=torch.float32)
    ps = PointSampler(NC, NF, C.NEAR, C.FAR, "lindepth", True, torch.float32, dev)

    def leaves():
        return [inp[k].clone().requires_grad_(True) for k in C.LEAVES]

    eager = []
    np.random.seed(17)
    for _ in range(2):
        lv = leaves()
        loss, _ = eval_step_loss(*lv, inp["target"], (rs, ps), embedders(dev), eval_models, C.LAM,
                                 t_rand=inp["t_rand"], u=inp["u"])
        loss.backward()
        eager.append((loss.item(), [t.grad.clone() for t in lv]))
    torch.cuda.synchronize()
    side = S.concurrent_streams(1)[0]
    with torch.cuda.stream(side):
        th, ph, rh, zs, zt = lv = leaves()
        opt = AdamW([{"params": [zs, zt]}, {"params": [th, ph]}, {"params": [rh]}], lr=1e-2)
        np.random.seed(17)
        step = GraphedEvalStep(th, ph, rh, zs, zt, inp["target"], (rs, ps), embedders(dev), eval_models, opt, C.LAM,
                               t_rand=inp["t_rand"], u=inp["u"], optimizer_in_graph=False)
        got = [torch.empty_like(step.loss)] + [torch.empty_like(t) for t in lv]    # allocated before any spin
        side.synchronize()
        gc.collect()
        for i in range(2):
            held = S.spin(torch.cuda.default_stream(), 20.0)
            loss, _ = step.step()
            for dst, src in zip(got, [loss] + [t.grad for t in lv]):
                dst.copy_(src)
            assert not held.query(), "inconclusive: the default stream's spin ended before the copies were enqueued"
            side.synchronize()
            le, ge = eager[i]
            assert got[0].item() == le, (i, got[0].item(), le)
            for name, t, ref in zip(C.LEAVES, got[1:], ge):
                assert torch.equal(t, ref), (f"replay {i} {name}", (t - ref).abs().max().item())
    torch.cuda.synchronize()


# ---------------------------------------------------------------- refusals, in a process of their own
#
# A capture that raised leaves its stream's capture invalidated and the allocator's capture pool open: nothing
# the rest of the session should inherit.  So the captures that must fail run in one fresh child process, which
# prints what became of each.

CHILD_CASES = {"occupancy_cull": "occupancy-cull-1x1", "weight_cull": "weight-cull-1x1", "isosurface": "isosurface-33"}


def _outcome(call):
    try:
        call()
        return {"outcome": "captured"}
    except S.Refused as e:
        return {"outcome": "refused", "detail": str(e)[:300]}
    except AssertionError as e:
        return {"outcome": "wrong replay", "detail": str(e)[:300]}
    except Exception as e:        # noqa: BLE001 -- reported, and the parent fails on it
        return {"outcome": "error", "detail": f"{type(e).__name__}: {e}"[:300]}


def _adamw(device):
    from codenerf.optim import AdamW
    g = torch.Generator().manual_seed(2)
    p = torch.nn.Parameter((torch.randn(256, 63, generator=g) * 0.1).to(device))
    opt = AdamW([{"params": [p], "lr": 1e-3, "weight_decay": 0.05}])
    return p, opt, (torch.randn(256, 63, generator=g) * 1e-2).to(device)


def refusals_main():
    import codenerf
    codenerf.load_library()
    device = torch.device("cuda", 0)
    toy = make_toy()
    x = torch.arange(1.0, 1025.0, device=device)
    results = {}

    def toy_probe(name):
        with S.plain(module=toy, record=True) as base:
            getattr(toy, name)(x)
        return _outcome(lambda: S.capture_replay(base.records[0]))

    # what must be captured, first
    results["toy.correct"] = toy_probe("correct")
    p, opt, grad = _adamw(device)
    opt.zero_grad(set_to_none=False)
    p.grad.copy_(grad)
    host = np.zeros(3, dtype=np.float32)
    opt.graph_scalars(host)
    scalars = torch.from_numpy(host).to(device)
    results["AdamW.graph_scalars + graph_step"] = _outcome(lambda: S.capture(lambda: opt.graph_step(scalars)))
    # what must not
    results["toy.reads_back"] = toy_probe("reads_back")
    results["toy.on_default"] = toy_probe("on_default")
    cases = {c.id: c.values for c in BC.case_list()}
    for name, case in CHILD_CASES.items():
        run, _ = cases[case]
        with S.plain(record=True) as base:
            run(device, None)
        recs = [r for r in S.distinct(base.records) if r.name == name]
        assert recs, name
        results[name] = _outcome(lambda: S.capture_replay(recs[0], BC.outputs_of, None, BC.BOUNDS, close))
    p, opt, grad = _adamw(device)
    p.grad = grad.clone()
    opt.step()
    torch.cuda.synchronize()
    results["AdamW.step"] = _outcome(lambda: S.capture(opt.step))
    # and the refusals left the process able to capture
    results["toy.correct, afterwards"] = toy_probe("correct")
    print("STREAMS_REFUSALS " + json.dumps(results))


def test_the_table_refuses_capture_and_the_toys_are_told_apart(dev):
    """(b) in a child process: the correct toy and the optimiser's captured form are captured and replay to the
    eager bits; the toy that reads a value back refuses; the toy that works under the default stream refuses or
    replays wrongly (its work ran at capture time and never entered the graph); every entry of NOT_CAPTURABLE
    refuses; and a capture still works after all of that."""
    torch.cuda.synchronize()
    here = os.path.dirname(os.path.abspath(__file__))
    done = subprocess.run([sys.executable, "-c", "import conftest, test_gpu_streams as M; M.refusals_main()"],
                          cwd=here, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in done.stdout.splitlines() if ln.startswith("STREAMS_REFUSALS ")]
    assert done.returncode == 0 and lines, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    results = json.loads(lines[-1][len("STREAMS_REFUSALS "):])
    print(lines[-1])
    got = {k: v["outcome"] for k, v in results.items()}
    assert got["toy.correct"] == got["toy.correct, afterwards"] == "captured", results
    assert got["AdamW.graph_scalars + graph_step"] == "captured", results
    assert got["toy.reads_back"] == "refused", results
    assert got["toy.on_default"] in ("refused", "wrong replay"), results
    for name in NOT_CAPTURABLE:
        assert got[name] == "refused", (name, results)
