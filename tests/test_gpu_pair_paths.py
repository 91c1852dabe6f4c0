"""The paired field backward (autograd.FieldPair) off the path the drivers take: a field that waits
alone, a partner that cannot pair, a loss that reaches one field.

The steps here are built from the pieces evaluate.eval_step_loss and train.train_minibatch use, so the
loss can be chosen.  Every case is held against the same step with pairing off (bit for bit: the
unpaired route is the one the C5 / C3 fixtures pin to the reference), the eval cases also against the
oracle's op sequence in float64 on the kernels' own fine depths (pair_path_cases.eval_reference), and
the path each case is meant to reach is counted.
"""
import pytest
import torch

import pair_path_cases as C
from test_gpu_grad import dev, embedders, model  # noqa: F401

pytestmark = pytest.mark.gpu


def _spies(monkeypatch):
    """Counts of the launches that tell the paths apart, the FieldPairs render_rays made, the fine depths."""
    from codenerf import autograd as A, ops
    seen = {"multi": 0, "x3": 0, "flush": 0, "train_multi": [], "pairs": [], "z_fine": None}
    real = {"multi": ops.field_backward_x3_multi, "x3": ops.field_backward_x3, "flush": A._pair_flush,
            "train_multi": ops.field_backward_train_multi, "pair": A.new_field_pair, "pdf": ops.sample_pdf}

    def multi(*a, **k):
        seen["multi"] += 1
        return real["multi"](*a, **k)

    def x3(*a, **k):
        seen["x3"] += 1
        return real["x3"](*a, **k)

    def flush(pair):
        seen["flush"] += int(pair.pending is not None)     # (the end-of-pass callback finds nothing: not counted)
        return real["flush"](pair)

    def train_multi(fields, precision="f32"):
        seen["train_multi"].append(len(fields))
        return real["train_multi"](fields, precision)

    def new_pair():
        p = real["pair"]()
        seen["pairs"].append(p)
        return p

    def pdf(*a, **k):
        r = real["pdf"](*a, **k)
        seen["z_fine"] = r[1].detach().cpu()
        return r
    monkeypatch.setattr(ops, "field_backward_x3_multi", multi)
    monkeypatch.setattr(ops, "field_backward_x3", x3)
    monkeypatch.setattr(A, "_pair_flush", flush)
    monkeypatch.setattr(ops, "field_backward_train_multi", train_multi)
    monkeypatch.setattr(A, "new_field_pair", new_pair)
    monkeypatch.setattr(ops, "sample_pdf", pdf)
    return seen, real


def _reset(seen):
    seen.update(multi=0, x3=0, flush=0, train_multi=[], pairs=[], z_fine=None)


# ---------------------------------------------------------------- the eval step


def _eval_step(dev, inp, nc, nf, loss_kind, models, train_codes=True):
    """eval_step_loss's pieces (evaluate.py) with the loss's images chosen -> (loss, the leaves' gradients,
    the rays' sink, the code rows' sink).  ``train_codes=False``: the codes are constants (pose only)."""
    from codenerf import autograd as A, evaluate as E, nerf
    from codenerf.models.model import CodeRows, code_rows_with_sink
    from codenerf.nerf import PointSampler, RaySampler
    from codenerf.optim import AdamW
    lv = {k: inp[k].clone().to(dev).requires_grad_(train_codes or k not in ("z_s", "z_t")) for k in C.LEAVES}
    groups = [{"params": [lv["theta"], lv["phi"]]}, {"params": [lv["rho"]]}]
    opt = AdamW(([{"params": [lv["z_s"], lv["z_t"]]}] if train_codes else []) + groups, lr=1e-2)
    opt.zero_grad()
    rs = RaySampler(C.SIZE, C.SIZE, C.intrinsics(), sample_size=C.N_RAYS, device=dev, datatype=torch.float32)
    ps = PointSampler(nc, nf, C.NEAR, C.FAR, "lindepth", True, torch.float32, dev)
    with A.eval_ray_sinks():
        ro, rd, _, _, tp = rs.sample_spherical(lv["theta"], lv["phi"], lv["rho"], target=inp["target"].to(dev),
                                               sel=inp["sel"].to(dev))
    n = ro.shape[0]
    assert n == C.N_RAYS
    sc, tc = code_rows_with_sink(lv["z_s"], lv["z_t"])
    z_s, z_t = sc.expand(n, -1), tc.expand(n, -1)
    z_s._cn_code_rows = z_t._cn_code_rows = CodeRows(sc, tc, None)
    with A.paired_fields():
        out = nerf.render_rays(ro, rd, z_s, z_t, ps, embedders(dev), models["nerf_coarse"], models["nerf_fine"],
                               chunk_rows=n, t_rand=inp["t_rand"].to(dev), u=inp["u"].to(dev))
    rgb_c = out["rgb_coarse"] if loss_kind in ("both", "coarse") else None
    rgb_f = out["rgb_fine"] if loss_kind in ("both", "fine") else None
    loss, _ = E.nerf_loss(rgb_c, rgb_f, tp, sc, tc, n, C.LAM)
    A.backward_from(loss)
    torch.cuda.synchronize()
    return loss.item(), {k: v.grad for k, v in lv.items()}, ro._cn_ray_sink, getattr(sc, "_cn_sink", None)


@pytest.fixture(scope="module")
def eval_models(dev):
    ms = {"nerf_coarse": model(dev, 0), "nerf_fine": model(dev, 1)}
    for m in ms.values():
        m.train()
        m.requires_grad_(False)
    return ms


@pytest.mark.parametrize("loss_kind", C.LOSSES)
@pytest.mark.parametrize("nc,nf", C.SAMPLES)
def test_eval_field_backs_up_alone(dev, monkeypatch, eval_models, nc, nf, loss_kind):
    """One eval step (16x16 view, 100 rays, frozen fp32 models, leaf pose and codes in a flat AdamW) per
    sample count and loss.  (1) the loss and d(theta, phi, rho, z_s, z_t) bit for bit those of the step
    with pairing off; (2) each gradient within 2e-3 of the float64 reference's largest magnitude (pose
    scalars: floor 1e-2), on the kernels' own fine depths; (3) the launches and flushes the case is meant
    to take were taken, and nothing is left waiting: the ray sink holds no pair, no pair is pending.

    Before PoseRays.backward and CodeGradSink.take() ran a waiting field themselves, the five cases in
    which a field waits alone with no partner to flush it -- 16 + 16 fine only / coarse only, 32 + 24
    both / coarse only, 24 + 40 fine only -- raised from the end-of-pass callback (_pair_flush's
    RuntimeError: the code rows had been handed out before it ran the field); only that check on the
    codes stood between such a step and pose gradients silently missing the field's rays.

    32 + 24 and 24 + 40 hold a field of 56 or 24 samples, whose waves straddle rays: (1) is bitwise there
    only because the fp32 eval backward sums such a field's ray terms in a fixed order too (per sample
    rows, ops.field_backward_x3).  With the float-atomic kernel two runs of that field's own call differed
    by up to 4e-6 of a gradient's largest magnitude, pairing or not."""
    from codenerf import autograd as A
    from conftest import margin
    seen, real = _spies(monkeypatch)
    inp = C.eval_inputs(nc, nf)
    loss, grads, ray_sink, code_sink = _eval_step(dev, inp, nc, nf, loss_kind, eval_models)
    calls = (seen["multi"], seen["x3"], seen["flush"])
    pairs, z_fine = list(seen["pairs"]), seen["z_fine"]
    # (3) the path
    assert calls == C.EXPECTED_CALLS[((nc, nf), loss_kind)], calls
    assert len(pairs) == 1 and pairs[0].pending is None and pairs[0].between is None and pairs[0].sink is None
    assert ray_sink is not None and ray_sink.hold is None
    assert getattr(code_sink, "hold", None) is None and not code_sink.pending
    for k in C.LEAVES:
        assert grads[k] is not None and torch.isfinite(grads[k]).all(), k
    # (2) float64, on the kernels' fine depths
    tag = f"pair_paths_eval[{nc}+{nf},{loss_kind}]"
    l64, g64, _ = C.eval_reference(inp, nc, nf, loss_kind, torch.float64, z_fine=z_fine)
    margin(tag, "loss", abs(loss - l64), 1e-5 * max(1.0, abs(l64)))
    for k, e in C.relative_errors(grads, g64).items():
        margin(tag, "d " + k, e, C.RTOL)
    # (1) the unpaired step
    _reset(seen)
    monkeypatch.setattr(A, "new_field_pair", lambda: None)
    loss_u, grads_u, _, _ = _eval_step(dev, inp, nc, nf, loss_kind, eval_models)
    assert seen["multi"] == 0 and seen["flush"] == 0
    assert torch.equal(seen["z_fine"], z_fine)
    diff = {k: (grads[k] - grads_u[k]).abs().max().item() / max(grads_u[k].abs().max().item(), 1e-30)
            for k in C.LEAVES}
    print("PAIR_PATH_BITS", tag, "loss", loss - loss_u, {k: float(f"{v:.3e}") for k, v in diff.items()})
    assert loss == loss_u, (loss, loss_u)
    for k in C.LEAVES:
        assert torch.equal(grads[k], grads_u[k]), (k, diff[k])


@pytest.mark.parametrize("nc,nf,loss_kind", [(16, 16, "fine"), (16, 16, "coarse"), (32, 24, "coarse")])
def test_eval_field_backs_up_alone_codes_frozen(dev, monkeypatch, eval_models, nc, nf, loss_kind):
    """The same step with the codes constant (pose only), for the three cases in which a field waits alone
    and every field has a multiple of 16 samples: nothing but PoseRays.backward is left to run the
    waiting field before its sums are read -- with leaf codes CodeGradSink.take() gets there first.
    d(theta, phi, rho) bit for bit the unpaired step's and within the float64 reference's bound; one
    flush, none pending.  Before PoseRays.backward ran the waiting field these gradients silently lacked
    its rays: nothing raised."""
    from codenerf import autograd as A
    from conftest import margin
    seen, real = _spies(monkeypatch)
    inp = C.eval_inputs(nc, nf)
    loss, grads, ray_sink, code_sink = _eval_step(dev, inp, nc, nf, loss_kind, eval_models, train_codes=False)
    assert (seen["multi"], seen["x3"], seen["flush"]) == C.EXPECTED_CALLS[((nc, nf), loss_kind)] == (0, 1, 1)
    assert code_sink is None and grads["z_s"] is None and grads["z_t"] is None
    assert ray_sink.hold is None and len(seen["pairs"]) == 1 and seen["pairs"][0].pending is None
    z_fine = seen["z_fine"]
    tag = f"pair_paths_eval[{nc}+{nf},{loss_kind},codes frozen]"
    l64, g64, _ = C.eval_reference(inp, nc, nf, loss_kind, torch.float64, z_fine=z_fine)
    margin(tag, "loss", abs(loss - l64), 1e-5 * max(1.0, abs(l64)))
    pose = ("theta", "phi", "rho")
    err = C.relative_errors({k: (grads[k] if k in pose else g64[k]) for k in C.LEAVES}, g64)
    for k in pose:
        margin(tag, "d " + k, err[k], C.RTOL)
    _reset(seen)
    monkeypatch.setattr(A, "new_field_pair", lambda: None)
    loss_u, grads_u, _, _ = _eval_step(dev, inp, nc, nf, loss_kind, eval_models, train_codes=False)
    assert seen["flush"] == 0 and torch.equal(seen["z_fine"], z_fine) and loss == loss_u
    for k in pose:
        assert torch.equal(grads[k], grads_u[k]), (k, (grads[k] - grads_u[k]).abs().max().item())


# ---------------------------------------------------------------- the training step

TRAIN_RAYS = 64
# case -> (the loss's images, the model whose .grad is set before the backward, on_grads calls,
#          cn_field_backward_train_multi calls: fields per call; the per-field call is a call of one)
TRAIN_CASES = {
    "both": ("both", None, 1, [2]),
    "fine": ("fine", None, 0, [1]),              # the fine field waits, its partner never runs
    "coarse": ("coarse", None, 0, [1]),
    # fresh zeros instead of slots for the fine field, reached first: it runs at once (the per-field call),
    # the coarse one then waits alone
    "both,fine_grad_set": ("both", "nerf_fine", 0, [1, 1]),
    # the fine field waits; the coarse one joins it with fresh zeros, returned through autograd
    "both,coarse_grad_set": ("both", "nerf_coarse", 0, [2]),
}


def _train_step(dev, loss_kind, preset, on_grads):
    """train_minibatch's pieces (train.py) with the loss's images chosen -> {name: .grad or None}."""
    import numpy as np
    from codenerf import autograd as A, nerf, synthetic, train as T
    from codenerf.nerf import PointSampler
    from test_gpu_train import _opt_cfg, _train_models
    torch.manual_seed(0)
    models = _train_models(dev, 3)
    opt, _ = T.prepare_optimizer(_opt_cfg(), models)
    ps = PointSampler(16, 16, C.NEAR, C.FAR, spacing_mode="lindepth", perturb=True, dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(5)
    ro = (torch.randn(TRAIN_RAYS, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 1.3])).to(dev)
    rd = (torch.randn(TRAIN_RAYS, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0])).to(dev)
    target = torch.rand(TRAIN_RAYS, 4, generator=g).to(dev)
    ids = torch.full((TRAIN_RAYS,), 1, dtype=torch.int64, device=dev)
    ids._cn_host_ids = np.full(TRAIN_RAYS, 1, dtype=np.int64)
    t_rand, u = synthetic.uniforms01(22, 1, (TRAIN_RAYS, 16)).to(dev), synthetic.uniforms01(22, 2, (TRAIN_RAYS, 16)).to(dev)
    codes = models["embedding"](ids)
    with A.paired_fields(on_grads=on_grads):
        out = nerf.render_rays(ro, rd, *codes, ps, embedders(dev), models["nerf_coarse"], models["nerf_fine"],
                               t_rand=t_rand, u=u)
    rgb_c = out["rgb_coarse"] if loss_kind in ("both", "coarse") else None
    rgb_f = out["rgb_fine"] if loss_kind in ("both", "fine") else None
    shape_params, texture_params = T.get_params_tensor(models["embedding"], False)
    loss, _ = T.render_loss_autograd(rgb_c, rgb_f, target, shape_params, texture_params, 1, C.LAM)
    opt.zero_grad()
    if preset is not None:
        for p in models[preset].parameters():
            p.grad = torch.full_like(p, 0.25)
    A.backward_from(loss)
    torch.cuda.synchronize()
    return {f"{k}.{n}": (None if p.grad is None else p.grad.detach().clone())
            for k, m in models.items() for n, p in m.named_parameters()}


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_train_field_backs_up_alone(dev, monkeypatch, case):
    """One training step (64 rays, 16 + 16 samples, one object, fp32, weights trained) with the loss on
    both images, the fine one or the coarse one, and with one model's .grad already set so that its field
    gets fresh zeros and does not wait: every parameter's and both code tables' .grad bit for bit the
    unpaired step's; what the loss does not reach is None or zero in both; on_grads runs once when both
    fields run in the shared call into the optimiser's slots, and never otherwise.

    Before CodeGradSink.take() ran a waiting field itself, "fine", "coarse" and "both,fine_grad_set"
    raised from the end-of-pass callback: the tables' gradient rows had been handed out before it."""
    from codenerf import autograd as A
    loss_kind, preset, n_on_grads, multi_calls = TRAIN_CASES[case]
    seen, real = _spies(monkeypatch)
    called = []
    got = _train_step(dev, loss_kind, preset, lambda: called.append(1))
    assert len(called) == n_on_grads, called
    assert seen["train_multi"] == multi_calls, seen["train_multi"]
    assert len(seen["pairs"]) == 1 and seen["pairs"][0].pending is None
    _reset(seen)
    monkeypatch.setattr(A, "new_field_pair", lambda: None)
    want = _train_step(dev, loss_kind, preset, None)
    assert seen["train_multi"] == [1] * (2 if loss_kind == "both" else 1), seen["train_multi"]
    unreached = {"both": (), "fine": ("nerf_coarse.",), "coarse": ("nerf_fine.",)}[loss_kind]
    for k in want:
        a, b = got[k], want[k]
        if unreached and k.startswith(unreached):
            assert (a is None or not a.any()) and (b is None or not b.any()), k
            continue
        assert a is not None and b is not None, k
        assert torch.equal(a, b), (k, (a - b).abs().max().item())
        assert a.any(), k
