"""Training step on the HIP kernels.

* codenerf.optim.AdamW -- one cn_adamw_step launch over flat buffers -- against
  torch.optim.AdamW on the CPU, the optimiser the reference instantiates
  (utils/util.py:159-164), over several steps under LambdaLR with per-group learning
  rates, including a step where one parameter has no gradient (skipped, as in torch).
  ADAM_RTOL is relative to each tensor's largest magnitude: the same fp32 op sequence,
  but torch's CPU kernels may contract a mul+add into an FMA in their scalar tails.
* one train.py:92-114 chunk step (embedding lookup -> 16+16 render -> losses ->
  backward -> AdamW -> LambdaLR) against torch autograd over the oracle on the same
  parameters: the loss within 1e-5 and every parameter / code-table gradient within
  GRAD_RTOL, for chunks holding one object and several (the per-object code index).
* a whole train_iteration (ray sampling, target gather, chunk loop) runs and steps.
"""
import types

import numpy as np
import pytest
import torch

from test_gpu_grad import (GRAD_RTOL, MASK_BAND, O, check_mask_agreement, close, dev, embedders,  # noqa: F401
                           explained_by_kinks, model, oracle_params)

pytestmark = pytest.mark.gpu

ADAM_RTOL = 1e-6
NS = types.SimpleNamespace


def test_adamw_matches_torch(dev):
    from codenerf.optim import AdamW
    g = torch.Generator().manual_seed(0)
    shapes = [[(256, 63), (256,), (3, 512), (3,)], [(257, 512), (257,)], [(40, 256), (40, 256)]]
    lrs = [1e-4, 2e-4, 1e-3]
    cpu = [[torch.nn.Parameter(torch.randn(*s, generator=g) * 0.1) for s in grp] for grp in shapes]
    gpu = [[torch.nn.Parameter(p.detach().clone().to(dev)) for p in grp] for grp in cpu]
    ref = torch.optim.AdamW([{"params": grp, "lr": lr} for grp, lr in zip(cpu, lrs)], lr=1e-4, foreach=False)
    opt = AdamW([{"params": grp, "lr": lr} for grp, lr in zip(gpu, lrs)], lr=1e-4)
    lam = lambda e: 0.1 ** (e / 3)  # noqa: E731
    s_ref = torch.optim.lr_scheduler.LambdaLR(ref, lam)
    s_opt = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    pc = [p for grp in cpu for p in grp]
    pg = [p for grp in gpu for p in grp]
    for it in range(6):
        for a, b in zip(pc, pg):
            scale = 10.0 ** float(torch.randint(-6, 1, (1,), generator=g))
            gr = torch.randn(a.shape, generator=g) * scale
            a.grad, b.grad = gr.clone(), gr.to(dev)
        if it == 3:
            pc[1].grad = None
            pg[1].grad = None
        ref.step()
        opt.step()
        s_ref.step()
        s_opt.step()
        ref.zero_grad()
        opt.zero_grad()
    for a, b in zip(pc, pg):
        close(b.detach(), a.detach(), ADAM_RTOL, "param")
        close(opt.state[b]["exp_avg"], ref.state[a]["exp_avg"], ADAM_RTOL, "exp_avg")
        close(opt.state[b]["exp_avg_sq"], ref.state[a]["exp_avg_sq"], ADAM_RTOL, "exp_avg_sq")
        assert float(opt.state[b]["step"]) == float(ref.state[a]["step"])
    assert float(opt.state[pg[1]]["step"]) == 5.0


def test_adamw_graph_step_equals_step(dev):
    """The graph-capturable update (graph_scalars + graph_step: cn_adamw_scalars folded on the host,
    cn_adamw_step_dev reading them from device memory) is bit-identical to step()."""
    import numpy as np
    from codenerf.optim import AdamW
    g = torch.Generator().manual_seed(2)
    shapes = [[(256, 63), (3,)], [(40, 256)]]
    lrs = [1e-3, 3e-4]
    base = [[torch.randn(*s, generator=g) * 0.1 for s in grp] for grp in shapes]
    sets = []
    for _ in range(2):
        ps = [[torch.nn.Parameter(t.clone().to(dev)) for t in grp] for grp in base]
        sets.append((ps, AdamW([{"params": grp, "lr": lr, "weight_decay": 0.05} for grp, lr in zip(ps, lrs)])))
    (pa, oa), (pb, ob) = sets
    flat_a = [p for grp in pa for p in grp]
    flat_b = [p for grp in pb for p in grp]
    ob.zero_grad(set_to_none=False)
    scal = torch.zeros(3 * 8, dtype=torch.float32, device=dev)
    host = np.zeros(3 * 8, dtype=np.float32)
    for it in range(4):
        grads = [torch.randn(p.shape, generator=g).to(dev) * 10.0 ** (-it) for p in flat_a]
        oa.zero_grad()
        for p, gr in zip(flat_a, grads):
            p.grad = gr.clone()
        oa.step()
        for p, gr in zip(flat_b, grads):
            p.grad.copy_(gr)
        ob.graph_scalars(host)
        scal.copy_(torch.from_numpy(host))
        ob.graph_step(scal)
    torch.cuda.synchronize()
    for a, b in zip(flat_a, flat_b):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"])
        assert float(oa.state[a]["step"]) == float(ob.state[b]["step"]) == 4.0


def test_adamw_state_dict_interop(dev):
    """Optimiser checkpoints (train.py:130-137) move between this AdamW and torch.optim.AdamW."""
    from codenerf.optim import AdamW
    g = torch.Generator().manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(64, 32, generator=g).to(dev)) for _ in range(3)]
    opt = AdamW([{"params": ps[:2]}, {"params": ps[2:], "lr": 1e-3}], lr=1e-4)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).to(dev)
        opt.step()
    ref_ps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ref = torch.optim.AdamW([{"params": ref_ps[:2]}, {"params": ref_ps[2:], "lr": 1e-3}], lr=1e-4)
    ref.load_state_dict(opt.state_dict())
    for p, q in zip(ps, ref_ps):
        assert torch.equal(ref.state[q]["exp_avg"], opt.state[p]["exp_avg"])
        assert float(ref.state[q]["step"]) == 2.0
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = AdamW([{"params": qs[:2]}, {"params": qs[2:], "lr": 1e-3}], lr=1e-4)
    opt2.load_state_dict(ref.state_dict())
    f = opt2.flat_buffers()
    for p, q in zip(ps, qs):
        st = opt2.state[q]
        assert torch.equal(st["exp_avg_sq"], opt.state[p]["exp_avg_sq"])
        assert st["exp_avg"].data_ptr() - f["exp_avg"].data_ptr() == q.data_ptr() - f["param"].data_ptr()
    for p, q in zip(ps, qs):                     # both continue identically
        gr = torch.randn(p.shape, generator=g).to(dev)
        p.grad, q.grad = gr.clone(), gr.clone()
    opt.step()
    opt2.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach())


def _train_models(dev, n_obj, case=None):
    """Synthetic nets; case "t4" / "t3": trained-magnitude weights (synthetic.TRAINED_CASES: weights
    x4 / x3, sigma_raw in the 10-50 range) and unit-variance codes."""
    from codenerf import synthetic
    from codenerf.models import CodeNeRFModel, ShapeTextureEmbedding
    emb = ShapeTextureEmbedding(n_obj, 256, 256)
    g = torch.Generator().manual_seed(11)
    std = 1.0 if case else 0.3
    with torch.no_grad():
        emb.shape_embedding.weight.copy_(torch.randn(n_obj, 256, generator=g) * std)
        emb.texture_embedding.weight.copy_(torch.randn(n_obj, 256, generator=g) * std)

    def field(seed):
        if case is None:
            return model(dev, seed)
        m = CodeNeRFModel(hidden_size=256, shape_code_size=256, texture_code_size=256, num_encoding_fn_xyz=10,
                          num_encoding_fn_dir=4)
        m.load_state_dict(synthetic.trained_params(seed, case))
        return m.to(dev)
    return {"embedding": emb.to(dev), "nerf_coarse": field(0), "nerf_fine": field(1)}


def _opt_cfg():
    return NS(optimizer=NS(type="AdamW", lr=1e-4, embedding_lr=1e-3, scheduler_gamma=0.1,
                           scheduler_step_size=5000000))


@pytest.mark.parametrize("chunk,mixed,precision,case,host", [
    (64, False, "f32", None, False), (128, True, "f32", None, False), (64, False, "bf16x3", None, False),
    (128, True, "bf16x3", None, False), (64, False, "f32", "t4", False), (128, True, "bf16x3", "t4", False),
    (64, False, "f32", None, True), (128, True, "f32", None, True), (64, False, "bf16x3", "t4", True)])
def test_train_minibatch_matches_oracle(dev, monkeypatch, chunk, mixed, precision, case, host):
    """One chunk step vs the oracle three ways: (1) fully independent (its own fine depths and
    ReLU decisions) at INDEPENDENT_RTOL; (2) the kernels' discrete decisions -- fine depths and
    ReLU masks read from the saved activations -- agree with the oracle's up to the precision's
    rounding band; (3) with those decisions fed to the oracle, every gradient matches at GRAD_RTOL.
    precision: the field kernels' arithmetic (models' precision = train_precision); bf16x3 runs the
    3xbf16 fused training pair (32 coarse + 32 fine samples: one code row per 32-sample wave).
    case "t4": trained-magnitude weights and codes (the 3xbf16 error grows with sum |w x|).
    host: the chunk's ids also given on the host (``_cn_host_ids``, as train_iteration hands them
    over): one-object chunks take the table-row view path (_TableRow, the gradient written into the
    optimiser's slot), mixed ones the host-unique + searchsorted path."""
    from codenerf import ops, train as T
    from codenerf.nerf import PointSampler
    seen = {"z_fine": None, "saved": [], "w_coarse": None}
    real_pdf, real_train, real_w16 = ops.sample_pdf, ops.radiance_field_train, ops.radiance_field_train_w16

    def spy_pdf(*a, **k):
        r = real_pdf(*a, **k)
        seen["z_fine"] = r[1].detach().cpu()
        seen["w_coarse"] = a[2].detach().cpu().clone()       # the kernel's weights[..., 1:-1]
        return r

    def spy_train(*a, **k):
        raw, saved = real_train(*a, **k)
        seen["saved"].append(saved)
        return raw, saved
    def spy_w16(*a, **k):           # the fused training path (one code row per wave)
        raw, saved, masks = real_w16(*a, **k)
        seen["saved"].append(saved)
        seen["fused"] = k.get("precision", "f32")
        return raw, saved, masks
    monkeypatch.setattr(ops, "sample_pdf", spy_pdf)
    monkeypatch.setattr(ops, "radiance_field_train", spy_train)
    monkeypatch.setattr(ops, "radiance_field_train_w16", spy_w16)

    def relu_masks(saved):
        sv = saved.detach().cpu()
        return {k: (sv[i] > 0).float() for k, i in (("h1", 0), ("h2", 1), ("v1", 3), ("v2", 4))}
    o = O()
    n_obj, n, lam = 3, 128, 1e-5
    models = _train_models(dev, n_obj, case)
    for key in ("nerf_coarse", "nerf_fine"):
        models[key].precision = models[key].train_precision = precision
    S = 32 if precision == "bf16x3" else 16
    g = torch.Generator().manual_seed(chunk)
    ro = torch.randn(n, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 1.3])
    rd = torch.randn(n, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0])
    ids = torch.randint(0, n_obj, (n,), generator=g) if mixed else torch.tensor([0] * 64 + [2] * 64)
    tgt = torch.rand(n, 4, generator=g)
    opt, sched = T.prepare_optimizer(_opt_cfg(), models)
    ps = PointSampler(S, S, 0.8, 1.8, spacing_mode="lindepth", perturb=False, dtype=torch.float32, device=dev)
    emb = embedders(dev)
    smp, ecfg = o.Sampling(S, S, 0.8, 1.8), o.EmbedCfg()
    for c0 in range(0, n, chunk):
        sl = slice(c0, c0 + chunk)
        r, d = ro[sl], rd[sl]
        snap = {"pc": oracle_params(models["nerf_coarse"]), "pf": oracle_params(models["nerf_fine"]),
                "ts": models["embedding"].shape_embedding.weight.detach().cpu().clone(),
                "tt": models["embedding"].texture_embedding.weight.detach().cpu().clone()}
        seen["saved"].clear()
        seen["fused"] = None
        ids_d = ids[sl].to(dev)
        if host:
            ids_d._cn_host_ids = ids[sl].numpy()
        logs = T.train_minibatch(models, opt, sched, ps, emb, ro[sl].to(dev), rd[sl].to(dev), ids_d,
                                 tgt[sl].to(dev), lam)

        def oracle_step(masks_c=None, masks_f=None, z_f=None, pre_c=None, pre_f=None):
            """The reference's chunk step under torch autograd on the pre-step parameters."""
            pc = {k: v.detach().clone().requires_grad_(True) for k, v in snap["pc"].items()}
            pf = {k: v.detach().clone().requires_grad_(True) for k, v in snap["pf"].items()}
            ts, tt = snap["ts"].clone().requires_grad_(True), snap["tt"].clone().requires_grad_(True)
            zs, zt = ts[ids[sl]], tt[ids[sl]]
            pts_c, z_c = o.sample_uniform(r, d, smp.bins, None)
            rgb_c, _, _, w_c, _ = o.volume_render(o.forward_pass(pc, ecfg, d, pts_c, zs, zt, masks_c, pre_c), z_c, d)
            if z_f is None:
                z_f = o.sample_pdf(r, d, w_c.detach()[..., 1:-1], z_c, S)[1]
            pts_f = r[..., None, :] + d[..., None, :] * z_f[..., :, None]
            rgb_f = o.volume_render(o.forward_pass(pf, ecfg, d, pts_f, zs, zt, masks_f, pre_f), z_f, d)[0]
            lc = torch.nn.functional.mse_loss(rgb_c[..., :3], tgt[sl, :3])
            lf = torch.nn.functional.mse_loss(rgb_f[..., :3], tgt[sl, :3])
            loss = lc + lf + lam * (torch.norm(ts.detach(), p=2) + torch.norm(tt.detach(), p=2))
            loss.backward()
            return loss.item(), pc, pf, ts, tt, z_f, w_c.detach(), z_c

        def grads_of(res):
            _, pc, pf, ts, tt = res[:5]
            out = {f"{key}.{name}": ref[name].grad for key, ref in (("nerf_coarse", pc), ("nerf_fine", pf))
                   for name in ref}
            out.update({"shape table": ts.grad, "texture table": tt.grad})
            return out

        got = {f"{key}.{name}": prm.grad for key in ("nerf_coarse", "nerf_fine")
               for name, prm in models[key].named_parameters()}
        got.update({"shape table": models["embedding"].shape_embedding.weight.grad,
                    "texture table": models["embedding"].texture_embedding.weight.grad})

        # 1. the oracle on its OWN decisions (fine depths, ReLU kinks): independent of the kernels
        pre_c, pre_f = {}, {}
        own = oracle_step(pre_c=pre_c, pre_f=pre_f)
        assert abs(float(logs["total_loss"]) - own[0]) <= 1e-5 * max(1.0, abs(own[0]))
        # 2. the kernels' discrete decisions are the reference's up to their rounding:
        #    (a) coarse weights within 1e-5 of the oracle's, (b) sample_pdf of those weights is the
        #    kernel's z_fine bit for bit, (c) every differing ReLU decision is inside the fp32 band
        w_own, z_c = own[6], own[7]
        assert (seen["w_coarse"] - w_own[..., 1:-1]).abs().max().item() <= 1e-5
        assert seen["fused"] == precision, f"the fused {precision} training path did not run"
        assert torch.equal(o.sample_pdf(r, d, seen["w_coarse"], z_c, S)[1], seen["z_fine"])
        # the fine masks against the oracle's own decisions at the kernel's fine depths (a depth that
        # moved across a cdf bin -- trained nets' peaky weights -- moves its whole sample)
        pre_f_k = {}
        oracle_step(z_f=seen["z_fine"], pre_f=pre_f_k)
        n_dis = (check_mask_agreement(relu_masks(seen["saved"][0]), pre_c, MASK_BAND[precision], "coarse")
                 + check_mask_agreement(relu_masks(seen["saved"][1]), pre_f_k, MASK_BAND[precision], "fine"))
        z_dis = int((seen["z_fine"] != own[5]).sum())
        print(f"chunk {c0}: differing ReLU decisions (all in-band) {n_dis}, differing fine depths {z_dis}")
        # 3. with exactly those decisions the oracle matches every gradient at GRAD_RTOL ...
        fed = oracle_step(relu_masks(seen["saved"][0]), relu_masks(seen["saved"][1]), seen["z_fine"])
        assert abs(float(logs["total_loss"]) - fed[0]) <= 1e-5 * max(1.0, abs(fed[0]))
        g_own, g_fed = grads_of(own), grads_of(fed)
        for k in got:
            close(got[k], g_fed[k], GRAD_RTOL, "recorded decisions " + k)
            # ... so every deviation from the independent oracle is what the in-band kinks move
            explained_by_kinks(got[k], g_own[k], g_fed[k], k)
            if n_dis == 0 and z_dis == 0:
                close(got[k], g_own[k], GRAD_RTOL, "independent " + k)
    assert float(opt.state[models["nerf_fine"].fc_rgb.weight]["step"]) == n // chunk
    assert sched.last_epoch == n // chunk


@pytest.mark.parametrize("mixed", [False, True])
def test_host_id_lookup_bitwise(dev, mixed):
    """The production embedding lookups (codenerf.train hands each chunk's ids over from the host:
    one object -> _TableRow views writing the optimiser's gradient slot; several -> host unique +
    device searchsorted) against the torch.unique lookup: after three chunk steps every gradient
    and every parameter -- the code tables included -- is bit-identical for one-object chunks (the
    deterministic step); with several objects per chunk the code gradients are float-atomic sums
    (DESIGN.md section 4), so the two agree to fp32 reassociation."""
    from codenerf import train as T
    from codenerf.nerf import PointSampler
    runs = []
    for host in (False, True):
        torch.manual_seed(3)
        models = _train_models(dev, 4)
        opt, sched = T.prepare_optimizer(_opt_cfg(), models)
        ps = PointSampler(16, 16, 0.8, 1.8, spacing_mode="lindepth", perturb=False, dtype=torch.float32, device=dev)
        g = torch.Generator().manual_seed(5)
        grads = []
        for step in range(3):
            n = 192
            ro = (torch.randn(n, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 1.3])).to(dev)
            rd = (torch.randn(n, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0])).to(dev)
            ids_h = torch.randint(0, 4, (n,), generator=g) if mixed else torch.full((n,), (step * 3) % 4)
            ids = ids_h.to(dev)
            if host:
                ids._cn_host_ids = ids_h.numpy()
            tgt = torch.rand(n, 4, generator=g).to(dev)
            T.train_minibatch(models, opt, sched, ps, embedders(dev), ro, rd, ids, tgt, 1e-5)
            grads.append({f"{k}.{n_}": p.grad.detach().clone() for k, m in models.items()
                          for n_, p in m.named_parameters() if p.grad is not None})
        torch.cuda.synchronize()
        params = {f"{k}.{n_}": p.detach().clone() for k, m in models.items() for n_, p in m.named_parameters()}
        runs.append((grads, params))
    (g0, p0), (g1, p1) = runs
    for a, b in zip(g0, g1):
        assert a.keys() == b.keys()
        for k in a:
            if mixed:
                close(b[k], a[k], 1e-5, ("grad", k))
            else:
                assert torch.equal(a[k], b[k]), ("grad", k)
    for k in p0:
        if mixed:
            assert (p0[k] - p1[k]).abs().max().item() <= 2.05 * 3 * 1e-3, ("param", k)   # 3 steps, |step| <= lr
        else:
            assert torch.equal(p0[k], p1[k]), ("param", k)


@pytest.mark.parametrize("precision,off", [("f32", "sink"), ("bf16x3", "sink"), ("f32", "prefetch")])
def test_step_fusions_bitwise(dev, monkeypatch, precision, off):
    """The training step's launch merges against the plain route, three steps of one-object chunks, every
    gradient and parameter bit-identical:
    * "sink": both fields' code gradients added into the code tables' gradient rows in place
      (CodeGradSink: fp32, one two-field cn_code_dz launch per step; 3xbf16, each field's
      accumulate_dz launch), the tables' .grad the optimiser's flat slices, vs dz returned, summed by
      autograd and added into the row;
    * "prefetch": both fields' pre-field launches as one (cn_field_prepare_models, once per step) vs one
      per field."""
    from codenerf import autograd as A, ops, train as T
    from codenerf.models import model as M
    from codenerf.nerf import PointSampler
    real_dz, real_pm = ops.code_dz, ops.field_prepare_models
    calls = {"sunk": [], "models": []}

    def spy_dz(jobs, *a, **k):
        calls["sunk"].append((len(jobs), k.get("dz_into") is not None))
        return real_dz(jobs, *a, **k)

    def spy_pm(models, *a, **k):
        calls["models"].append(len(models))
        return real_pm(models, *a, **k)
    monkeypatch.setattr(ops, "code_dz", spy_dz)
    monkeypatch.setattr(ops, "field_prepare_models", spy_pm)
    S = 32 if precision == "bf16x3" else 16
    runs = []
    for on in (True, False):
        if not on and off == "sink":
            monkeypatch.setattr(M.CodeGradSink, "rows", lambda self: None)
        if not on and off == "prefetch":
            monkeypatch.setattr(A, "prefetch_render_prepares", lambda *a, **k: False)
        calls.update(sunk=[], models=[])
        torch.manual_seed(3)
        models = _train_models(dev, 4)
        for key in ("nerf_coarse", "nerf_fine"):
            models[key].precision = models[key].train_precision = precision
        opt, sched = T.prepare_optimizer(_opt_cfg(), models)
        ps = PointSampler(S, S, 0.8, 1.8, spacing_mode="lindepth", perturb=False, dtype=torch.float32, device=dev)
        g = torch.Generator().manual_seed(5)
        grads = []
        for step in range(3):
            n = 192
            ro = (torch.randn(n, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 1.3])).to(dev)
            rd = (torch.randn(n, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0])).to(dev)
            ids_h = torch.full((n,), (step * 3) % 4)
            ids = ids_h.to(dev)
            ids._cn_host_ids = ids_h.numpy()
            tgt = torch.rand(n, 4, generator=g).to(dev)
            T.train_minibatch(models, opt, sched, ps, embedders(dev), ro, rd, ids, tgt, 1e-5)
            grads.append({f"{k}.{n_}": p.grad.detach().clone() for k, m in models.items()
                          for n_, p in m.named_parameters() if p.grad is not None})
            if on and off == "sink":
                flat = opt.flat_buffers()["grad"]
                lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
                for w in (models["embedding"].shape_embedding.weight, models["embedding"].texture_embedding.weight):
                    assert lo <= w.grad.data_ptr() < hi, "the table's .grad is not the optimiser's flat slice"
        if off == "sink" and precision == "f32":
            # sink: one two-field dz launch per step into the table rows; else one per field, returned
            assert calls["sunk"] == ([(2, True)] * 3 if on else [(1, False)] * 6), calls
        elif off == "prefetch":
            assert calls["models"] == ([2] * 3 if on else [1] * 6), calls
        torch.cuda.synchronize()
        params = {f"{k}.{n_}": p.detach().clone() for k, m in models.items() for n_, p in m.named_parameters()}
        runs.append((grads, params))
    (g0, p0), (g1, p1) = runs
    for step, (a, b) in enumerate(zip(g0, g1)):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), ("grad", step, k)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), ("param", k)


def test_train_iteration_runs(dev):
    from codenerf import nerf as N, synthetic, train as T
    from codenerf.evaluate import pose_spherical
    cfg = NS(is_distributed=False,
             models=NS(embedding=NS(shape_code_size=256, texture_code_size=256), nerf_coarse=NS(hidden_size=256),
                       nerf_fine=NS(hidden_size=256)),
             nerf=NS(embedder=NS(num_encoding_fn_xyz=10, include_input_xyz=True, log_sampling_xyz=True,
                                 num_encoding_fn_dir=4, include_input_dir=True, log_sampling_dir=True,
                                 use_viewdirs=True),
                     ray_sampler=NS(num_random_rays=96),
                     point_sampler=NS(num_coarse=16, num_fine=16, near_limit=0.8, far_limit=1.8,
                                      spacing_mode="lindepth", perturb=True),
                     train=NS(chunksize=64)),
             optimizer=_opt_cfg().optimizer, experiment=NS(regularizer_lambda=1e-5))
    torch.manual_seed(0)
    np.random.seed(0)
    models = T.prepare_models(cfg, 5, dev)
    opt, sched = T.prepare_optimizer(cfg, models)
    samplers = N.prepare_samplers(cfg, 32, 32, synthetic.srn_intrinsics(32, 35.0), torch.float32, dev)
    embs = N.prepare_embedders(cfg, torch.float32, dev)
    poses = torch.stack([pose_spherical(torch.tensor(0.5 + 0.4 * i), torch.tensor(0.3), torch.tensor(1.3))
                         for i in range(2)])
    data = {"color": torch.rand(2, 32, 32, 4).to(dev), "pose": poses.to(dev), "object_id": torch.tensor([1, 3]).to(dev)}
    before = [p.detach().clone() for p in models["nerf_fine"].parameters()]
    logs = T.train_iteration(cfg, data, models, opt, sched, samplers, embs)
    assert len(logs) == 3                        # 2 x 96 rays in chunks of 64 (the middle one holds both objects)
    assert all(np.isfinite(float(lg["total_loss"])) for lg in logs)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, models["nerf_fine"].parameters()))
    assert sched.last_epoch == 3


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_train_minibatch_deterministic(dev, precision):
    """Chunk steps with one object per chunk (every C3 step) are bit-reproducible in both precisions:
    g_code is formed by fixed-order column sums folded into the dW GEMMs (no float atomics in the step),
    so two identical model sets stepped on the same chunks end bit-identical -- what a checkpoint resume
    relies on (train.py:129-138 + util.py:175-213)."""
    from codenerf import train as T
    from codenerf.nerf import PointSampler
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        models = _train_models(dev, 3)
        for key in ("nerf_coarse", "nerf_fine"):
            models[key].precision = models[key].train_precision = precision
        opt, sched = T.prepare_optimizer(_opt_cfg(), models)
        S = 32 if precision == "bf16x3" else 16     # the 3xbf16 backward: one code row per 32-sample wave
        ps = PointSampler(S, S, 0.8, 1.8, spacing_mode="lindepth", perturb=True, dtype=torch.float32, device=dev)
        g = torch.Generator().manual_seed(5)
        for step in range(3):
            n = 256
            ro = (torch.randn(n, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 1.3])).to(dev)
            rd = (torch.randn(n, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0])).to(dev)
            ids = torch.full((n,), step % 3, dtype=torch.int64, device=dev)
            tgt = torch.rand(n, 4, generator=g).to(dev)
            T.train_minibatch(models, opt, sched, ps, embedders(dev), ro, rd, ids, tgt, 1e-5)
        torch.cuda.synchronize()
        runs.append({f"{k}.{n_}": p.detach().clone() for k, m in models.items() for n_, p in m.named_parameters()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


# C3 at-size bounds, per precision, at about twice the achieved error (profiles/r04/parity_margins.json):
# max |g - g_ref| relative to the tensor's largest |g_ref| (full tensors), projections relative to the
# tensor's norm, post-step projections relative to lr sqrt(n).  They sit above GRAD_RTOL (2e-4) because
# the run is independent of the reference's discrete decisions: test_train_c3_decisions_at_size counts
# the fine depths and ReLU decisions that differ and shows that with the kernels' decisions the
# reference's arithmetic (the oracle) matches every gradient at GRAD_RTOL.
C3_GRAD_RTOL = {"f32": 1e-3, "bf16x3": 1.4e-3}
C3_PROJ_RTOL = {"f32": 1.2e-3, "bf16x3": 3.8e-3}
C3_STEP_PROJ = {"f32": 6e-3, "bf16x3": 2.7e-2}


def _proj_directions(idx, shape):
    """make_golden.py proj_directions: 16 seeded N(0, 1) directions for parameter ``idx``."""
    return torch.randn((16,) + tuple(shape), generator=torch.Generator().manual_seed(7000 + idx))


def _proj(r, t):
    return (r.double() * t.detach().double().cpu()[None]).reshape(r.shape[0], -1).sum(1)


def spy_step_images(monkeypatch):
    """The images train_minibatch hands to its loss (train.render_loss_autograd's first two arguments),
    kept as detached copies -> {"rgb_coarse", "rgb_fine"}, filled by the step."""
    from codenerf import train as T
    seen = {}
    real = T.render_loss_autograd

    def spy(rgb_c, rgb_f, *a, **k):
        seen["rgb_coarse"], seen["rgb_fine"] = rgb_c.detach().clone(), rgb_f.detach().clone()
        return real(rgb_c, rgb_f, *a, **k)
    monkeypatch.setattr(T, "render_loss_autograd", spy)
    return seen


def check_step_pixels(tag, seen, g):
    """The step's own rgb_coarse and rgb_fine against the reference's (the fixture's), every pixel and
    channel, at the project's fp32 parity target |d| <= 1e-4."""
    from conftest import margin
    for key in ("rgb_coarse", "rgb_fine"):
        assert seen[key].shape == g[key].shape and seen[key].dtype == torch.float32, key
        margin(tag, key, (seen[key].double() - g[key].double()).abs().max().item(), 1e-4)


_C3_RESULTS = {}
C3_OBJECTS = 2458
C3_IDS = [17, 1234]


def _c3_setup(dev, precision):
    """train_c3.npz's chunk step inputs (make_golden.py gen_c3train): the models before the step, the
    optimiser, the reference's stratified / fine uniforms, the point sampler."""
    from codenerf import synthetic, train as T
    from codenerf.models import CodeNeRFModel, ShapeTextureEmbedding
    from codenerf.nerf import PointSampler
    from test_gpu_parity import load
    g = load("train_c3.npz", dev)
    emb_t = ShapeTextureEmbedding(C3_OBJECTS, 256, 256)
    with torch.no_grad():
        emb_t.shape_embedding.weight.copy_(synthetic.latent_codes(40, C3_OBJECTS))
        emb_t.texture_embedding.weight.copy_(synthetic.latent_codes(41, C3_OBJECTS))
    models = {"embedding": emb_t.to(dev)}
    for key, seed in (("nerf_coarse", 0), ("nerf_fine", 1)):
        m = CodeNeRFModel(hidden_size=256, shape_code_size=256, texture_code_size=256, num_encoding_fn_xyz=10,
                          num_encoding_fn_dir=4)
        m.load_state_dict(synthetic.codenerf_params(seed))
        models[key] = m.to(dev)
        m.precision = m.train_precision = precision
    opt, sched = T.prepare_optimizer(_opt_cfg(), models)
    torch.manual_seed(4343)
    t_rand, u = torch.rand(4096, 64), torch.rand(4096, 64)
    assert torch.equal(t_rand[:4].to(dev), g["t_rand_head"]) and torch.equal(u[:4].to(dev), g["u_head"])
    assert abs(t_rand.double().sum().item() - g["t_rand_sum"].item()) < 0.02   # stored as float32
    assert abs(u.double().sum().item() - g["u_sum"].item()) < 0.02
    ps = PointSampler(64, 64, 0.8, 1.8, spacing_mode="lindepth", perturb=True, dtype=torch.float32, device=dev)
    return g, models, opt, sched, t_rand, u, ps


@pytest.mark.parametrize("host_ids", [False, True])
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_train_c3_chunk_at_size(dev, monkeypatch, precision, host_ids):
    """C3 at size vs the reference's own chunk step (train_c3.npz, make_golden.py gen_c3train:
    train.py:96-114 on one 4096-ray chunk of two objects of a 2458-object table, 64 + 64 perturbed
    samples with the reference's draws, AdamW + LambdaLR), element-wise: the losses; for fp32 the
    rendered rgb_coarse and rgb_fine the step hands to its loss, every pixel at 1e-4; nerf_fine's
    gradients and post-step values in full; for nerf_coarse five tensors in full and 16 seeded
    projections of EVERY tensor's gradient and post-step change; the two touched code rows'
    gradients and values, every untouched row only decayed.  ``host_ids``: the chunk's object ids
    also handed over from the host (``_cn_host_ids``, as train_iteration does); with two objects in
    the chunk the code gradients are float-atomic sums (determinism scope), so
    the two lookups agree to fp32 reassociation, not bit for bit.  Achieved errors are recorded
    (conftest.margin), per tensor for the full ones."""
    from codenerf import train as T
    from conftest import margin
    tag = f"c3_train[{precision}{',host_ids' if host_ids else ''}]"
    g, models, opt, sched, t_rand, u, ps = _c3_setup(dev, precision)
    before = {f"{k}.{n}": p.detach().clone() for k, m in models.items() for n, p in m.named_parameters()}
    ids_t = g["ids"].long()
    if host_ids:
        ids_t._cn_host_ids = g["ids"].long().cpu().numpy()
    seen = spy_step_images(monkeypatch)
    logs = T.train_minibatch(models, opt, sched, ps, embedders(dev), g["ro"], g["rd"], ids_t, g["target"],
                             1e-5, uniforms=(t_rand.to(dev), u.to(dev)))
    torch.cuda.synchronize()
    if precision == "f32":
        check_step_pixels(tag, seen, g)
    got_l = {"lc": logs["nerf_loss_coarse"], "lf": logs["nerf_loss_fine"], "reg": logs["embedding_loss"],
             "loss": logs["total_loss"]}
    for k, v in got_l.items():
        margin(tag, "loss " + k, abs(float(v) - g[k].item()), 1e-5 * max(1.0, abs(g[k].item())))
    rtol, prtol = C3_GRAD_RTOL[precision], C3_PROJ_RTOL[precision]
    named = {f"{k}.{n}": p for k, m in models.items() for n, p in m.named_parameters()}
    ids = C3_IDS
    worst = {"grad": (0.0, ""), "proj": (0.0, ""), "firm_step": (0.0, ""), "step_proj": (0.0, "")}
    per_tensor = {}
    flips = 0
    for idx, k in enumerate(sorted(named)):
        p = named[k]
        if k.startswith("embedding."):
            ref = g["grows_" + k]
            e = (p.grad[ids] - ref).abs().max().item() / ref.abs().max().item()
            margin(tag, "touched rows grad " + k, e, rtol)
            rest = float(p.grad.norm() ** 2 - p.grad[ids].norm() ** 2)
            assert abs(rest) <= 1e-12 and g["gnorm_rest_" + k].item() == 0.0, k
            # after the step: the touched rows moved by about lr; every other row only decays
            fs, nf = _post_step(p.detach()[ids], g["prows_" + k], ref, 1e-3, rtol)
            margin(tag, "touched rows firm post-step " + k, fs, 1e-6)
            flips += nf
            mask = torch.ones(C3_OBJECTS, dtype=torch.bool, device=dev)
            mask[ids] = False
            decayed = before[k][mask] * (1 - 1e-3 * 1e-2)
            assert (p.detach()[mask] - decayed).abs().max().item() <= 1e-7, k
            continue
        lr = 1e-4
        if "g_" + k in g:                                    # full tensors
            ref = g["g_" + k]
            e = (p.grad - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)
            per_tensor[k] = e
            worst["grad"] = max(worst["grad"], (e, k))
            fs, nf = _post_step(p.detach(), g["p_" + k], ref, lr, rtol)
            worst["firm_step"] = max(worst["firm_step"], (fs, k))
            flips += nf
        r = _proj_directions(idx, p.shape)
        gn = max(g["gnorm_" + k].item(), 1e-12)
        ep = (_proj(r, p.grad) - g["gproj_" + k].cpu()).abs().max().item() / gn
        worst["proj"] = max(worst["proj"], (ep, k))
        # post-step change projected: AdamW's first step is ~lr sign(g) per element, so the projection's
        # scale is lr sqrt(n); only elements whose gradient sign is undetermined at rtol can differ
        dp = (_proj(r, p.detach() - before[k]) - g["pproj_" + k].cpu()).abs().max().item()
        worst["step_proj"] = max(worst["step_proj"], (dp / (lr * p.numel() ** 0.5), k))
    margin(tag, "grad full tensors (worst: %s)" % worst["grad"][1], worst["grad"][0], rtol,
           per_tensor={k: float(f"{v:.3e}") for k, v in per_tensor.items()},
           above_grad_rtol=sorted(k for k, v in per_tensor.items() if v > GRAD_RTOL))
    margin(tag, "grad projections (worst: %s)" % worst["proj"][1], worst["proj"][0], prtol)
    margin(tag, "firm post-step (worst: %s)" % worst["firm_step"][1], worst["firm_step"][0], 1e-6,
           sign_undetermined_elements=flips)
    margin(tag, "post-step projections (worst: %s)" % worst["step_proj"][1], worst["step_proj"][0],
           C3_STEP_PROJ[precision])
    assert sched.last_epoch == 1
    if host_ids and precision in _C3_RESULTS:          # the device-id case ran first (parametrize order)
        e = 0.0
        for k, p in named.items():
            a, b = _C3_RESULTS[precision][k]
            e = max(e, (a - p.grad).abs().max().item() / max(a.abs().max().item(), 1e-30))
            assert (b - p.detach()).abs().max().item() <= 2.05 * (1e-3 if k.startswith("embedding.") else 1e-4), k
        margin(tag, "host-id vs device-id lookup (two objects: float-atomic code sums)", e, 1e-5)
    elif not host_ids:
        _C3_RESULTS[precision] = {k: (p.grad.detach().clone(), p.detach().clone()) for k, p in named.items()}


# The reference's runnable training shapes (round 6; make_golden.py gen_train_shape, one object per
# chunk): about twice the errors the first GPU run measured (gpurun_out/r06a, profiles/r06/parity_margins.json:
# full tensors 2.84e-4 / 4.47e-4, projections 9.59e-4 / 7.08e-4; the step is bit-reproducible, so the
# same kernels give the same errors on every box).
SHAPE_GRAD_RTOL = {"train_cars_code": 6e-4, "train_3080": 9e-4}
SHAPE_PROJ_RTOL = {"train_cars_code": 1.9e-3, "train_3080": 1.4e-3}


@pytest.mark.parametrize("name", ["train_cars_code", "train_3080"])
def test_train_shape_chunk_at_size(dev, monkeypatch, name):
    """The reference's own runnable training shapes, one chunk step each vs the reference
    (make_golden.py gen_train_shape): srn-cars-code.yml (Nc 32 / Nf 128: a 160-sample fine pass,
    chunk 4096) and srn-cars-code-3080.yml (64 / 128: 192 fine samples, chunk 1024 -- the first chunk
    of a 4096-ray draw), perturbed samples with the reference's draws, one object per chunk (the
    deterministic path every runnable config takes), AdamW + LambdaLR.  fp32 (the reference's
    precision) through train_minibatch: losses; the rendered rgb_coarse and rgb_fine the step hands to its
    loss (train.render_loss_autograd's first two arguments) against the fixture's, every pixel and channel
    at 1e-4; five gradients in full, 16 projections of every gradient and post-step change, the touched
    code row (gradient and post-step), every other row only decayed.  Run twice: the step (its two images
    included) is bit-reproducible."""
    from codenerf import synthetic, train as T
    from codenerf.models import CodeNeRFModel, ShapeTextureEmbedding
    from codenerf.nerf import PointSampler
    from conftest import margin
    from test_gpu_parity import load
    g = load(name + ".npz", dev)
    nc, nf, chunk = int(g["nc"].item()), int(g["nf"].item()), int(g["chunk"].item())
    near, far = float(g["near"].item()), float(g["far"].item())
    torch.manual_seed(4343)
    t_rand, u = torch.rand(chunk, nc), torch.rand(chunk, nf)
    assert torch.equal(t_rand[:4].to(dev), g["t_rand_head"]) and torch.equal(u[:4].to(dev), g["u_head"])
    runs = []
    seen = spy_step_images(monkeypatch)
    for rep in range(2):
        emb_t = ShapeTextureEmbedding(C3_OBJECTS, 256, 256)
        with torch.no_grad():
            emb_t.shape_embedding.weight.copy_(synthetic.latent_codes(40, C3_OBJECTS))
            emb_t.texture_embedding.weight.copy_(synthetic.latent_codes(41, C3_OBJECTS))
        models = {"embedding": emb_t.to(dev)}
        for key, seed in (("nerf_coarse", 0), ("nerf_fine", 1)):
            m = CodeNeRFModel(hidden_size=256, shape_code_size=256, texture_code_size=256, num_encoding_fn_xyz=10,
                              num_encoding_fn_dir=4)
            m.load_state_dict(synthetic.codenerf_params(seed))
            models[key] = m.to(dev)
        opt, sched = T.prepare_optimizer(_opt_cfg(), models)
        ps = PointSampler(nc, nf, near, far, spacing_mode="lindepth", perturb=True, dtype=torch.float32, device=dev)
        before = {f"{k}.{n}": p.detach().clone() for k, m in models.items() for n, p in m.named_parameters()}
        ids_t = g["ids"].long()
        ids_t._cn_host_ids = g["ids"].long().cpu().numpy()
        logs = T.train_minibatch(models, opt, sched, ps, embedders(dev), g["ro"], g["rd"], ids_t, g["target"],
                                 1e-5, uniforms=(t_rand.to(dev), u.to(dev)))
        torch.cuda.synchronize()
        named = {f"{k}.{n}": p for k, m in models.items() for n, p in m.named_parameters()}
        runs.append({k: (p.grad.detach().clone(), p.detach().clone()) for k, p in named.items()})
        runs[-1].update({k: (v, v) for k, v in seen.items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k][0], runs[1][k][0]) and torch.equal(runs[0][k][1], runs[1][k][1]), \
            ("not bit-reproducible", k)
    tag = f"{name}[f32]"
    check_step_pixels(tag, seen, g)
    for k, key in (("lc", "nerf_loss_coarse"), ("lf", "nerf_loss_fine"), ("reg", "embedding_loss"),
                   ("loss", "total_loss")):
        margin(tag, "loss " + k, abs(float(logs[key]) - g[k].item()), 1e-5 * max(1.0, abs(g[k].item())))
    rtol, prtol = SHAPE_GRAD_RTOL[name], SHAPE_PROJ_RTOL[name]
    oid = int(g["ids"][0].item())
    worst = {"grad": (0.0, ""), "proj": (0.0, ""), "firm_step": (0.0, ""), "step_proj": (0.0, "")}
    flips = 0
    for idx, k in enumerate(sorted(named)):
        p = named[k]
        if k.startswith("embedding."):
            ref = g["grows_" + k]
            margin(tag, "touched row grad " + k, (p.grad[[oid]] - ref).abs().max().item() / ref.abs().max().item(),
                   rtol)
            assert float(p.grad.norm() ** 2 - p.grad[[oid]].norm() ** 2) == 0.0, k
            fs, nf_ = _post_step(p.detach()[[oid]], g["prows_" + k], ref, 1e-3, rtol)
            margin(tag, "touched row firm post-step " + k, fs, 1e-6)
            flips += nf_
            mask = torch.ones(C3_OBJECTS, dtype=torch.bool, device=dev)
            mask[oid] = False
            assert (p.detach()[mask] - before[k][mask] * (1 - 1e-3 * 1e-2)).abs().max().item() <= 1e-7, k
            continue
        lr = 1e-4
        if "g_" + k in g:
            ref = g["g_" + k]
            worst["grad"] = max(worst["grad"], ((p.grad - ref).abs().max().item() / ref.abs().max().item(), k))
            fs, nf_ = _post_step(p.detach(), g["p_" + k], ref, lr, rtol)
            worst["firm_step"] = max(worst["firm_step"], (fs, k))
            flips += nf_
        r = _proj_directions(idx, p.shape)
        gn = max(g["gnorm_" + k].item(), 1e-12)
        perr = _proj(r, p.grad) - g["gproj_" + k].cpu()
        worst["proj"] = max(worst["proj"], (perr.abs().max().item() / gn, k))
        # post-step change, projected: AdamW's first step moves element i by lr q(g_i), q(x) = x / (|x| + eps)
        # (+ the same decay), so an element moves differently only as far as the gradient error e_i moves
        # q: by at most 2 lr where |g_i| <= E (the sign may flip), else by lr eps E / ((|g_i| + eps)
        # (|g_i| - E + eps)) -- with E twice the error norm estimated from the 16 projections
        # (E[(r . e)^2] = |e|^2).  The bound per direction sums those caps weighted by |r| (+ float slack);
        # the error is stated as a fraction of it.
        dp = (_proj(r, p.detach() - before[k]) - g["pproj_" + k].cpu()).abs()
        gd = p.grad.detach().double().cpu().reshape(-1).abs()
        E, eps = 2.0 * perr.pow(2).mean().sqrt().item() + 1e-12, 1e-8
        ci = torch.where(gd <= E, torch.full_like(gd, 2.0), eps * E / ((gd + eps) * (gd - E + eps)))
        cap = 1.05 * lr * (r.double().reshape(r.shape[0], -1).abs() * ci[None]).sum(1) + 1e-3 * lr * p.numel() ** 0.5
        worst["step_proj"] = max(worst["step_proj"], ((dp / cap).max().item(), k))
    margin(tag, "grad full tensors (worst: %s)" % worst["grad"][1], worst["grad"][0], rtol)
    margin(tag, "grad projections (worst: %s)" % worst["proj"][1], worst["proj"][0], prtol)
    margin(tag, "firm post-step (worst: %s)" % worst["firm_step"][1], worst["firm_step"][0], 1e-6,
           sign_undetermined_elements=flips)
    margin(tag, "post-step projections / sign-undetermined cap (worst: %s)" % worst["step_proj"][1],
           worst["step_proj"][0], 1.0)


def _post_step(got, ref, g_ref, lr, rtol):
    """AdamW's first step moves each element by lr g / (|g| + eps) (+ decay): where the reference's
    |g| is well above both eps (1e-8) and the gradient tolerance (rtol x the tensor's max) that is
    lr * sign(g) and must agree to float rounding ("firm"); elsewhere the quotient follows the
    gradient's last digits, so only the step's bound (2 lr) holds.  -> (max firm error, the number
    of non-firm elements that differ by more than float rounding)."""
    d = (got - ref).abs()
    firm = g_ref.abs() > max(1e-6, 10 * rtol * g_ref.abs().max().item())
    assert d.max().item() <= 2.05 * lr, d.max().item()
    return (d[firm].max().item() if firm.any() else 0.0), int(((~firm) & (d > 1e-6)).sum().item())


def test_train_c3_decisions_at_size(dev, monkeypatch):
    """Why the at-size C3 bounds sit above GRAD_RTOL, with counts: the same chunk step (fp32) also
    run by the oracle (the reference's op sequence on the CPU, pinned by the fixture itself here) on
    its OWN discrete decisions and on the KERNELS' -- fine depths from sample_pdf and ReLU masks read
    from the saved activation planes.  (1) the oracle's own run reproduces the reference's gradients
    (the oracle is the reference at size); (2) the kernels' decisions that differ from the oracle's --
    fine depths, ReLU signs -- are counted, every differing ReLU inside the fp32 band of its
    pre-activation; (3) fed those decisions, the oracle matches every kernel gradient at GRAD_RTOL;
    so the at-size gaps are the moved decisions, not the arithmetic."""
    from codenerf import ops, train as T
    from conftest import margin
    o = O()
    seen = {"z_fine": None, "w_coarse": None, "saved": []}
    real_pdf, real_w16 = ops.sample_pdf, ops.radiance_field_train_w16

    def spy_pdf(*a, **k):
        r = real_pdf(*a, **k)
        seen["z_fine"] = r[1].detach().cpu()
        seen["w_coarse"] = a[2].detach().cpu().clone()
        return r

    def spy_w16(*a, **k):
        raw, saved, masks = real_w16(*a, **k)
        sv = saved.detach()
        seen["saved"].append({name: (sv[i] > 0).cpu().float() for name, i in (("h1", 0), ("h2", 1), ("v1", 3), ("v2", 4))})
        return raw, saved, masks
    monkeypatch.setattr(ops, "sample_pdf", spy_pdf)
    monkeypatch.setattr(ops, "radiance_field_train_w16", spy_w16)
    g, models, opt, sched, t_rand, u, ps = _c3_setup(dev, "f32")
    snap = {"pc": oracle_params(models["nerf_coarse"]), "pf": oracle_params(models["nerf_fine"]),
            "ts": models["embedding"].shape_embedding.weight.detach().cpu().clone(),
            "tt": models["embedding"].texture_embedding.weight.detach().cpu().clone()}
    T.train_minibatch(models, opt, sched, ps, embedders(dev), g["ro"], g["rd"], g["ids"].long(), g["target"], 1e-5,
                      uniforms=(t_rand.to(dev), u.to(dev)))
    torch.cuda.synchronize()
    assert len(seen["saved"]) == 2, "the fused fp32 training forward ran for both fields"
    got = {f"{key}.{name}": prm.grad.detach().cpu() for key in ("nerf_coarse", "nerf_fine")
           for name, prm in models[key].named_parameters()}
    got["shape table"] = models["embedding"].shape_embedding.weight.grad[C3_IDS].cpu()
    got["texture table"] = models["embedding"].texture_embedding.weight.grad[C3_IDS].cpu()
    ro, rd, ids, tgt = g["ro"].cpu(), g["rd"].cpu(), g["ids"].long().cpu(), g["target"].cpu()
    smp, ecfg = o.Sampling(64, 64, 0.8, 1.8), o.EmbedCfg()
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))

    def oracle_step(masks_c=None, masks_f=None, z_f=None, pre_c=None, pre_f=None):
        pc = {k: v.detach().clone().requires_grad_(True) for k, v in snap["pc"].items()}
        pf = {k: v.detach().clone().requires_grad_(True) for k, v in snap["pf"].items()}
        ts, tt = snap["ts"].clone().requires_grad_(True), snap["tt"].clone().requires_grad_(True)
        zs, zt = ts[ids], tt[ids]
        pts_c, z_c = o.sample_uniform(ro, rd, smp.bins, t_rand)
        rgb_c, _, _, w_c, _ = o.volume_render(o.forward_pass(pc, ecfg, rd, pts_c, zs, zt, masks_c, pre_c), z_c, rd)
        if z_f is None:
            z_f = o.sample_pdf(ro, rd, w_c.detach()[..., 1:-1], z_c, 64, u)[1]
        pts_f = ro[..., None, :] + rd[..., None, :] * z_f[..., :, None]
        rgb_f = o.volume_render(o.forward_pass(pf, ecfg, rd, pts_f, zs, zt, masks_f, pre_f), z_f, rd)[0]
        lc = torch.nn.functional.mse_loss(rgb_c[..., :3], tgt[..., :3])
        lf = torch.nn.functional.mse_loss(rgb_f[..., :3], tgt[..., :3])
        loss = lc + lf + 1e-5 * (torch.norm(ts.detach(), p=2) + torch.norm(tt.detach(), p=2))
        loss.backward()
        out = {f"nerf_coarse.{k}": v.grad for k, v in pc.items()}
        out.update({f"nerf_fine.{k}": v.grad for k, v in pf.items()})
        out["shape table"], out["texture table"] = ts.grad[C3_IDS], tt.grad[C3_IDS]
        return out, z_f, w_c.detach(), z_c

    # 1. the oracle on its own decisions: the reference's op sequence, on this host's CPU (other
    #    threads / BLAS blocking than the container that wrote the fixture) -- at size it differs
    #    from the reference by the same kind of moved decisions (r04d: 3.0e-4), which is the
    #    problem's conditioning, not the kernels'
    pre_c, pre_f = {}, {}
    own, z_own, w_own, z_c = oracle_step(pre_c=pre_c, pre_f=pre_f)
    e_ref, per = (0.0, ""), {}
    for k in own:
        if ("g_" + k) in g:
            ref = g["g_" + k].cpu()
            per[k] = (own[k] - ref).abs().max().item() / ref.abs().max().item()
            e_ref = max(e_ref, (per[k], k))
    margin("c3_decisions[f32]", "CPU oracle (own decisions) vs reference, full tensors (worst: %s)" % e_ref[1],
           e_ref[0], C3_GRAD_RTOL["f32"], per_tensor={k: float(f"{v:.3e}") for k, v in per.items()})
    # 2. the kernels' discrete decisions against the oracle's
    assert (seen["w_coarse"] - w_own[..., 1:-1]).abs().max().item() <= 1e-5
    assert torch.equal(o.sample_pdf(ro, rd, seen["w_coarse"], z_c, 64, u)[1], seen["z_fine"])
    z_dis = int((seen["z_fine"] != z_own).sum())
    z_far = int(((seen["z_fine"] - z_own).abs() > 1e-4).sum())
    pre_f_k = {}
    oracle_step(z_f=seen["z_fine"], pre_f=pre_f_k)
    n_dis_c = check_mask_agreement(seen["saved"][0], pre_c, MASK_BAND["f32"], "coarse")
    n_dis_f = check_mask_agreement(seen["saved"][1], pre_f_k, MASK_BAND["f32"], "fine")
    # 3. fed the kernels' decisions, the oracle matches every gradient at GRAD_RTOL
    fed = oracle_step(seen["saved"][0], seen["saved"][1], seen["z_fine"])[0]
    worst, worst_own = (0.0, ""), (0.0, "")
    for k in got:
        scale = fed[k].abs().max().item()
        e = (got[k].double() - fed[k].double()).abs().max().item() / max(scale, 1e-30)
        worst = max(worst, (e, k))
        e_own = (got[k].double() - own[k].double()).abs().max().item() / max(own[k].abs().max().item(), 1e-30)
        worst_own = max(worst_own, (e_own, k))
        explained_by_kinks(got[k], own[k], fed[k], k)
    n_samples = {"coarse": 4096 * 64, "fine": 4096 * 128}
    margin("c3_decisions[f32]", "kernels vs oracle on the kernels' decisions (worst: %s)" % worst[1], worst[0],
           GRAD_RTOL, fine_depths_differing=z_dis, fine_depths_differing_over_1em4=z_far,
           fine_depths=4096 * 128, relu_decisions_differing_coarse=n_dis_c,
           relu_decisions_differing_fine=n_dis_f, relu_decisions_coarse=4 * 256 * n_samples["coarse"],
           relu_decisions_fine=4 * 256 * n_samples["fine"])
    margin("c3_decisions[f32]", "kernels vs oracle on its own decisions (worst: %s)" % worst_own[1], worst_own[0],
           C3_GRAD_RTOL["f32"])


# ---------------------------------------------------------------- round 6: a render's two fields in shared launches


@pytest.mark.parametrize("rays,nc,nf", [(4096, 64, 128), (1024, 64, 192), (4096, 32, 160), (512, 64, 128)])
def test_field_backward_train_pair_bitwise(dev, rays, nc, nf):
    """cn_field_backward_train_multi with a coarse and a fine field (one dX launch, one batched dW launch,
    one layer_xyz1 launch, one reduction launch for both) against the two per-field calls: every weight,
    bias and g_code gradient bit for bit.  Shapes: C3's chunk, the 3080 config's 1024-ray chunk (64 + 192
    samples), cars-code's 32 + 160, and a chunk below the batched dW plan (M < 64 Ki: the fields then run
    one after the other inside the call)."""
    from codenerf import ops, synthetic
    fx, fd = [2.0 ** k for k in range(10)], [2.0 ** k for k in range(4)]
    g = torch.Generator().manual_seed(rays + nc + nf)
    ro = (torch.randn(rays, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 1.3])).to(dev)
    rd = torch.randn(rays, 3, generator=g).to(dev)
    zs, zt = synthetic.latent_codes(5, 1).to(dev), synthetic.latent_codes(6, 1).to(dev)
    fields = []
    for seed, s in ((0, nc), (1, nf)):
        m = model(dev, seed)
        params = [p.detach() for p in m.param_list()]
        z = torch.sort(0.8 + torch.rand(rays, s, generator=g), dim=-1).values.to(dev)
        gout = torch.randn(rays, s, 4, generator=g).to(dev)
        cb = ops.code_bias(params, zs, zt)
        _, saved, masks = ops.radiance_field_train_w16(ops.mlp_pack(params, "f32_w16"), cb, rd, s, rays, fx, fd, ro=ro,
                                                       z=z, precision="f32")
        fields.append(dict(packed_t=ops.mlp_pack(params, "f32_w16_t"), params=params, masks=masks, saved=saved,
                           x_enc=None, d_raw=gout, n_rays=rays, n_samples=s, chunk_rows=rays, n_codes=1, freqs_xyz=fx,
                           freqs_dir=fd, rd=rd, ro=ro, z=z))
    out = {}
    for mode in ("single", "pair", "pair2"):
        pgs = [[torch.zeros_like(p) for p in f["params"]] for f in fields]
        gcs = [torch.zeros(1, 520, device=dev) for _ in fields]
        jobs = [dict(f, param_grads=pg, g_code=gc) for f, pg, gc in zip(fields, pgs, gcs)]
        if mode == "single":
            for j in jobs:
                ops.field_backward_train_multi([j])
        else:
            ops.field_backward_train_multi(jobs[::-1])          # fine first, as the deferred pair runs them
        torch.cuda.synchronize()
        out[mode] = (pgs, gcs)
    for mode in ("pair", "pair2"):
        for f in range(2):
            for k, (a, b) in enumerate(zip(out[mode][0][f], out["single"][0][f])):
                assert torch.equal(a, b), (mode, f, k, (a - b).abs().max().item())
            assert torch.equal(out[mode][1][f], out["single"][1][f]), (mode, f, "g_code")


@pytest.mark.parametrize("name", ["train_cars_code", "train_3080"])
def test_train_minibatch_paired_fields_bitwise(dev, monkeypatch, name):
    """train_minibatch pairs the two fields' training backwards (autograd.FieldPair: the fine field's
    backward waits for the coarse one's, then ONE cn_field_backward_train_multi call runs both) -- the
    gradients, the code rows and the post-AdamW parameters bit for bit those of the unpaired step, on the
    reference's runnable chunk shapes (one object per chunk: train_cars_code.npz 4096 rays at 32 + 128,
    train_3080.npz 1024 rays at 64 + 128)."""
    from codenerf import autograd as A, ops, synthetic, train as T
    from codenerf.models import CodeNeRFModel, ShapeTextureEmbedding
    from codenerf.nerf import PointSampler
    from test_gpu_parity import load
    g = load(name + ".npz", dev)
    nc, nf, chunk = int(g["nc"].item()), int(g["nf"].item()), int(g["chunk"].item())
    torch.manual_seed(4343)
    t_rand, u = torch.rand(chunk, nc).to(dev), torch.rand(chunk, nf).to(dev)
    calls = []
    real = ops.field_backward_train_multi

    def spy(fields, precision="f32"):
        calls.append(len(fields))
        return real(fields, precision)
    monkeypatch.setattr(ops, "field_backward_train_multi", spy)
    res = {}
    for paired in (True, False):
        if not paired:
            monkeypatch.setattr(A, "new_field_pair", lambda: None)
        calls.clear()
        emb_t = ShapeTextureEmbedding(C3_OBJECTS, 256, 256)
        with torch.no_grad():
            emb_t.shape_embedding.weight.copy_(synthetic.latent_codes(40, C3_OBJECTS))
            emb_t.texture_embedding.weight.copy_(synthetic.latent_codes(41, C3_OBJECTS))
        models = {"embedding": emb_t.to(dev)}
        for key, seed in (("nerf_coarse", 0), ("nerf_fine", 1)):
            m = CodeNeRFModel(hidden_size=256, shape_code_size=256, texture_code_size=256, num_encoding_fn_xyz=10,
                              num_encoding_fn_dir=4)
            m.load_state_dict(synthetic.codenerf_params(seed))
            models[key] = m.to(dev)
        opt, sched = T.prepare_optimizer(_opt_cfg(), models)
        ps = PointSampler(nc, nf, 0.8, 1.8, spacing_mode="lindepth", perturb=True, dtype=torch.float32, device=dev)
        ids = g["ids"].long()
        ids._cn_host_ids = g["ids"].long().cpu().numpy()
        logs = T.train_minibatch(models, opt, sched, ps, embedders(dev), g["ro"], g["rd"], ids, g["target"], 1e-5,
                                 uniforms=(t_rand, u))
        torch.cuda.synchronize()
        # every gradient is its flat slot (no clone by AccumulateGrad, no copy back by the optimiser)
        flat = opt.flat_buffers()["grad"]
        lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * flat.numel()
        for k, mm in models.items():
            for n, p in mm.named_parameters():
                assert lo <= p.grad.data_ptr() < hi, f"{k}.{n}: .grad is not its flat slot"
        res[paired] = ({f"{k}.{n}": (p.grad.detach().clone(), p.detach().clone()) for k, mm in models.items()
                        for n, p in mm.named_parameters()}, float(logs["total_loss"]), list(calls))
    assert res[True][2] == [2], res[True][2]              # one shared call for both fields
    assert res[False][2] == [1, 1], res[False][2]
    assert res[True][1] == res[False][1]
    for k, (gr, pv) in res[True][0].items():
        g2, p2 = res[False][0][k]
        assert torch.equal(gr, g2), (k, (gr - g2).abs().max().item())
        assert torch.equal(pv, p2), k
