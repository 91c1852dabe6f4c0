"""The fp16 inference field kernel (CN_FMT_F16, csrc/mlp_f16.hip) on the device.

Bitwise: on the integer probes of tests/exact_cases.py the device returns the float64 rule of
tests/field_f16_cases.py bit for bit (tests/test_field_f16_cpu.py proves the rule has one right answer there and
that the probes pin round-to-nearest-even).  Random weights: the device stays within a recorded margin of the
rule -- 2x the largest error seen on the MI355X (profiles/f16/parity_margins.json), the project's convention
for 3xbf16 -- and that margin is capped by the rule's own distance from the unrounded float64 model on the same
inputs (mean: a quarter of it, max: all of it): the only slack the rule leaves is the fp32 summation order and
the rare activation that order pushes across an fp16 rounding boundary, so a kernel that rounds anything the
rule keeps in fp32 misses the caps.  Then non-finite rows, stores past m, a side stream, graph replay and the
renders that run on models of precision "f16"."""
import json
import os

import numpy as np
import pytest
import torch

import buffers as B
import exact_cases as E
import field_f16_cases as H
import occupancy_cases as OC
import streams as S
from conftest import ROOT
from test_gpu_field_exact import FD, FX, code_bias, geo_inputs, ident, on_dev, packed, same
from test_gpu_parity import dev, embedders, load, models  # noqa: F401

pytestmark = pytest.mark.gpu

MARGINS = os.path.join(ROOT, "profiles", "f16", "parity_margins.json")


def margins():
    with open(MARGINS) as f:
        return json.load(f)


def device_raw(dev, case):
    from codenerf import ops
    d = on_dev(dev, case)
    pk, cb = packed(dev, case, "f16"), code_bias(dev, case)
    if case["mode"] == "enc":
        return ops.mlp_forward(pk, cb, d["x"], d["code_index"], precision="f16")
    raw = ops.radiance_field(pk, cb, d["rd"], case["s"], case["chunk"], FX, FD, code_index=d["code_index"],
                             precision="f16", **geo_inputs(case, d))
    return raw.reshape(-1, 4)


# ---------------------------------------------------------------- 3. bitwise on the probes


@pytest.mark.parametrize("case", H.probe_cases(), ids=ident)
def test_probe_is_the_rule_bit_for_bit(dev, case):
    """Encoded rows at m in {1, 31, 32, 33, 127, 128, 129, 255, 256, 257} with the three code layouts, the model
    set, one dense model per layer, and geometry from points and from rays + depths with chunk_rows."""
    same(code_bias(dev, case), E.reference(case)["code_bias"], "code_bias")
    same(device_raw(dev, case), H.rule(case), "raw")


def test_second_tile_of_every_workgroup(dev):
    """One row past exact_cases.persistent_rows: every persistent workgroup loops to a second 128-sample tile."""
    case = H.second_tile_case(torch.cuda.get_device_properties(dev).multi_processor_count)
    H.check(case)
    same(device_raw(dev, case), H.rule(case), "raw")


# ---------------------------------------------------------------- 4. random weights


def _weights(name):
    from codenerf import synthetic
    return {"synthetic1": lambda: synthetic.codenerf_params(1), "t4": lambda: synthetic.trained_params(1, "t4"),
            "t3": lambda: synthetic.trained_params(2, "t3")}[name]()


_RANDOM = {}


def random_case(dev, name, layout):
    """Device raw, the rule and the unrounded model on 4096 random points and directions -> (|device - rule|,
    |rule - unrounded|), each (4096, 4) float64; computed once."""
    from codenerf import ops
    key = (name, layout)
    if key not in _RANDOM:
        params = _weights(name)
        pts, rd, zs, zt, ci = H.random_inputs(seed={"synthetic1": 11, "t4": 12, "t3": 13}[name])
        if layout == "one":
            zs, zt, ci = zs[:1], zt[:1], None
        plist = [t.to(dev) for t in E.params_list(params)]
        cb = ops.code_bias(plist, zs.to(dev), zt.to(dev))
        m = pts.shape[0]
        raw = ops.radiance_field(ops.mlp_pack(plist, "f16"), cb, rd.to(dev), 1, m, FX, FD, pts=pts.to(dev),
                                 code_index=None if ci is None else ci.to(dev), precision="f16").reshape(m, 4)
        x = H.encode(pts, rd)
        code = ci if ci is not None else torch.zeros(m, dtype=torch.long)
        rule = H.forward(params, x, cb.cpu(), code)
        exact = H.unrounded(params, x, cb.cpu(), code)
        _RANDOM[key] = ((raw.cpu().double() - rule).abs(), (rule - exact).abs())
    return _RANDOM[key]


@pytest.mark.parametrize("layout", ["one", "index"])
@pytest.mark.parametrize("name", ["synthetic1", "t4", "t3"])
def test_random_weights_within_the_recorded_margin(dev, name, layout):
    err, dist = random_case(dev, name, layout)
    assert bool(torch.isfinite(err).all())
    figures = dict(max=float(err.max()), mean=float(err.mean()))
    caps = dict(max=float(dist.max()), mean=float(dist.mean()) / 4)
    print("F16_MARGIN " + json.dumps({"key": f"{name}/{layout}", "err": figures, "caps": caps}))
    bound = margins()["field"][f"{name}/{layout}"]
    for k in ("max", "mean"):
        assert bound[k] <= caps[k], f"{k}: the recorded margin {bound[k]:.3g} exceeds its cap {caps[k]:.3g}"
        assert figures[k] <= bound[k], f"{k}: |device - rule| {figures[k]:.3g} over the margin {bound[k]:.3g}"


# ---------------------------------------------------------------- 5. edges


EDGES = [("dense:layer_dir2", ((66, -1e5),), False),      # -inf through layer_dir1: rgb NaN, sigma finite
         ("dense:layer_xyz1", ((5, 1e5), (40, -1e5)), True)]   # inf x 0 = NaN in layer_xyz2, ReLU takes NaN to 0


@pytest.mark.parametrize("model,edits,finite", EDGES, ids=[e[0] for e in EDGES])
def test_non_finite_row_and_no_store_past_m(dev, model, edits, finite):
    """|x| = 1e5 in one encoded row of a dense model rounds to inf: the row's outputs are non-finite exactly
    where the rule's are (and have its bits where they are finite), its neighbours keep the rule's bits, and
    nothing is stored past row m (m = 33: 95 idle lanes of the tile would land in the guard)."""
    from codenerf import ops
    case = E.encoded_case(model, 33, "one")
    ref = E.reference(case)
    x = ref["x"].clone()
    for col, v in edits:
        x[7, col] = v
    want = H.forward(case["params"], x, ref["code_bias"], ref["code"])
    assert bool(torch.isfinite(want[7]).all()) == finite and bool(torch.isfinite(want[7]).any())
    pk, cb = packed(dev, case, "f16"), code_bias(dev, case)
    with B.contracts("poison") as arena:
        raw = ops.mlp_forward(pk, cb, x.float().to(dev), None, precision="f16")
        assert arena.n_allocations >= 1
    raw = raw.cpu()
    ok = torch.isfinite(want[7])
    assert torch.equal(torch.isfinite(raw[7]), ok)
    assert torch.equal(raw[7][ok], want[7][ok].float())
    keep = torch.ones(33, dtype=torch.bool)
    keep[7] = False
    same(raw[keep], want[keep], "the other rows")


# ---------------------------------------------------------------- 6. stream and graph


def _field_call(dev, case, d):
    from codenerf import ops
    return lambda: ops.radiance_field(packed(dev, case, "f16"), code_bias(dev, case), d["rd"], case["s"],
                                      case["chunk"], FX, FD, code_index=d["code_index"], precision="f16",
                                      **geo_inputs(case, d))


def test_side_stream(dev):
    """The call's work is on the current stream: issued on a side stream while the default stream spins, its
    output is complete before the spin ends, with the default-stream run's bits."""
    case = E.geometry_case(2, "rayz", 37, 8, 10, "index")
    call = _field_call(dev, case, on_dev(dev, case))
    call()
    with S.plain() as base:
        call()
    with S.side_stream(wall_ms=base.wall_ms) as side:
        call()
    assert side.slack_ms and min(side.slack_ms) > 0
    assert [r[0] for r in base.returns] == [r[0] for r in side.returns]
    S.compare_logs(base.returns, side.returns, "the side-stream run")


def test_graph_replay_on_new_inputs(dev):
    """One kernel, captured alone and replayed after its inputs changed in place: the eager call's bits."""
    from codenerf import ops
    case, other = E.geometry_case(2, "rayz", 37, 8, 10, "one"), E.geometry_case(3, "rayz", 37, 8, 10, "one")
    d = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in on_dev(dev, case).items()}
    pk, cb = packed(dev, case, "f16"), code_bias(dev, case)

    def call():
        return ops.radiance_field(pk, cb, d["rd"], 8, 10, FX, FD, precision="f16", ro=d["ro"], z=d["z"])
    eager = call().clone()
    graph, out = S.capture(call)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    same(out.reshape(-1, 4), H.rule(case), "raw")
    o = on_dev(dev, other)
    for k in ("ro", "rd", "z"):
        d[k].copy_(o[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    assert torch.equal(replayed, call())
    assert not torch.equal(replayed, eager)


# ---------------------------------------------------------------- 7. renders


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def scene(dev):
    """8 x 8 rays of the render_small.npz pose, synthetic coarse and fine models at "f16" and at "f32"."""
    from codenerf.nerf import OccupancyGrid, PointSampler, RaySampler
    g = load("render_small.npz", dev)
    k = torch.tensor([[7.0, 0, 4.0, 0], [0, 7.0, 4.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    rs = RaySampler(8, 8, k, sample_size=64, device=dev, datatype=torch.float32)
    ro, rd = (t.reshape(-1, 3) for t in rs.get_bundle(g["pose"]))
    n = ro.shape[0]
    mc, mf = models(dev, precision="f16")
    rc, rf = models(dev, precision="f32")
    bits = OC.grid_bits("sphere", 32, bound=1.0, radius=0.45)
    return dict(g=g, ro=ro, rd=rd, n=n, mc=mc, mf=mf, rc=rc, rf=rf, zs=g["z_s"].expand(n, -1),
                zt=g["z_t"].expand(n, -1), emb=embedders(dev), bits=bits,
                grid=OccupancyGrid(T(np.asarray(bits).view(np.int32), dev), 32, 1.0),
                ps=PointSampler(16, 16, 0.8, 1.8, "lindepth", False, torch.float32, dev))


def _composed(sc, dev, keep_of=None):
    """render_rays' entries from ops.radiance_field(precision="f16") and the existing samplers and volume_render
    (``keep_of``: depths -> the kept mask of an occupancy grid; a culled sample is the empty row)."""
    from codenerf import ops
    ro, rd, ps, g = sc["ro"], sc["rd"], sc["ps"], sc["g"]
    empty = torch.tensor([0.0, 0.0, 0.0, -1.0e4], device=dev)

    def field(model, z):
        raw = ops.radiance_field(model.packed("f16"), model.code_bias(g["z_s"], g["z_t"]), rd, z.shape[1], sc["n"],
                                 FX, FD, ro=ro, z=z, precision="f16")
        return raw if keep_of is None else torch.where(keep_of(z)[..., None], raw, empty)
    _, z_c = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
    rgb_c, disp_c, acc_c, w_c, depth_c = ops.volume_render(field(sc["mc"], z_c), z_c, rd)
    _, z_f = ops.sample_pdf(ro, rd, w_c[..., 1:-1], z_c, ps.num_samples_fine, ps.u_lin, want_pts=False)
    rgb_f, disp_f, acc_f, _, depth_f = ops.volume_render(field(sc["mf"], z_f), z_f, rd)
    return {"rgb_coarse": rgb_c, "disp_coarse": disp_c, "acc_coarse": acc_c, "weights_coarse": w_c,
            "depth_coarse": depth_c, "z_coarse": z_c, "rgb_fine": rgb_f, "disp_fine": disp_f, "acc_fine": acc_f,
            "depth_fine": depth_f, "z_fine": z_f}


def _same_dict(out, want):
    assert sorted(out) == sorted(want)
    for k in want:
        a, b = out[k], want[k]
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), k


def _render(sc, mc, mf, **kw):
    from codenerf.nerf import render_rays
    with torch.no_grad():
        return render_rays(sc["ro"], sc["rd"], sc["zs"], sc["zt"], sc["ps"], sc["emb"], mc, mf, **kw)


def test_render_rays_is_the_composition(dev, scene):
    sc = scene
    assert sc["mc"].inference_format() == sc["mc"].kernel_format() == "f16"
    with torch.no_grad():
        want = _composed(sc, dev)
    _same_dict(_render(sc, sc["mc"], sc["mf"]), want)


def test_render_rays_with_occupancy_keeps_the_unculled_bits(dev, scene):
    sc = scene

    def keep_of(z):
        pts = OC.ray_points(sc["ro"].cpu().numpy(), sc["rd"].cpu().numpy(), z.cpu().numpy())
        return T(OC.lookup(pts, sc["bits"], 32, 1.0), dev)
    with torch.no_grad():
        want = _composed(sc, dev, keep_of)
    out = _render(sc, sc["mc"], sc["mf"], occupancy=sc["grid"])
    _same_dict(out, want)
    assert float(out["acc_fine"].max()) > 0


def test_render_with_span_probes_runs(dev, scene):
    sc = scene
    from codenerf.nerf import PointSampler
    ps = PointSampler(16, 16, 0.8, 1.8, "lindisp", False, torch.float32, dev)
    out = _render(dict(sc, ps=ps), sc["mc"], sc["mf"], occupancy=sc["grid"], span_probes=64)
    assert bool(torch.isfinite(out["rgb_fine"]).all()) and "ray_span" in out


def test_parallel_image_render_is_render_rays(dev, scene):
    """An 8 x 8 image of the "f16" models, with and without a grid: render_rays' rgb_fine in chunks of 40 rays."""
    from types import SimpleNamespace as NS
    from codenerf.nerf import RaySampler, parallel_image_render
    sc = scene
    k = torch.tensor([[7.0, 0, 4.0, 0], [0, 7.0, 4.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    rs = RaySampler(8, 8, k, sample_size=64, device=dev, datatype=torch.float32)
    cfg = NS(is_distributed=False, gpus=1, nerf=NS(validation=NS(chunksize=40)))
    mdls = {"nerf_coarse": sc["mc"], "nerf_fine": sc["mf"]}
    args = (cfg, sc["g"]["pose"], [sc["g"]["z_s"], sc["g"]["z_t"]], mdls, (rs, sc["ps"]), sc["emb"], dev)
    for kw in ({}, dict(occupancy=sc["grid"])):
        img = parallel_image_render(*args, **kw)
        assert torch.equal(img, _render(sc, sc["mc"], sc["mf"], chunk_rows=40, **kw)["rgb_fine"])


def test_render_scene_with_two_objects(dev, scene):
    from codenerf import synthetic
    from codenerf.nerf import SceneObject, render_scene
    sc = scene
    zs2, zt2 = synthetic.latent_codes(11, 1).to(dev), synthetic.latent_codes(12, 1).to(dev)
    objects = [SceneObject(sc["g"]["z_s"], sc["g"]["z_t"], sc["grid"]),
               SceneObject(zs2, zt2, sc["grid"], translation=(0.2, 0.0, 0.1))]
    with torch.no_grad():
        out = render_scene(sc["ro"], sc["rd"], objects, sc["ps"], sc["emb"], sc["mc"], sc["mf"])
    assert out["rgb_fine"].shape == (sc["n"], 3) and bool(torch.isfinite(out["rgb_fine"]).all())
    assert out["acc_objects_fine"].shape == (2, sc["n"])


def test_render_is_close_to_the_fp32_render(dev, scene):
    """|rgb_fine - the fp32 render's| within the recorded margin (2x the MI355X's figure), itself at most 1/255."""
    sc = scene
    diff = (_render(sc, sc["mc"], sc["mf"])["rgb_fine"] - _render(sc, sc["rc"], sc["rf"])["rgb_fine"]).abs()
    figure = float(diff.max())
    print("F16_MARGIN " + json.dumps({"key": "render/rgb_fine", "err": {"max": figure, "mean": float(diff.mean())}}))
    bound = margins()["render"]["rgb_fine"]["max"]
    assert bound <= 1.0 / 255.0
    assert figure <= bound


def test_refusals(dev, scene):
    """What every precision but "f32" is refused, with the existing errors; gradients: NotImplementedError."""
    from codenerf import nerf
    sc = scene
    refused = (ValueError, NotImplementedError)
    for kw in (dict(occupancy=sc["grid"], sync_free=True), dict(coarse_rgb=False), dict(rgb_tolerance=0.01),
               dict(normals=True)):
        with pytest.raises(refused):
            _render(sc, sc["mc"], sc["mf"], **kw)
    pts = torch.zeros(4, 3, device=dev)
    with torch.no_grad():
        with pytest.raises(refused):
            nerf.density(sc["mf"], sc["emb"], pts, sc["g"]["z_s"])
        with pytest.raises(refused):
            nerf.density_grid(sc["mf"], sc["emb"], sc["g"]["z_s"], 8, 1.0)
        with pytest.raises(refused):
            nerf.extract_mesh(sc["mf"], sc["emb"], sc["g"]["z_s"], 8, 1.0, 10.0)
    objects = [nerf.SceneObject(sc["g"]["z_s"], sc["g"]["z_t"], sc["grid"])]
    for m in (sc["mc"], sc["mf"]):
        m.requires_grad_(False)
    try:
        with pytest.raises(refused):
            nerf.render_scene_autograd(sc["ro"], sc["rd"], objects, sc["ps"], sc["emb"], sc["mc"], sc["mf"])
        zs = sc["zs"].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError):
            nerf.render_rays(sc["ro"], sc["rd"], zs, sc["zt"], sc["ps"], sc["emb"], sc["mc"], sc["mf"])
        x = torch.zeros(4, 90, device=dev)
        with pytest.raises(NotImplementedError):
            sc["mf"](zs[:4], sc["zt"][:4], x)
    finally:
        for m in (sc["mc"], sc["mf"]):
            m.requires_grad_(True)
