"""The launch sequence and the result keys of the three hierarchical renders, configuration by configuration.

render_rays, render_scene and render_scene_autograd are host-side orchestration: what they launch, in which
order, is their whole behaviour beyond the kernels' own.  Every library launch in ``codenerf.ops`` goes through
``check(rc, "cn_...")``; a recorder in its place logs the entry names of one render, and the log must equal the
list committed in golden/render_launch_sequences.json, which the same recorder produced from the package of the
commit named in that file's header (``python tests/test_gpu_render_launches.py --write PACKAGE COMMIT PATH`` with that
commit's package importable as PACKAGE -- never from the tree under test).  Each configuration is rendered once
unrecorded first, so that the weight packs it needs are cached and its log does not depend on which
configurations ran before it.  The result dict's key order is asserted beside it.

37 rays (no multiple of 16), chunk_rows 16, 8 + 8 samples between 0.8 and 1.8, the synthetic models and codes,
OccupancyGrids at resolution 32: a sphere that keeps part of the samples and an all-zero grid that keeps none --
with no kept row a synchronising culled call launches no field, a sync-free one launches it at capacity."""
import contextlib
import importlib
import json
import math
import os
import sys

import pytest
import torch

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_launch_sequences.json")
N_RAYS, CHUNK_ROWS = 37, 16


def make_scene(dev, package="codenerf"):
    """The shared, read-only inputs, built from ``package``'s classes."""
    nerf, synthetic = importlib.import_module(package + ".nerf"), importlib.import_module(package + ".synthetic")
    model_cls = importlib.import_module(package + ".models").CodeNeRFModel
    gen = torch.Generator().manual_seed(37)
    xy = torch.rand(N_RAYS, 2, generator=gen) * 0.7 - 0.35
    ms = []
    for seed in (0, 1):
        m = model_cls(256, 1, 256, 256, 10, 4)
        m.load_state_dict(synthetic.codenerf_params(seed))
        ms.append(m.to(dev).eval().requires_grad_(False))
    g = 32
    c = (torch.arange(g, dtype=torch.float64) + 0.5) * (2.0 / g) - 1.0
    inside = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) <= 0.45 ** 2
    words = (inside.reshape(-1, 32).long() << torch.arange(32)).sum(dim=1)        # bit c & 31 of word c >> 5
    sphere = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    sampler = {(mode, perturb): nerf.PointSampler(8, 8, 0.8, 1.8, mode, perturb, torch.float32, dev)
               for mode, perturb in (("lindepth", False), ("lindisp", False), ("lindepth", True))}
    a = 0.5
    return dict(
        nerf=nerf, ro=torch.tensor([0.1, -0.2, 1.3]).repeat(N_RAYS, 1).to(dev),
        rd=torch.cat([xy, -torch.ones(N_RAYS, 1)], dim=1).to(dev), mc=ms[0], mf=ms[1], sampler=sampler,
        codes=[synthetic.latent_codes(s, 1).to(dev) for s in (5, 6, 11, 12)],
        emb=(nerf.PositionalEmbedder(10, True, True, torch.float32, dev),
             nerf.PositionalEmbedder(4, True, True, torch.float32, dev)),
        grids={"sphere": nerf.OccupancyGrid(sphere.to(dev), g, 1.0),
               "empty": nerf.OccupancyGrid(torch.zeros(g * g * g // 32, dtype=torch.int32, device=dev), g, 1.0)},
        rotation=[[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]],
        translation=[0.1, 0.0, -0.1], t_rand=torch.rand(N_RAYS, 8, generator=gen).to(dev),
        u=torch.rand(N_RAYS, 8, generator=gen).to(dev))


def rays_case(sampler=("lindepth", False), grid=None, grad=False, inject=False, **kw):
    """A render_rays configuration -> a callable scene -> (result dict, gradients or None)."""
    def run(sc):
        zs, zt = (c.clone().requires_grad_(grad) for c in sc["codes"][:2])
        draws = dict(t_rand=sc["t_rand"], u=sc["u"]) if inject else {}
        with torch.set_grad_enabled(grad):
            out = sc["nerf"].render_rays(sc["ro"], sc["rd"], zs.expand(N_RAYS, -1), zt.expand(N_RAYS, -1),
                                         sc["sampler"][sampler], sc["emb"], sc["mc"], sc["mf"], chunk_rows=CHUNK_ROWS,
                                         occupancy=None if grid is None else sc["grids"][grid], **draws, **kw)
        if not grad:
            return out, None
        (out["rgb_coarse"].sum() + (out["rgb_fine"] * out["depth_fine"][:, None]).sum()).backward()
        return out, [zs.grad, zt.grad]
    return run


def scene_objects(sc, codes, scale):
    obj = sc["nerf"].SceneObject
    return [obj(codes[0], codes[1], sc["grids"]["sphere"]),
            obj(codes[2], codes[3], sc["grids"]["sphere"], rotation=sc["rotation"], translation=sc["translation"],
                **({} if scale == 1.0 else dict(scale=scale)))]


def scene_case(sampler=("lindepth", False), scale=0.5, **kw):
    def run(sc):
        with torch.no_grad():
            return sc["nerf"].render_scene(sc["ro"], sc["rd"], scene_objects(sc, sc["codes"], scale),
                                           sc["sampler"][sampler], sc["emb"], sc["mc"], sc["mf"], **kw), None
    return run


def scene_grad_case(sc, sampler=("lindepth", False)):
    codes = [c.clone().requires_grad_(True) for c in sc["codes"]]
    identity = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    posed = [v for row in sc["rotation"] for v in row] + sc["translation"] + [0.5]
    poses = torch.tensor([identity, posed], device=sc["ro"].device).requires_grad_(True)
    out = sc["nerf"].render_scene_autograd(sc["ro"], sc["rd"], scene_objects(sc, codes, 1.0),
                                           sc["sampler"][sampler], sc["emb"], sc["mc"], sc["mf"], poses=poses)
    (out["rgb_coarse"].sum() + (out["rgb_fine"] * out["depth_fine"][:, None]).sum()
     + out["acc_objects_fine"][1].sum()).backward()
    return out, [poses.grad] + [c.grad for c in codes]


# name -> (the render, what its key order depends on)
CASES = {
    "rays": (rays_case(), {}),
    "rays-coarse_only": (rays_case(coarse_only=True), dict(coarse_only=True)),
    "rays-density_coarse": (rays_case(coarse_rgb=False), dict(coarse_rgb=False)),
    "rays-occupancy-sphere": (rays_case(grid="sphere"), {}),
    "rays-occupancy-empty": (rays_case(grid="empty"), {}),
    "rays-occupancy-sync_free-sphere": (rays_case(grid="sphere", sync_free=True), {}),
    "rays-occupancy-sync_free-empty": (rays_case(grid="empty", sync_free=True), {}),
    "rays-tolerance": (rays_case(rgb_tolerance=1e-3), {}),
    "rays-tolerance-occupancy-sync_free": (rays_case(grid="sphere", rgb_tolerance=1e-3, sync_free=True), {}),
    "rays-normals": (rays_case(normals=True), dict(normals=True)),
    "rays-span": (rays_case(("lindisp", False), grid="sphere", span_probes=64), dict(span=True)),
    "rays-perturb-injected": (rays_case(("lindepth", True), inject=True), {}),
    "rays-grad": (rays_case(grad=True), {}),
    "scene": (scene_case(), dict(objects=True)),
    "scene-unit_scales": (scene_case(scale=1.0), dict(objects=True)),
    "scene-coarse_only": (scene_case(coarse_only=True), dict(objects=True, coarse_only=True)),
    "scene-density_coarse": (scene_case(coarse_rgb=False), dict(objects=True, coarse_rgb=False)),
    "scene-span": (scene_case(("lindisp", False), span_probes=64), dict(objects=True, span=True)),
    "scene-sync_free": (scene_case(sync_free=True), dict(objects=True)),
    "scene-grad": (scene_grad_case, dict(objects=True)),
}


def expected_keys(coarse_rgb=True, coarse_only=False, objects=False, span=False, normals=False):
    """The result dict's keys in insertion order."""
    keys = ["rgb_coarse"] * coarse_rgb + ["disp_coarse", "acc_coarse", "weights_coarse", "depth_coarse", "z_coarse"]
    keys += ["acc_objects_coarse"] * objects + ["ray_span", "ray_hit"] * span
    if not coarse_only:
        keys += ["rgb_fine", "disp_fine", "acc_fine", "depth_fine", "z_fine"]
        keys += ["acc_objects_fine"] * objects + ["normal_fine"] * normals
    return keys


@contextlib.contextmanager
def recorded_launches(package="codenerf"):
    """The entry names ``package``.ops hands to ``check``, in call order, while the context is active."""
    ops = importlib.import_module(package + ".ops")
    real, seen = ops.check, []

    def check(rc, what):
        seen.append(what)
        return real(rc, what)
    ops.check = check
    try:
        yield seen
    finally:
        ops.check = real


def record(sc, name, package="codenerf"):
    """One warm render, then the recorded one -> (launches, result keys)."""
    run = CASES[name][0]
    run(sc)
    with recorded_launches(package) as seen:
        out, _ = run(sc)
        torch.cuda.synchronize()
    return list(seen), list(out)


@pytest.fixture(scope="module")
def scene():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import codenerf
    codenerf.load_library()
    return make_scene(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_render_launch_sequence_and_key_order(scene, golden, name):
    launches, keys = record(scene, name)
    assert keys == expected_keys(**CASES[name][1])
    assert launches and all(what.startswith("cn_") for what in launches)
    assert launches == golden["sequences"][name]


def test_golden_covers_every_case(golden):
    assert sorted(golden["sequences"]) == sorted(CASES) and golden["header"]["commit"]


if __name__ == "__main__":        # --write PACKAGE COMMIT PATH: the golden file, from another commit's package
    _, flag, package, commit, path = sys.argv
    assert flag == "--write" and package != "codenerf", "the golden file comes from the parent commit's package"
    importlib.import_module(package).load_library()
    sc = make_scene(torch.device("cuda", 0), package)
    doc = {"header": {"commit": commit, "what": "entry names passed to ops.check during one warm render per case, "
                      "recorded by tests/test_gpu_render_launches.py on that commit's package"},
           "sequences": {name: record(sc, name, package)[0] for name in sorted(CASES)}}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
