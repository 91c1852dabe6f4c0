"""Measure what uniform scale costs the scene render: the scaled composition launch against the unscaled one,
and render_scene of four copies.  Needs an MI355X: there is no CPU fallback.

    python tools/bench_scene_scale.py [--step compose|render|all] [--reps 30] [--out PATH]
                                      [--parent-lib PATH] [--package-root DIR]

Each step merges its section into the JSON at --out (default profiles/scenescale/bench_scene_scale.json).  All
times are device events around one call; the variants of a step alternate inside one process after a warm-up of
all of them, and every figure carries its spread (min / median / max over the repetitions), as
tools/bench_scene.py.

``compose``: 16,384 rays, S = 64 and 192, K = 1, 4, 8 objects of random raw rows (about half of each object's
slots empty, as after a cull): cn_volume_render_compose_scaled with scales drawn from {0.5, 1, 2, 0.37, 3.1}
and with every scale 1, beside cn_volume_render_compose on the same tensors -- this library's, and with
--parent-lib also the entry of another build of the library (the parent commit's), loaded beside this one and
called on the same tensors in the same alternation.
``render``: one 128 x 128 view, 64 + 64 samples, unperturbed; render_scene of four copies of one synthetic
object translated along a line (sphere grids of radius 0.4, G = 128) with scales (1, 1, 1, 1) -- the rigid path --
and, where the package has it, with scales (0.5, 1, 2, 0.37) -- the scaled entries.  --package-root runs this
step on another checkout's package (the parent commit's, with its own built library): the two processes'
"unit" figures are the comparison across commits.
The models are the synthetic ones: no trained checkpoint ships with the repository, so what trained objects
look like in a scene is not measured here.
"""
import argparse
import ctypes
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-nerf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_density import alternate, setup, spread, view_rays  # noqa: E402
from bench_occupancy import sphere_grid  # noqa: E402
from bench_scene import EMPTY_ROW, RAYS, compose_bytes  # noqa: E402

SCALES = (0.5, 1.0, 2.0, 0.37, 3.1)


def beyond_spread(a, b):
    return a["max_ms"] < b["min_ms"] or a["min_ms"] > b["max_ms"]


def parent_compose(path):
    """cn_volume_render_compose of the library at ``path`` -> a callable on this process's tensors, writing into
    outputs it allocates once per shape."""
    from codenerf import _lib
    lib = ctypes.CDLL(path)
    fn = lib.cn_volume_render_compose
    fn.restype, fn.argtypes = _lib.SIGNATURES["cn_volume_render_compose"]
    outs = {}

    def call(raws, z, rd):
        n, s = z.shape
        key = (n, s, len(raws))
        if key not in outs:
            outs[key] = [torch.empty(n, 3, device=z.device), torch.empty(n, device=z.device),
                         torch.empty(n, device=z.device), torch.empty(n, s, device=z.device),
                         torch.empty(n, device=z.device), torch.empty(len(raws), n, device=z.device)]
        pointers, keep = _lib.pointer_array(raws)
        rc = fn(pointers, len(raws), z.data_ptr(), rd.data_ptr(), n, s, *(t.data_ptr() for t in outs[key]),
                torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return outs[key]

    return call


def step_compose(dev, reps, parent_lib):
    from codenerf import ops
    parent = parent_compose(parent_lib) if parent_lib else None
    res = {"shape": {"rays": RAYS}, "parent_library": bool(parent), "launches": {}}
    for s in (64, 192):
        g = torch.Generator().manual_seed(s)
        z = torch.sort(1 + torch.rand(RAYS, s, generator=g), -1).values.to(dev)
        rd = torch.randn(RAYS, 3, generator=g).to(dev)
        raws = []
        for _ in range(8):
            raw = torch.randn(RAYS, s, 4, generator=g) * 2
            raw[torch.rand(RAYS, s, generator=g) < 0.5] = torch.tensor(EMPTY_ROW)
            raws.append(raw.to(dev))
        for k in (1, 4, 8):
            scales = [SCALES[(3 * j + 1) % len(SCALES)] for j in range(k)]
            if all(v == 1.0 for v in scales):
                scales[0] = 0.37
            out = {}
            fns = {"unscaled": lambda k=k: out.__setitem__("unscaled", ops.volume_render_compose(raws[:k], z, rd)),
                   "scaled_unit": lambda k=k: out.__setitem__("unit", ops.volume_render_compose(raws[:k], z, rd,
                                                                                               scales=[1.0] * k)),
                   "scaled": lambda k=k, scales=scales: out.__setitem__("scaled", ops.volume_render_compose(
                       raws[:k], z, rd, scales=scales))}
            if parent:
                fns["parent"] = lambda k=k: out.__setitem__("parent", parent(raws[:k], z, rd))
            ms = alternate(fns, reps)
            same = lambda a, b: all(torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)) for x, y in zip(a, b))  # noqa: E731
            assert same(out["unit"], out["unscaled"]), "unit scales differ from the unscaled entry"
            if parent:
                assert same(out["parent"], out["unscaled"]), "the unscaled entry differs from the parent library's"
            nbytes = compose_bytes(RAYS, s, k)
            sec = {name: dict(spread(v), gb_per_s=nbytes / (spread(v)["median_ms"] * 1e-3) / 1e9) for name, v in ms.items()}
            ref = "parent" if parent else "unscaled"
            sec.update(objects=k, bytes=nbytes, scales=scales, reference=ref,
                       scaled_over_reference_median=sec["scaled"]["median_ms"] / sec[ref]["median_ms"],
                       scaled_unit_over_reference_median=sec["scaled_unit"]["median_ms"] / sec[ref]["median_ms"],
                       unscaled_over_reference_median=sec["unscaled"]["median_ms"] / sec[ref]["median_ms"],
                       scaled_beyond_spread=beyond_spread(sec["scaled"], sec[ref]))
            res["launches"][f"s{s}_k{k}"] = sec
    return res


def step_render(dev, reps):
    from codenerf.nerf import PointSampler, SceneObject, render_scene
    (mc, mf), emb, zs, zt = setup(dev)
    ro, rd = view_rays(dev, 1.3)
    n = ro.shape[0]
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    grid = sphere_grid(dev, 1.0, 0.4)
    shifts = [[0.0, 0.0, 0.35 * (j - 1.5)] for j in range(4)]
    has_scale = "scale" in inspect.signature(SceneObject.__init__).parameters
    out = {}

    def scene(name, objects):
        def run():
            with torch.no_grad():
                out[name] = render_scene(ro, rd, objects, ps, emb, mc, mf)
        return run

    fns = {"unit": scene("unit", [SceneObject(zs, zt, grid, translation=t) for t in shifts])}
    if has_scale:
        fns["unit_explicit"] = scene("unit_explicit", [SceneObject(zs, zt, grid, translation=t, scale=1.0) for t in shifts])
        fns["scaled"] = scene("scaled", [SceneObject(zs, zt, grid, translation=t, scale=s)
                                         for t, s in zip(shifts, (0.5, 1.0, 2.0, 0.37))])
    ms = alternate(fns, reps)
    res = {"shape": {"rays": n, "coarse": 64, "fine_pass_samples": 128, "objects": 4, "translations": shifts},
           "package_has_scale": has_scale}
    for name, v in ms.items():
        res[name] = dict(spread(v), rays_per_s=n / (spread(v)["median_ms"] * 1e-3),
                         covered_fraction=float((out[name]["acc_fine"] > 0).float().mean()))
    if has_scale:
        assert all(torch.equal(torch.nan_to_num(out["unit"][key]), torch.nan_to_num(v))
                   for key, v in out["unit_explicit"].items())
        res["scaled_over_unit_median"] = res["scaled"]["median_ms"] / res["unit"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("compose", "render", "all"))
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each variant (>= 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenescale", "bench_scene_scale.json"))
    ap.add_argument("--parent-lib", default=None, help="compose: another build of the library to time beside this one")
    ap.add_argument("--package-root", default=None, help="a checkout whose code-nerf_amd package (and library) to use")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_scene_scale.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_scale.py: no HIP device -- this benchmark has no CPU fallback")
    if args.package_root:
        sys.path.insert(0, os.path.join(os.path.abspath(args.package_root), "code-nerf_amd"))
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    steps = {"compose": lambda: step_compose(dev, args.reps, args.parent_lib), "render": lambda: step_render(dev, args.reps)}
    results = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results["device"] = torch.cuda.get_device_name(0)
    results["library"] = codenerf.build_info()["version"]
    results["models"] = "synthetic"
    for name in (steps if args.step == "all" else [args.step]):
        results[name] = steps[name]()
        print(json.dumps({name: results[name]}))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
