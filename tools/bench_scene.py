"""Measure scene rendering: the composition launch (cn_volume_render_compose) and render_scene against
separate single-object renders, in one process.  Needs an MI355X: there is no CPU fallback.

    python tools/bench_scene.py [--step compose|render|all] [--reps 30] [--out PATH]

Each step merges its section into the JSON at --out (default profiles/scene/bench_scene.json).  All times
are device events around one call; the variants of a step alternate inside one process after a warm-up of
all of them, and every figure carries its spread (min / median / max over the repetitions).

``compose``: 16,384 rays, S = 64 and 192, K = 1, 2, 4, 8 objects of random raw rows (about half of each
object's slots empty, as after a cull), in GB/s of the launch's algorithmic traffic -- (16 K + 4) S + 12
bytes in and 4 S + 20 + 4 K out per ray -- beside cn_volume_render on the first object's tensor.
``render``: one 128 x 128 view, 64 + 64 samples, unperturbed; render_scene of K = 1, 2, 4 copies of one
synthetic object translated along a line (sphere grids of radius 0.4, G = 128) against K separate
render_rays(occupancy=) calls on the objects' own rays, and K = 1 against render_rays(occupancy=) itself.
The K separate renders are what a host-side blend of finished images would start from (the blend itself
is not timed); they do not compute the same image where the objects overlap on a ray.
The models are the synthetic ones: no trained checkpoint ships with the repository, so what trained
objects look like in a scene is not measured here.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-nerf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_density import alternate, setup, spread, view_rays  # noqa: E402
from bench_occupancy import G, sphere_grid  # noqa: E402

RAYS = 16384
EMPTY_ROW = (0.0, 0.0, 0.0, -1.0e4)


def compose_bytes(n, s, k):
    return n * (12 + (16 * k + 4) * s + 4 * s + 20 + 4 * k)


def step_compose(dev, reps):
    from codenerf import ops
    res = {"shape": {"rays": RAYS}, "launches": {}}
    for s in (64, 192):
        g = torch.Generator().manual_seed(s)
        z = torch.sort(1 + torch.rand(RAYS, s, generator=g), -1).values.to(dev)
        rd = torch.randn(RAYS, 3, generator=g).to(dev)
        raws = []
        for _ in range(8):
            raw = torch.randn(RAYS, s, 4, generator=g) * 2
            raw[torch.rand(RAYS, s, generator=g) < 0.5] = torch.tensor(EMPTY_ROW)
            raws.append(raw.to(dev))
        out = {}
        fns = {"volume_render": lambda: out.__setitem__("plain", ops.volume_render(raws[0], z, rd))}
        for k in (1, 2, 4, 8):
            fns[f"compose_k{k}"] = lambda k=k: out.__setitem__(k, ops.volume_render_compose(raws[:k], z, rd))
        ms = alternate(fns, reps)
        assert all(torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) for a, b in zip(out[1][:5], out["plain"])), \
            "one composed object differs from cn_volume_render"
        sec = {}
        for name, k in (("volume_render", 1), ("compose_k1", 1), ("compose_k2", 2), ("compose_k4", 4), ("compose_k8", 8)):
            sp = spread(ms[name])
            nbytes = compose_bytes(RAYS, s, k) - (4 * k * RAYS if name == "volume_render" else 0)
            sec[name] = dict(sp, objects=k, bytes=nbytes, gb_per_s=nbytes / (sp["median_ms"] * 1e-3) / 1e9)
        a, b = sec["compose_k1"], sec["volume_render"]
        sec["k1_over_volume_render_median"] = a["median_ms"] / b["median_ms"]
        sec["k1_slower_beyond_spread"] = a["min_ms"] > b["max_ms"]
        res["launches"][f"s{s}"] = sec
    return res


def step_render(dev, reps):
    from codenerf.nerf import PointSampler, SceneObject, render_rays, render_scene
    (mc, mf), emb, zs, zt = setup(dev)
    ro, rd = view_rays(dev, 1.3)
    n = ro.shape[0]
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    grid = sphere_grid(dev, 1.0, 0.4)
    z_s, z_t = zs.expand(n, -1), zt.expand(n, -1)
    res = {"shape": {"rays": n, "coarse": 64, "fine_pass_samples": 128, "grid": G, "bound": 1.0, "sphere_radius": 0.4,
                     "occupied_fraction": grid.occupied_fraction()}, "scenes": {}}
    out = {}
    for k in (1, 2, 4):
        shifts = [[0.0, 0.0, 0.35 * (j - (k - 1) / 2)] for j in range(k)]
        objects = [SceneObject(zs, zt, grid, translation=t) for t in shifts]
        rays = [(ro - torch.tensor(t, device=dev), rd) for t in shifts]

        def scene(k=k, objects=objects):
            with torch.no_grad():
                out[k] = render_scene(ro, rd, objects, ps, emb, mc, mf)

        def separate(k=k, rays=rays):
            with torch.no_grad():
                out[-k] = [render_rays(o, d, z_s, z_t, ps, emb, mc, mf, chunk_rows=None, occupancy=grid)
                           for o, d in rays]

        ms = alternate({"render_scene": scene, "separate_render_rays": separate}, reps)
        a, b = spread(ms["render_scene"]), spread(ms["separate_render_rays"])
        sec = {"render_scene": dict(a, rays_per_s=n / (a["median_ms"] * 1e-3)),
               "separate_render_rays": dict(b, rays_per_s=n / (b["median_ms"] * 1e-3)),
               "scene_over_separate_median": a["median_ms"] / b["median_ms"],
               "beyond_spread": a["max_ms"] < b["min_ms"] or a["min_ms"] > b["max_ms"],
               "covered_fraction": float((out[k]["acc_fine"] > 0).float().mean()),
               "translations": shifts}
        if k == 1:
            sec["bit_equal_to_render_rays"] = all(
                torch.equal(torch.nan_to_num(out[1][key]), torch.nan_to_num(v)) for key, v in out[-1][0].items())
            assert sec["bit_equal_to_render_rays"], "a scene of one object differs from render_rays(occupancy=)"
        res["scenes"][f"k{k}"] = sec
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("compose", "render", "all"))
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each variant (>= 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene", "bench_scene.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_scene.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene.py: no HIP device -- this benchmark has no CPU fallback")
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    steps = {"compose": lambda: step_compose(dev, args.reps), "render": lambda: step_render(dev, args.reps)}
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
