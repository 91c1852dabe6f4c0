"""Measure per-ray depth spans (ops.sample_span, render_rays' / render_scene's ``span_probes=``) against the
plain renders of the same process.  Needs an MI355X: there is no CPU fallback.

    python tools/bench_ray_span.py [--step launch|render|scene|all] [--reps 30] [--out PATH]
                                   [--checkpoint FILE.ckpt --object K --threshold T]

Each step merges its section into the JSON at --out (default profiles/rayspan/bench_ray_span.json), so the
steps can run as separate commands, each under its own time limit.  All times are device events around one
call; the variants of a step alternate inside one process after a warm-up of all of them, and every figure
carries its spread (min / median / max over the repetitions).  A render under a grid reads its kept counts
back on the host (one per field call), and so does ops.occupancy_cull: their event times include that.

``launch``: the cn_sample_span launch at 16,384 rays, 64 depths, P = 128 / 256 / 512 probes and K = 1 / 4 grids,
beside sample_uniform and beside ops.occupancy_cull (three launches and the read-back) on the same rays.
``render``: one 128 x 128 view, chunk 4096, unperturbed, coarse_rgb=False, a sampler linear in depth over
[0.8, 1.8]: render_rays(occupancy=) with 64 + 64 plain depths against span renders with 64, 32 and 16 coarse
depths (+ 64 fine), P = 256.  ``scene``: bench_scene.py's four-copy scene through render_scene, likewise.
Each render carries its max and mean |rgb_fine - dense| against one dense render of the same rays: 512 plain
coarse depths, no resampling, the fine model (the hierarchical pass cannot take 512 + 64 samples).  So that the
coarse weights steer the resampling towards the density the fine pass integrates -- what a trained pair of
models approximates -- the renders here use the fine model for both passes; the times do not depend on the
weights.  A sample count is reported ``cheaper`` only where its slowest repetition is under the plain
render's fastest.

Grids are spheres (G = 128, bound 1, radius 0.4) and the models the synthetic ones: no trained checkpoint
ships with the repository, so a trained object's spans are NOT measured.  With --checkpoint the models and
object K's codes come from a training checkpoint and the grid from the model's density
(OccupancyGrid.from_density, --threshold).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-nerf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_density import alternate, spread, view_rays  # noqa: E402
from bench_occupancy import G, density_grid_of, load_scene, sphere_grid  # noqa: E402

NEAR, FAR, RHO, BOUND, RADIUS = 0.8, 1.8, 1.3, 1.0, 0.4
PROBES = 256
COARSE = (64, 32, 16)
FINE = 64
DENSE = 512


def the_grid(dev, args, model, emb, zs):
    return density_grid_of(args, model, emb, zs, BOUND) or sphere_grid(dev, BOUND, RADIUS)


def scene_shifts(k):
    """bench_scene.py's k-copy scene: the copies 0.35 apart along z."""
    return [[0.0, 0.0, 0.35 * (j - (k - 1) / 2)] for j in range(k)]


def step_launch(dev, args):
    from codenerf import ops
    from codenerf.nerf import PointSampler
    (mc, _), emb, zs, _ = load_scene(dev, args)
    ro, rd = view_rays(dev, RHO)
    n, nc = ro.shape[0], 64
    ps = PointSampler(nc, FINE, NEAR, FAR, "lindisp", False, torch.float32, dev)
    grid = the_grid(dev, args, mc, emb, zs)
    rays = {1: (ro[None].contiguous(), rd[None].contiguous())}
    rays[4] = ops.object_rays(ro, rd, [([[1, 0, 0], [0, 1, 0], [0, 0, 1]], t) for t in scene_shifts(4)])
    _, z = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
    fns = {"sample_uniform": lambda: ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False),
           "occupancy_cull": lambda: ops.occupancy_cull(ro, rd, z, 4096, grid.bits, grid.resolution, grid.bound,
                                                        want_code=False)}
    for k, (ro_k, rd_k) in rays.items():
        for p in (128, 256, 512):
            fns[f"sample_span/k{k}/p{p}"] = lambda ro_k=ro_k, rd_k=rd_k, k=k, p=p: ops.sample_span(
                ro_k, rd_k, [grid] * k, NEAR, FAR, p, nc)
    ms = alternate(fns, args.reps)
    res = {"shape": {"rays": n, "depths": nc, "grid": grid.resolution, "bound": grid.bound,
                     "occupied_fraction": grid.occupied_fraction()},
           "sample_uniform": spread(ms["sample_uniform"]), "occupancy_cull": spread(ms["occupancy_cull"]),
           "sample_span": {}}
    for k, (ro_k, rd_k) in rays.items():
        for p in (128, 256, 512):
            sp = spread(ms[f"sample_span/k{k}/p{p}"])
            pr = ops.sample_span(ro_k, rd_k, [grid] * k, NEAR, FAR, p, nc)[2]
            res["sample_span"][f"k{k}_p{p}"] = dict(
                sp, hit_fraction=float((pr[:, 0] >= 0).float().mean()),
                lookups_per_s=n * p * k / (sp["median_ms"] * 1e-3),
                over_occupancy_cull_median=sp["median_ms"] / res["occupancy_cull"]["median_ms"])
    return res


def outside_fraction(ops, rays, grids, z, span):
    """Of the dense depths ``z`` occupied in some grid, the share outside their ray's ``span``."""
    n, s = z.shape
    occ = torch.zeros(n * s, dtype=torch.bool, device=z.device)
    for (o, d), g in zip(rays, grids):
        idx = ops.occupancy_cull(o, d, z, n, g.bits, g.resolution, g.bound, want_code=False)[1]
        occ[idx.long()] = True
    occ = occ.view(n, s)
    out = occ & ((z < span[:, :1]) | (z > span[:, 1:]))
    return int(occ.sum()), int(out.sum())


def compare(render, dense_rgb, n, reps):
    """``render(nc, span) -> out``: the plain 64 + 64 render against the span renders, alternating."""
    out = {}
    fns = {"plain_64": lambda: out.__setitem__("plain_64", render(64, None))}
    for nc in COARSE:
        fns[f"span_{nc}"] = lambda nc=nc: out.__setitem__(f"span_{nc}", render(nc, PROBES))
    ms = alternate(fns, reps)
    base = spread(ms["plain_64"])
    res = {}
    for name in fns:
        sp = spread(ms[name])
        err = (out[name]["rgb_fine"] - dense_rgb).abs()
        res[name] = dict(sp, rays_per_s=n / (sp["median_ms"] * 1e-3), over_plain_median=sp["median_ms"] / base["median_ms"],
                         cheaper=name != "plain_64" and sp["max_ms"] < base["min_ms"],
                         max_abs_rgb_error_vs_dense=float(err.max()), mean_abs_rgb_error_vs_dense=float(err.mean()))
    hit = out["span_64"]["ray_hit"]
    width = out["span_64"]["ray_span"][:, 1] - out["span_64"]["ray_span"][:, 0]
    res["hit_fraction"] = float(hit.float().mean())
    res["mean_span_over_range_of_hit_rays"] = float(width[hit].mean()) / (FAR - NEAR) if bool(hit.any()) else None
    return res, out["span_64"]["ray_span"]


def samplers(dev):
    from codenerf.nerf import PointSampler
    ps = {nc: PointSampler(nc, FINE, NEAR, FAR, "lindisp", False, torch.float32, dev) for nc in COARSE}
    ps[DENSE] = PointSampler(DENSE, FINE, NEAR, FAR, "lindisp", False, torch.float32, dev)
    return ps


def step_render(dev, args):
    from codenerf import ops
    from codenerf.nerf import render_rays
    (_, mf), emb, zs, zt = load_scene(dev, args)
    ro, rd = view_rays(dev, RHO)
    n = ro.shape[0]
    grid = the_grid(dev, args, mf, emb, zs)
    z_s, z_t = zs.expand(n, -1), zt.expand(n, -1)
    ps = samplers(dev)

    def render(nc, span, **kw):
        with torch.no_grad():
            return render_rays(ro, rd, z_s, z_t, ps[nc], emb, mf, mf, chunk_rows=4096, occupancy=grid,
                               **(kw or dict(coarse_rgb=False, span_probes=span)))

    dense = render(DENSE, None, coarse_only=True)
    res, span = compare(render, dense["rgb_coarse"], n, args.reps)
    occupied, outside = outside_fraction(ops, [(ro, rd)], [grid], dense["z_coarse"], span)
    res.update({"shape": {"rays": n, "fine": FINE, "chunk_rows": 4096, "coarse_rgb": False, "probes": PROBES,
                          "near": NEAR, "far": FAR, "grid": grid.resolution, "bound": grid.bound,
                          "occupied_fraction": grid.occupied_fraction(), "dense_depths": DENSE},
                "dense_occupied_samples": occupied, "dense_occupied_samples_outside_span": outside,
                "outside_fraction": outside / max(occupied, 1)})
    return res


def step_scene(dev, args):
    from codenerf import ops
    from codenerf.nerf import SceneObject, render_scene
    (_, mf), emb, zs, zt = load_scene(dev, args)
    ro, rd = view_rays(dev, RHO)
    n = ro.shape[0]
    grid = the_grid(dev, args, mf, emb, zs)
    shifts = scene_shifts(4)
    objects = [SceneObject(zs, zt, grid, translation=t) for t in shifts]
    ps = samplers(dev)

    def render(nc, span, **kw):
        with torch.no_grad():
            return render_scene(ro, rd, objects, ps[nc], emb, mf, mf, **(kw or dict(coarse_rgb=False, span_probes=span)))

    dense = render(DENSE, None, coarse_only=True)
    res, span = compare(render, dense["rgb_coarse"], n, args.reps)
    rays = [(ro - torch.tensor(t, device=dev), rd) for t in shifts]
    occupied, outside = outside_fraction(ops, rays, [grid] * 4, dense["z_coarse"], span)
    res.update({"shape": {"rays": n, "objects": 4, "translations": shifts, "fine": FINE, "coarse_rgb": False,
                          "probes": PROBES, "near": NEAR, "far": FAR, "grid": grid.resolution, "bound": grid.bound,
                          "dense_depths": DENSE},
                "dense_occupied_samples": occupied, "dense_occupied_samples_outside_span": outside,
                "outside_fraction": outside / max(occupied, 1)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("launch", "render", "scene", "all"))
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each variant (>= 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rayspan", "bench_ray_span.json"))
    ap.add_argument("--checkpoint", help="a training checkpoint (.ckpt): its models and codes instead of the synthetic ones")
    ap.add_argument("--object", type=int, default=0, help="the checkpoint's object (code row) to render")
    ap.add_argument("--threshold", type=float, help="activated-density threshold of the checkpoint's density grid")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_ray_span.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ray_span.py: no HIP device -- this benchmark has no CPU fallback")
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    steps = {"launch": lambda: step_launch(dev, args), "render": lambda: step_render(dev, args),
             "scene": lambda: step_scene(dev, args)}
    results = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results["device"] = torch.cuda.get_device_name(0)
    results["library"] = codenerf.build_info()["version"]
    results["models"] = args.checkpoint and os.path.basename(args.checkpoint) or "synthetic"
    for name in (steps if args.step == "all" else [args.step]):
        results[name] = steps[name]()
        print(json.dumps({name: results[name]}))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
