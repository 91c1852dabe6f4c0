"""Measure what the culled renders' host read-backs cost: render_rays / render_scene with ``sync_free=False``
(the kept count read back once per field call) against ``sync_free=True`` run eagerly and ``sync_free=True``
captured in a graph and replayed, in one process.  Needs an MI355X: there is no CPU fallback.

    python tools/bench_sync_free.py [--step render|scene|tolerance|small|all] [--reps 30] [--out PATH]

Each step merges its section into the JSON at --out (default profiles/syncfree/bench_sync_free.json).  The
setup is tools/bench_occupancy.py's: the synthetic models, one 128 x 128 view at 64 + 64 samples, chunk 4096,
unperturbed, coarse_rgb=False, G = 128 grids -- the full grid and spheres whose MEASURED kept fraction of the
coarse samples is near 0.5, 0.25 and 0.1.  All times are device events around one call (for the graph: around
one replay); the three variants of a grid alternate after a warm-up of all of them, and every figure carries
its spread (min / median / max over the repetitions).  The synchronising call's event time includes its
read-backs: the launch that follows one cannot be enqueued before it returns.  A difference is "beyond the
spread" when every repetition of one variant beat every repetition of the other.

``render``: render_rays(occupancy=) under each grid.  ``scene``: tools/bench_scene.py's four copies of one
object along a line (sphere grids of radius 0.4), render_scene.  ``tolerance``: render_rays(occupancy=,
rgb_tolerance=1e-3) under the 0.25 sphere.  ``small``: render_rays(occupancy=) under a sphere that keeps about
0.01 of the coarse samples, fewer tiles than the capacity-sized launch has workgroups.  Before timing, each variant's result is compared with the
synchronising render's, bit for bit.  The models are synthetic, so the kept fractions are chosen, not a trained
object's.
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
from bench_occupancy import G, kept_fraction, make_grids, sphere_grid  # noqa: E402

GRIDS = ("full", "sphere_0.5", "sphere_0.25", "sphere_0.1")
VARIANTS = ("sync", "sync_free", "sync_free_graph")


def same_bits(a, b):
    return sorted(a) == sorted(b) and all(
        torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)) for k in a)


def compare(fast, slow):
    """``fast`` over ``slow`` by their medians, and whether either beat the other in every repetition."""
    return {"over_sync_median": fast["median_ms"] / slow["median_ms"],
            "faster_beyond_spread": fast["max_ms"] < slow["min_ms"],
            "slower_beyond_spread": fast["min_ms"] > slow["max_ms"]}


def three_ways(render, reps):
    """``render(sync_free)`` -> a result dict.  Times the synchronising call, the sync-free call and the sync-free
    call's captured graph, alternating -> the three spreads and the two comparisons against the first."""
    out = {}
    ref = render(False)
    assert same_bits(render(True), ref), "the sync-free render differs from the synchronising one"
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        out["graph"] = render(True)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out["graph"], ref), "the replayed graph's render differs from the synchronising one"
    ms = alternate({"sync": lambda: render(False), "sync_free": lambda: render(True),
                    "sync_free_graph": graph.replay}, reps)
    res = {k: spread(ms[k]) for k in VARIANTS}
    for k in VARIANTS[1:]:
        res[k].update(compare(res[k], res["sync"]))
    return res


def small_grid(dev, bound, ro, rd, z, target=0.01):
    """A sphere whose kept fraction of the samples ``z`` is near ``target``: so few rows that most workgroups
    of a capacity-sized launch get no tile (256 tiles are 3 % of the coarse pass)."""
    lo, hi = 0.0, 2.0 * bound
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        if kept_fraction(sphere_grid(dev, bound, mid), ro, rd, z) < target:
            lo = mid
        else:
            hi = mid
    grid = sphere_grid(dev, bound, hi)
    return grid, kept_fraction(grid, ro, rd, z)


def step_render(dev, reps, tolerance=None, small=False):
    from codenerf import ops
    from codenerf.nerf import PointSampler, render_rays
    (mc, mf), emb, zs, zt = setup(dev)
    ro, rd = view_rays(dev, 1.3)
    n = ro.shape[0]
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    z_s, z_t = zs.expand(n, -1), zt.expand(n, -1)
    _, z_c = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
    grids = {"sphere_0.01": small_grid(dev, 4.0, ro, rd, z_c)} if small else make_grids(dev, 4.0, ro, rd, z_c)
    res = {"shape": {"rays": n, "coarse": 64, "fine_pass_samples": 128, "chunk_rows": 4096, "coarse_rgb": False,
                     "fold": bool(mf.fold), "grid": G, "bound": 4.0, "rgb_tolerance": tolerance,
                     "read_backs_per_sync_render": 2 if tolerance is None else 3}, "grids": {}}
    for name in (("sphere_0.01",) if small else GRIDS if tolerance is None else ("sphere_0.25",)):
        grid, frac = grids[name]

        def render(sync_free, grid=grid):
            with torch.no_grad():
                return render_rays(ro, rd, z_s, z_t, ps, emb, mc, mf, chunk_rows=4096, coarse_rgb=False,
                                   occupancy=grid, rgb_tolerance=tolerance, sync_free=sync_free)

        sec = three_ways(render, reps)
        sec["kept_fraction_coarse"] = frac
        sec["kept_fraction_fine"] = kept_fraction(grid, ro, rd, render(False)["z_fine"])
        res["grids"][name] = sec
    return res


def step_scene(dev, reps):
    from codenerf.nerf import PointSampler, SceneObject, render_scene
    (mc, mf), emb, zs, zt = setup(dev)
    ro, rd = view_rays(dev, 1.3)
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    grid = sphere_grid(dev, 1.0, 0.4)
    k = 4
    shifts = [[0.0, 0.0, 0.35 * (j - (k - 1) / 2)] for j in range(k)]
    objects = [SceneObject(zs, zt, grid, translation=t) for t in shifts]

    def render(sync_free):
        with torch.no_grad():
            return render_scene(ro, rd, objects, ps, emb, mc, mf, sync_free=sync_free)

    res = three_ways(render, reps)
    res["shape"] = {"rays": ro.shape[0], "objects": k, "coarse": 64, "fine_pass_samples": 128, "grid": G, "bound": 1.0,
                    "sphere_radius": 0.4, "translations": shifts, "read_backs_per_sync_render": 2 * k}
    res["covered_fraction"] = float((render(False)["acc_fine"] > 0).float().mean())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("render", "scene", "tolerance", "small", "all"))
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each variant (>= 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "syncfree", "bench_sync_free.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_sync_free.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_sync_free.py: no HIP device -- this benchmark has no CPU fallback")
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    steps = {"render": lambda: step_render(dev, args.reps), "scene": lambda: step_scene(dev, args.reps),
             "tolerance": lambda: step_render(dev, args.reps, tolerance=1e-3),
             "small": lambda: step_render(dev, args.reps, small=True)}
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
