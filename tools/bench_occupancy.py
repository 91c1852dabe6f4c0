"""Measure occupancy-grid sample culling (render_rays' ``occupancy=``) against the unculled render of
the same process.  Needs an MI355X: there is no CPU fallback.

    python tools/bench_occupancy.py [--step coarse|c3|chairs|all] [--reps 30] [--out PATH]
                                    [--checkpoint FILE.ckpt --object K --threshold T]

Each step merges its section into the JSON at --out (default profiles/occupancy/bench_occupancy.json),
so the steps can run as separate commands, each under its own time limit.  All times are device
events around one call; the variants of a step alternate inside one process after a warm-up of all
of them, and every figure carries its spread (min / median / max over the repetitions).  A culled
call's event time includes its host read-backs of the kept count (one per field call): the launch
that follows cannot be enqueued before it.

Grids: ``full`` and spheres around the origin whose MEASURED kept fraction of the coarse samples is
near 1.0, 0.5, 0.25 and 0.1 (the radius is bisected on the step's own rays).  The models are the
synthetic ones (no trained checkpoint ships with the repository), so the fractions are chosen, not a
scene's; with --checkpoint the models and object K's codes come from a training checkpoint and a sixth
grid, ``density``, is built from the model's density (OccupancyGrid.from_density, --threshold).
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

G = 128                 # grid resolution
TARGETS = (1.0, 0.5, 0.25, 0.1)


def sphere_grid(dev, bound, radius):
    from codenerf.nerf import OccupancyGrid
    c = (torch.arange(G, device=dev, dtype=torch.float32) + 0.5) * (2.0 * bound / G) - bound
    occ = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) < radius * radius
    w = (occ.reshape(-1, 32).to(torch.int64) << torch.arange(32, device=dev)).sum(dim=1)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)        # bit 31 is the sign
    return OccupancyGrid(w, G, bound)


def kept_fraction(grid, ro, rd, z):
    from codenerf import ops
    return ops.occupancy_cull(ro, rd, z, ro.shape[0], grid.bits, grid.resolution, grid.bound, want_code=False)[0] \
        / float(z.numel())


def make_grids(dev, bound, ro, rd, z, extra=None):
    """name -> (grid, measured kept fraction of the samples z): full, then a sphere per target."""
    from codenerf.nerf import OccupancyGrid
    grids = {"full": OccupancyGrid.full(G, bound, dev)}
    for target in TARGETS:
        lo, hi = 0.0, 2.0 * bound            # hi holds the whole cube
        for _ in range(24):
            mid = 0.5 * (lo + hi)
            if kept_fraction(sphere_grid(dev, bound, mid), ro, rd, z) < target:
                lo = mid
            else:
                hi = mid
        grids[f"sphere_{target:g}"] = sphere_grid(dev, bound, hi)
    if extra is not None:
        grids["density"] = extra
    return {k: (g, kept_fraction(g, ro, rd, z)) for k, g in grids.items()}


def break_even(points, base_ms):
    """The coarse kept fraction at which the culled call's median equals the unculled one's: linear
    between the two measured grids that bracket it; None when every measured grid is on one side."""
    pts = sorted(points)
    for (f0, t0), (f1, t1) in zip(pts, pts[1:]):
        if (t0 - base_ms) * (t1 - base_ms) <= 0 and t0 != t1:
            return f0 + (base_ms - t0) * (f1 - f0) / (t1 - t0)
    return None


def load_scene(dev, args):
    """-> (coarse, fine), embedders, z_s (1, 256), z_t (1, 256): synthetic, or a checkpoint's."""
    (mc, mf), emb, zs, zt = setup(dev)
    if args.checkpoint:
        ck = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
        strip = lambda sd: {k[7:] if k.startswith("module.") else k: v for k, v in sd.items()}
        mc.load_state_dict(strip(ck["model_nerf_coarse_state_dict"]))
        mf.load_state_dict(strip(ck["model_nerf_fine_state_dict"]))
        e = strip(ck["model_embedding_state_dict"])
        zs = e["shape_embedding.weight"][args.object:args.object + 1].to(dev).float()
        zt = e["texture_embedding.weight"][args.object:args.object + 1].to(dev).float()
    return (mc, mf), emb, zs, zt


def density_grid_of(args, model, emb, zs, bound):
    from codenerf.nerf import OccupancyGrid
    if not args.checkpoint:
        return None
    if args.threshold is None:
        raise SystemExit("bench_occupancy.py: --checkpoint needs --threshold (activated density)")
    return OccupancyGrid.from_density(model, emb, zs, resolution=G, bound=bound, threshold=args.threshold)


def step_coarse(dev, args):
    """The C2 coarse pass alone (16,384 rays x 64 samples, density kernel, chunk 4096): the cull, field
    and expand calls timed one by one, and cull + field + expand against the unculled launch."""
    from codenerf import ops
    from codenerf.models.model import density_code_bias
    from codenerf.nerf import PointSampler
    (mc, _), emb, zs, _ = load_scene(dev, args)
    ro, rd = view_rays(dev, 1.3)
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    _, z = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
    n, s = z.shape
    bound = 4.0
    packed, cb, fx = mc.packed(), density_code_bias(mc, zs), emb[0].freqs
    grids = make_grids(dev, bound, ro, rd, z, density_grid_of(args, mc, emb, zs, bound))

    def cull(g):
        return ops.occupancy_cull(ro, rd, z, 4096, g.bits, g.resolution, g.bound, want_code=False)

    def field(pts):
        return ops.density_field(packed, cb, fx, pts=pts, want_sigma=False, want_raw=True) if pts.shape[0] else None

    def whole(g):
        count, _, pts, _, _, state = cull(g)
        return ops.occupancy_expand(field(pts), state)

    fns = {"unculled": lambda: ops.density_field(packed, cb, fx, ro=ro, rd=rd, z=z, want_sigma=False, want_raw=True)}
    held = {}
    for name, (g, _) in grids.items():
        held[name] = cull(g)
        fns[f"{name}/cull"] = lambda g=g: cull(g)
        fns[f"{name}/field"] = lambda name=name: field(held[name][2])
        fns[f"{name}/expand"] = lambda name=name: ops.occupancy_expand(field_out[name], held[name][5])
        fns[f"{name}/whole"] = lambda g=g: whole(g)
    field_out = {name: field(held[name][2]) for name in grids}
    ms = alternate(fns, args.reps)
    base = spread(ms["unculled"])
    res = {"shape": {"rays": n, "samples": s, "chunk_rows": 4096, "kernel": "density", "grid": G, "bound": bound},
           "unculled": base, "grids": {}}
    for name, (g, frac) in grids.items():
        parts = {k: spread(ms[f"{name}/{k}"]) for k in ("cull", "field", "expand", "whole")}
        res["grids"][name] = dict(parts, kept_fraction=frac, occupied_fraction=g.occupied_fraction(),
                                  whole_over_unculled_median=parts["whole"]["median_ms"] / base["median_ms"],
                                  field_over_unculled_median=parts["field"]["median_ms"] / base["median_ms"])
    res["overhead_at_full_ms_median"] = res["grids"]["full"]["whole"]["median_ms"] - base["median_ms"]
    res["break_even_kept_fraction"] = break_even(
        [(v["kept_fraction"], v["whole"]["median_ms"]) for v in res["grids"].values()], base["median_ms"])
    return res


def step_render(dev, args, nc, nf, near, far, rho, bound):
    """One 128 x 128 view, chunk 4096, unperturbed, coarse_rgb=False, fold on: render_rays unculled and
    under every grid, alternating."""
    from codenerf import ops
    from codenerf.nerf import PointSampler, render_rays
    (mc, mf), emb, zs, zt = load_scene(dev, args)
    ro, rd = view_rays(dev, rho)
    n = ro.shape[0]
    ps = PointSampler(nc, nf, near, far, "lindepth", False, torch.float32, dev)
    z_s, z_t = zs.expand(n, -1), zt.expand(n, -1)
    _, z_c = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
    grids = make_grids(dev, bound, ro, rd, z_c, density_grid_of(args, mc, emb, zs, bound))
    out = {}

    def render(key, grid):
        with torch.no_grad():
            out[key] = render_rays(ro, rd, z_s, z_t, ps, emb, mc, mf, chunk_rows=4096, coarse_rgb=False, occupancy=grid)

    fns = {"unculled": lambda: render("unculled", None)}
    for name, (g, _) in grids.items():
        fns[name] = lambda name=name, g=g: render(name, g)
    ms = alternate(fns, args.reps)
    base = spread(ms["unculled"])
    full_equal = all(torch.equal(out["full"][k], out["unculled"][k]) for k in out["unculled"])
    assert full_equal, "the full-grid render differs from the unculled one"
    res = {"shape": {"rays": n, "coarse": nc, "fine_pass_samples": nc + nf, "chunk_rows": 4096, "coarse_rgb": False,
                     "fold": bool(mf.fold), "grid": G, "bound": bound},
           "unculled": dict(base, rays_per_s=n / (base["median_ms"] * 1e-3)), "full_grid_bit_equal": full_equal,
           "grids": {}}
    for name, (g, frac_c) in grids.items():
        sp = spread(ms[name])
        res["grids"][name] = dict(sp, kept_fraction_coarse=frac_c,
                                  kept_fraction_fine=kept_fraction(g, ro, rd, out[name]["z_fine"]),
                                  occupied_fraction=g.occupied_fraction(), rays_per_s=n / (sp["median_ms"] * 1e-3),
                                  over_unculled_median=sp["median_ms"] / base["median_ms"],
                                  beyond_spread=sp["max_ms"] < base["min_ms"] or sp["min_ms"] > base["max_ms"])
    res["overhead_at_full_ms_median"] = res["grids"]["full"]["median_ms"] - base["median_ms"]
    res["break_even_kept_fraction_coarse"] = break_even(
        [(v["kept_fraction_coarse"], v["median_ms"]) for v in res["grids"].values()], base["median_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("coarse", "c3", "chairs", "all"))
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each variant (>= 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy", "bench_occupancy.json"))
    ap.add_argument("--checkpoint", help="a training checkpoint (.ckpt): its models and codes instead of the synthetic ones")
    ap.add_argument("--object", type=int, default=0, help="the checkpoint's object (code row) to render")
    ap.add_argument("--threshold", type=float, help="activated-density threshold of the checkpoint's density grid")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_occupancy.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_occupancy.py: no HIP device -- this benchmark has no CPU fallback")
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    steps = {"coarse": lambda: step_coarse(dev, args),
             "c3": lambda: step_render(dev, args, 64, 64, 0.8, 1.8, 1.3, 4.0),
             "chairs": lambda: step_render(dev, args, 32, 128, 1.25, 2.75, 2.0, 6.0)}
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
