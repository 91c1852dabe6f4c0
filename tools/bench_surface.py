"""Measure iso-surface ray casting (nerf.render_surface and its three launches) against the volumetric render of
the same rays in the same process.  Needs an MI355X: there is no CPU fallback.

    python tools/bench_surface.py [--step render|launch|all] [--reps 30] [--out PATH]

Each step merges its section into the JSON at --out (default profiles/surface/bench_surface.json).  All times are
device events around one call; the variants of a step alternate inside one process after a warm-up of all of
them, and every figure carries its spread (min / median / max over the repetitions).

``render``: one 128 x 128 view (16,384 rays), 64 search depths linear in depth over [0.8, 1.8] (spacing_mode
"lindisp": quirk Q2's name for linear depth), the level the median sigma_raw of the search samples
(activated=False), refine in {0, 3, 6}, without a grid and with a sphere grid (G = 128, bound 1, radius 0.4) +
span_probes=256, beside render_rays(coarse_rgb=False) with 64 + 64 depths (chunk 4096) on the same rays.  Quality: mean |depth - depth at refine = 12| over the rays both calls hit.
A render under a grid reads its kept count back on the host once: its event time includes that.
``launch``: cn_surface_bracket (densities contiguous, and as column 3 of raw rows), cn_surface_step (an update
and the next depth) and cn_surface_shade on their own at 16,384 rays, with achieved bytes/s beside the
6.29 TB/s a copy reaches on this chip (README).  Bytes are what the rule makes each launch touch: for the
bracket the 64-sample groups each ray reads up to its crossing, whole 16-byte rows at stride 4.

The models are the synthetic ones: no trained checkpoint ships with the repository, so a trained object's
surface is NOT measured.
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
from bench_occupancy import sphere_grid  # noqa: E402

NEAR, FAR, RHO, BOUND, RADIUS = 0.8, 1.8, 1.3, 1.0, 0.4
SEARCH, FINE, PROBES = 64, 64, 256
REFINES = (0, 3, 6)
REFERENCE_REFINE = 12
COPY_BYTES_PER_S = 6.29e12


def search_level(dev, model, emb, zs, ro, rd, ps):
    """The median sigma_raw of the unperturbed search samples -> (level, z, raw (R, S, 4))."""
    from codenerf import ops
    from codenerf.models.model import density_code_bias
    _, z = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
    raw = ops.density_field(model.packed(), density_code_bias(model, zs), emb[0].freqs, ro=ro, rd=rd, z=z,
                            want_sigma=False, want_raw=True)
    return float(raw[..., 3].flatten().median()), z, raw


def step_render(dev, args):
    from codenerf.nerf import PointSampler, render_rays, render_surface
    (mc, mf), emb, zs, zt = setup(dev)
    ro, rd = view_rays(dev, RHO)
    n = ro.shape[0]
    z_s, z_t = zs.expand(n, -1), zt.expand(n, -1)
    ps = PointSampler(SEARCH, FINE, NEAR, FAR, "lindisp", False, torch.float32, dev)
    grid = sphere_grid(dev, BOUND, RADIUS)
    level, _, _ = search_level(dev, mf, emb, zs, ro, rd, ps)
    forms = {"plain": {}, "grid_span": dict(occupancy=grid, span_probes=PROBES)}

    def surface(refine, **kw):
        with torch.no_grad():
            return render_surface(ro, rd, z_s, z_t, ps, emb, mf, level, activated=False, refine=refine, **kw)

    out = {}
    fns = {"render_rays_64_64": lambda: out.__setitem__("volumetric", _volumetric(render_rays, ro, rd, z_s, z_t, ps,
                                                                                   emb, mc, mf))}
    for form, kw in forms.items():
        for refine in REFINES:
            fns[f"{form}/refine{refine}"] = lambda refine=refine, kw=kw, form=form: out.__setitem__(
                (form, refine), surface(refine, **kw))
    ms = alternate(fns, args.reps)
    base = spread(ms["render_rays_64_64"])
    res = {"shape": {"rays": n, "search_depths": SEARCH, "near": NEAR, "far": FAR, "level_sigma_raw": level,
                     "activated": False, "grid": grid.resolution, "bound": grid.bound, "radius": RADIUS,
                     "occupied_fraction": grid.occupied_fraction(), "probes": PROBES,
                     "reference_refine": REFERENCE_REFINE},
           "render_rays_64_64": dict(base, rays_per_s=n / (base["median_ms"] * 1e-3))}
    for form, kw in forms.items():
        ref = surface(REFERENCE_REFINE, **kw)
        res[form] = {}
        for refine in REFINES:
            sp = spread(ms[f"{form}/refine{refine}"])
            got = out[(form, refine)]
            both = (got["hit"] == 1) & (ref["hit"] == 1)
            err = (got["depth"] - ref["depth"])[both].abs()
            hit = got["hit"]
            res[form][f"refine{refine}"] = dict(
                sp, rays_per_s=n / (sp["median_ms"] * 1e-3), over_render_rays_median=sp["median_ms"] / base["median_ms"],
                cheaper=sp["max_ms"] < base["min_ms"],
                hit_fractions={str(h): float((hit == h).float().mean()) for h in (0, 1, 2)},
                mean_abs_depth_error_vs_reference=float(err.mean()) if bool(both.any()) else None,
                max_abs_depth_error_vs_reference=float(err.max()) if bool(both.any()) else None)
    return res


def _volumetric(render_rays, ro, rd, z_s, z_t, ps, emb, mc, mf):
    with torch.no_grad():
        return render_rays(ro, rd, z_s, z_t, ps, emb, mc, mf, chunk_rows=4096, coarse_rgb=False)


def step_launch(dev, args):
    from codenerf import ops
    from codenerf.nerf import PointSampler
    (_, mf), emb, zs, _ = setup(dev)
    ro, rd = view_rays(dev, RHO)
    n = ro.shape[0]
    ps = PointSampler(SEARCH, FINE, NEAR, FAR, "lindisp", False, torch.float32, dev)
    level, z, raw = search_level(dev, mf, emb, zs, ro, rd, ps)
    sigma = raw[..., 3].contiguous()
    bracket, hit = ops.surface_bracket(sigma, z, level)
    work = bracket.clone()
    t, pts = ops.surface_step(ro, rd, hit, work, level)
    probe = torch.full((n,), level - 1.0, device=dev)          # below the level: the low end moves every time
    field = torch.randn(n, 4, device=dev)
    fns = {"bracket_stride1": lambda: ops.surface_bracket(sigma, z, level, bracket=bracket, hit=hit),
           "bracket_stride4": lambda: ops.surface_bracket(raw[..., 3], z, level, bracket=bracket, hit=hit),
           "step": lambda: ops.surface_step(ro, rd, hit, work, level, t=t, probe=probe, pts=pts),
           "shade": lambda: ops.surface_shade(field, hit, t, pts)}
    ms = alternate(fns, args.reps)
    # the first crossing's 64-sample group per ray (all of them for a miss): what the bracket kernel reads
    first = torch.where((sigma >= level).any(dim=1), (sigma >= level).float().argmax(dim=1),
                        torch.full((n,), SEARCH - 1, device=dev))
    groups = int((first // 64 + 1).sum())
    live, miss = int((hit == 1).sum()), int((hit == 0).sum())
    touched = {"bracket_stride1": groups * 64 * 4 + n * (16 + 16 + 4),
               "bracket_stride4": groups * 64 * 16 + n * (8 + 32 + 16 + 4),
               "step": n * (12 + 12 + 4 + 16 + 4 + 12) + live * (4 + 4 + 16),
               "shade": n * (4 + 12 + 4) + (n - miss) * (16 + 4) + miss * 12}
    res = {"shape": {"rays": n, "search_depths": SEARCH, "hit_fractions": {
        str(h): float((hit == h).float().mean()) for h in (0, 1, 2)}}, "copy_bytes_per_s": COPY_BYTES_PER_S}
    for name in fns:
        sp = spread(ms[name])
        rate = touched[name] / (sp["median_ms"] * 1e-3)
        res[name] = dict(sp, bytes=touched[name], bytes_per_s=rate, of_copy=rate / COPY_BYTES_PER_S)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("render", "launch", "all"))
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each variant (>= 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface", "bench_surface.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_surface.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface.py: no HIP device -- this benchmark has no CPU fallback")
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    steps = {"render": lambda: step_render(dev, args), "launch": lambda: step_launch(dev, args)}
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
