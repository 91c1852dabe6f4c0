"""Measure weight-bounded colour culling (render_rays' ``rgb_tolerance=``) against the plain render of
the same process.  Needs an MI355X: there is no CPU fallback.

    python tools/bench_weight_cull.py [--step c3|chairs|steps|all] [--reps 30] [--tol 1e-3] [--out PATH]
                                      [--checkpoint FILE.ckpt --object K]

Each step merges its section into the JSON at --out (default profiles/weightcull/bench_weight_cull.json),
so the steps can run as separate commands, each under its own time limit.  All times are device
events around one call; the variants of a step alternate inside one process after a warm-up of all
of them, and every figure carries its spread (min / median / max over the repetitions).  A two-phase
call's event time includes its host read-back of the kept count: the field launch over the kept rows
cannot be enqueued before it.

Renders (c3: 64 + 64 over [0.8, 1.8]; chairs: 32 + 128 over [1.25, 2.75]): one 128 x 128 view, chunk
4096, unperturbed, coarse_rgb=False, fold on; the plain fine pass against the two-phase one at fine
kept fractions near 1.0, 0.5, 0.25 and 0.1, then once more under a sphere occupancy grid.  The
models are the synthetic ones (no trained checkpoint ships with the repository): the fractions are
CHOSEN, by bisecting a bias added to the fine model's sigma_raw output (fc_out.bias[0]) until the
measured kept fraction of the step's own fine samples reaches the target -- they are not a scene's.
With --checkpoint the models and object K's codes come from a training checkpoint and a variant
``checkpoint`` renders them as they are (its kept fraction is then the object's own at that view).

Every variant is checked while it is timed: each entry of the two-phase result but "rgb_fine" is the
plain render's, bit for bit (NaN in the same places for disp / depth), and every channel of
"rgb_fine" is within 0.501 tol + 2 S 2^-24 of it.

steps: the five parts of the two-phase fine pass of c3 timed one by one at each fraction -- the
density launch, the extra volume_render, the cull with its read-back, the field over the kept rows
and the scatter -- next to the plain fine field launch.
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-nerf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_density import alternate, spread, view_rays  # noqa: E402
from bench_occupancy import break_even, kept_fraction, load_scene, sphere_grid  # noqa: E402

TARGETS = (1.0, 0.5, 0.25, 0.1)
SHAPES = {"c3": (64, 64, 0.8, 1.8, 1.3, 4.0), "chairs": (32, 128, 1.25, 2.75, 2.0, 6.0)}
CHUNK = 4096
GRID_KEPT = 0.5         # share of the ungridded fine samples inside the sphere grid of the last run


class Scene:
    """One view's rays, the samplers' fine depths (they depend on the coarse model alone) and fine
    models with a chosen sigma bias."""

    def __init__(self, dev, args, shape):
        from codenerf import ops
        from codenerf.nerf import PointSampler, render_rays
        nc, nf, near, far, rho, bound = SHAPES[shape]
        (self.mc, self.mf), self.emb, zs, zt = load_scene(dev, args)
        self.dev, self.tol, self.bound, self.s = dev, args.tol, bound, nc + nf
        self.ro, self.rd = view_rays(dev, rho)
        self.n = self.ro.shape[0]
        self.ps = PointSampler(nc, nf, near, far, "lindepth", False, torch.float32, dev)
        self.zs, self.zt = zs, zt
        self.z_s, self.z_t = zs.expand(self.n, -1), zt.expand(self.n, -1)
        with torch.no_grad():
            self.z_f = render_rays(self.ro, self.rd, self.z_s, self.z_t, self.ps, self.emb, self.mc, self.mf,
                                   chunk_rows=CHUNK, coarse_rgb=False)["z_fine"]
        self.eps = ops.weight_cull_thresholds(self.tol, self.s)

    def fine_model(self, bias):
        m = copy.deepcopy(self.mf)
        m._packs = {}
        with torch.no_grad():
            m.fc_out.bias[0] += bias
        return m.eval()

    # the parts of the two-phase fine pass, as nerf._weight_culled_field runs them
    def density(self, m):
        from codenerf.nerf import _density_field_raw
        return _density_field_raw(m, self.emb, self.rd, self.z_s, self.z_t, CHUNK, ro=self.ro, z=self.z_f)

    def weights(self, raw):
        from codenerf import ops
        return ops.volume_render(raw, self.z_f, self.rd)[3]

    def cull(self, w):
        from codenerf import ops
        return ops.weight_cull(w, self.ro, self.rd, self.z_f, CHUNK, *self.eps, want_code=False)

    def field(self, m, kept):
        from codenerf.models.model import _field_op
        count, _, pts, vdir, _, _ = kept
        with torch.no_grad():
            return _field_op(m, self.zs, self.zt, vdir, count, self.emb[0].freqs, self.emb[1].freqs,
                             pts=pts.view(count, 1, 3))

    def plain_field(self, m):
        from codenerf.models.model import _field_op
        with torch.no_grad():
            return _field_op(m, self.zs, self.zt, self.rd, CHUNK, self.emb[0].freqs, self.emb[1].freqs, ro=self.ro,
                             z=self.z_f)

    def kept_fraction(self, m):
        """Measured: the share of this view's fine samples whose colours the two-phase pass computes."""
        with torch.no_grad():
            return self.cull(self.weights(self.density(m)))[0] / float(self.n * self.s)

    def models_at_targets(self):
        """name -> (fine model, its bias, its measured kept fraction): a bisection of the sigma bias per
        target; from the model as it is (bias 0, nearly every sample kept: the last sample of a ray takes
        whatever transmittance is left) the kept fraction falls as the bias grows and the transmittance
        dies sooner."""
        out = {}
        for target in TARGETS:
            lo, hi = 0.0, 2000.0             # kept(lo) is the most this sweep reaches
            if self.kept_fraction(self.fine_model(lo)) > target:
                for _ in range(20):
                    mid = 0.5 * (lo + hi)
                    if self.kept_fraction(self.fine_model(mid)) > target:
                        lo = mid
                    else:
                        hi = mid
            m = self.fine_model(lo)
            out[f"kept_{target:g}"] = (m, lo, self.kept_fraction(m))
        return out

    def render(self, m, **kw):
        from codenerf.nerf import render_rays
        with torch.no_grad():
            return render_rays(self.ro, self.rd, self.z_s, self.z_t, self.ps, self.emb, self.mc, m, chunk_rows=CHUNK,
                               coarse_rgb=False, **kw)

    def check(self, out, plain, name):
        """The claims of include/codenerf.h on one variant's result."""
        assert sorted(out) == sorted(plain), name
        for k in plain:
            if k == "rgb_fine":
                continue
            a, b = out[k], plain[k]
            same = torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
            assert same, f"{name}: {k} differs from the plain render's"
        err = (out["rgb_fine"] - plain["rgb_fine"]).abs().max().item()
        bound = 0.501 * self.tol + 2 * self.s * 2.0 ** -24
        assert err <= bound, f"{name}: rgb_fine is {err} from the plain render's, bound {bound}"
        return err


def versus(sp, base):
    return dict(sp, over_plain_median=sp["median_ms"] / base["median_ms"],
                beyond_spread=sp["max_ms"] < base["min_ms"] or sp["min_ms"] > base["max_ms"],
                faster_beyond_spread=sp["max_ms"] < base["min_ms"])


def step_render(dev, args, shape):
    sc = Scene(dev, args, shape)
    variants = sc.models_at_targets()
    if args.checkpoint:
        variants["checkpoint"] = (sc.mf, 0.0, sc.kept_fraction(sc.mf))
    lo, hi = 0.0, 2.0 * sc.bound             # the sphere grid that keeps about GRID_KEPT of the fine samples
    for _ in range(20):
        mid = 0.5 * (lo + hi)
        if kept_fraction(sphere_grid(dev, sc.bound, mid), sc.ro, sc.rd, sc.z_f) < GRID_KEPT:
            lo = mid
        else:
            hi = mid
    radius = hi
    grid = sphere_grid(dev, sc.bound, radius)
    grid_name = "kept_0.25"
    out, fns = {}, {}
    for name, (m, _, _) in variants.items():
        fns[f"{name}/plain"] = lambda name=name, m=m: out.__setitem__(f"{name}/plain", sc.render(m))
        fns[f"{name}/two_phase"] = lambda name=name, m=m: out.__setitem__(
            f"{name}/two_phase", sc.render(m, rgb_tolerance=sc.tol))
    mg = variants[grid_name][0]
    fns["grid/plain"] = lambda: out.__setitem__("grid/plain", sc.render(mg, occupancy=grid))
    fns["grid/two_phase"] = lambda: out.__setitem__("grid/two_phase", sc.render(mg, occupancy=grid, rgb_tolerance=sc.tol))
    ms = alternate(fns, args.reps)
    nc, nf = SHAPES[shape][:2]
    res = {"shape": {"rays": sc.n, "coarse": nc, "fine_pass_samples": sc.s, "chunk_rows": CHUNK, "coarse_rgb": False,
                     "fold": bool(sc.mf.fold), "rgb_tolerance": sc.tol, "eps_weight": sc.eps[0], "eps_tail": sc.eps[1]},
           "predicted_fine_cost_ratio": "(10 + 28 kept) / 28 of the plain fine pass, by weight chunks; a prediction",
           "bitwise_claims_hold": True, "variants": {}}
    for name, (m, bias, frac) in variants.items():
        base, sp = spread(ms[f"{name}/plain"]), spread(ms[f"{name}/two_phase"])
        err = sc.check(out[f"{name}/two_phase"], out[f"{name}/plain"], name)
        res["variants"][name] = {"sigma_bias": bias, "kept_fraction_fine": frac, "plain": dict(
            base, rays_per_s=sc.n / (base["median_ms"] * 1e-3)), "two_phase": dict(
            versus(sp, base), rays_per_s=sc.n / (sp["median_ms"] * 1e-3)), "rgb_fine_max_abs_diff": err,
            "predicted_fine_cost_ratio": (10 + 28 * frac) / 28}
    base, sp = spread(ms["grid/plain"]), spread(ms["grid/two_phase"])
    err = sc.check(out["grid/two_phase"], out["grid/plain"], "grid")
    z_f = out["grid/plain"]["z_fine"]
    res["with_grid"] = {"fine_model": grid_name, "grid": {"resolution": grid.resolution, "bound": grid.bound,
                                                          "radius": radius,
                                                          "kept_fraction_fine": kept_fraction(grid, sc.ro, sc.rd, z_f)},
                        "plain": base, "two_phase": versus(sp, base), "rgb_fine_max_abs_diff": err,
                        "grid_plain_over_ungridded_plain_median":
                            base["median_ms"] / res["variants"][grid_name]["plain"]["median_ms"]}
    res["break_even_kept_fraction_fine"] = break_even(
        [(v["kept_fraction_fine"], v["two_phase"]["median_ms"] - v["plain"]["median_ms"])
         for v in res["variants"].values()], 0.0)
    return res


def step_steps(dev, args):
    """The two-phase fine pass of c3 in its five calls, each timed alone on inputs held from a run of the
    ones before it, next to the plain fine field launch and the final volume_render both paths share."""
    from codenerf import ops
    sc = Scene(dev, args, "c3")
    variants = sc.models_at_targets()
    fns, held = {}, {}
    for name, (m, _, _) in variants.items():
        with torch.no_grad():
            raw = sc.density(m)
            w = sc.weights(raw)
            kept = sc.cull(w)
            rows = sc.field(m, kept) if kept[0] else None
        held[name] = (raw, w, kept, rows)
        fns[f"{name}/plain_field"] = lambda m=m: sc.plain_field(m)
        fns[f"{name}/density"] = lambda m=m: sc.density(m)
        fns[f"{name}/volume_render"] = lambda name=name: sc.weights(held[name][0])
        fns[f"{name}/cull_and_readback"] = lambda name=name: sc.cull(held[name][1])
        if kept[0]:
            fns[f"{name}/field_kept"] = lambda name=name, m=m: sc.field(m, held[name][2])
            fns[f"{name}/scatter"] = lambda name=name: ops.scatter_rgb(held[name][3], held[name][2][1], held[name][0])
    ms = alternate(fns, args.reps)
    res = {"shape": {"rays": sc.n, "fine_pass_samples": sc.s, "chunk_rows": CHUNK, "rgb_tolerance": sc.tol},
           "variants": {}}
    for name, (_, bias, frac) in variants.items():
        parts = {k.split("/", 1)[1]: spread(v) for k, v in ms.items() if k.startswith(name + "/")}
        two = sum(v["median_ms"] for k, v in parts.items() if k != "plain_field")
        res["variants"][name] = dict(parts, sigma_bias=bias, kept_fraction_fine=frac, kept_rows=held[name][2][0],
                                     sum_of_two_phase_medians_ms=two,
                                     sum_over_plain_field_median=two / parts["plain_field"]["median_ms"],
                                     field_kept_over_plain_field_median=(
                                         parts["field_kept"]["median_ms"] / parts["plain_field"]["median_ms"]
                                         if "field_kept" in parts else 0.0))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("c3", "chairs", "steps", "all"))
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each variant (>= 20)")
    ap.add_argument("--tol", type=float, default=1e-3, help="rgb_tolerance of the two-phase renders")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weightcull", "bench_weight_cull.json"))
    ap.add_argument("--checkpoint", help="a training checkpoint (.ckpt): its models and codes instead of the synthetic ones")
    ap.add_argument("--object", type=int, default=0, help="the checkpoint's object (code row) to render")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_weight_cull.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_weight_cull.py: no HIP device -- this benchmark has no CPU fallback")
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    steps = {"c3": lambda: step_render(dev, args, "c3"), "chairs": lambda: step_render(dev, args, "chairs"),
             "steps": lambda: step_steps(dev, args)}
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
