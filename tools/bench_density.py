"""Measure the density-only field kernel against the full field kernel, and the renders and the
density grid built on it.  Needs an MI355X: there is no CPU fallback.

    python tools/bench_density.py [--step kernel|c3|chairs|grid|all] [--reps 30] [--out PATH]

Each step merges its section into the JSON at --out (default profiles/density/bench_density.json),
so the steps can run as separate commands, each under its own time limit.  All times are device
events around one call; the two variants of a comparison alternate inside one process after a
warm-up of both, and every figure carries its spread (min / median / max over the repetitions).
TFLOP/s are algorithmic: the FLOP the layers need per sample (163,840 density, 572,416 full field)
over the launch's event time, and "of_peak" is that over the 157.3 TFLOP/s fp32 matrix peak.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-nerf_amd"))
import torch  # noqa: E402

FLOP_DENSITY = 2 * (63 * 256 + 256 * 256 + 256)     # layer_xyz1, layer_xyz2, fc_out row 0
FLOP_FIELD = 572_416                                 # the whole hoisted CodeNeRF MLP (bench.py)
PEAK_FP32_MFMA_TFLOPS = 157.3
H = W = 128
FOCAL = 131.25
FX = [2.0 ** k for k in range(10)]
FD = [2.0 ** k for k in range(4)]


def spread(ms):
    ms = sorted(ms)
    return {"min_ms": ms[0], "median_ms": ms[len(ms) // 2], "max_ms": ms[-1], "reps": len(ms)}


def separated(fast, slow):
    """The difference exceeds the measured spread: every repetition of ``fast`` beat every one of ``slow``."""
    return fast["max_ms"] < slow["min_ms"]


def alternate(fns, reps, warmup=3):
    """Time the callables of ``fns`` (name -> fn) alternating, ``reps`` times each -> name -> [ms]."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}


def pose(theta, phi, rho):
    """eval.py:22-38 pose_spherical (host, float32), as bench.py."""
    st, ct, sp, cp = math.sin(theta), math.cos(theta), math.sin(phi), math.cos(phi)
    m = torch.eye(4)
    m[0, 0], m[1, 0] = -sp, cp
    m[0, 1], m[1, 1], m[2, 1] = -st * cp, -st * sp, ct
    m[0, 2], m[1, 2], m[2, 2] = ct * cp, ct * sp, st
    m[0, 3], m[1, 3], m[2, 3] = rho * ct * cp, rho * ct * sp, rho * st
    return m


def setup(dev):
    from codenerf import synthetic
    from codenerf.models import CodeNeRFModel
    from codenerf.nerf import PositionalEmbedder
    models = []
    for seed in (0, 1):
        m = CodeNeRFModel(256, 1, 256, 256, 10, 4)
        m.load_state_dict(synthetic.codenerf_params(seed))
        models.append(m.to(dev).eval())
    emb = (PositionalEmbedder(10, True, True, torch.float32, dev), PositionalEmbedder(4, True, True, torch.float32, dev))
    return models, emb, synthetic.latent_codes(5, 1).to(dev), synthetic.latent_codes(6, 1).to(dev)


def view_rays(dev, rho):
    from codenerf import synthetic
    from codenerf.nerf import RaySampler
    rs = RaySampler(H, W, synthetic.srn_intrinsics(H, FOCAL), sample_size=4096, device=dev, datatype=torch.float32)
    ro, rd = rs.get_bundle(pose(0.5, 0.9, rho)[None].to(dev))
    return ro.reshape(-1, 3), rd.reshape(-1, 3)


def step_kernel(dev, reps):
    """The C2 coarse launch (16,384 rays x 64 samples, rays and depths, one code): density vs full field."""
    from codenerf import ops
    from codenerf.nerf import PointSampler
    (mc, _), _, zs, zt = setup(dev)
    ro, rd = view_rays(dev, 1.3)
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    _, z = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
    n, s = z.shape
    packed, cb = mc.packed(), mc.code_bias(zs, zt)
    out = {}
    fns = {"full_field": lambda: out.__setitem__("full", ops.radiance_field(packed, cb, rd, s, 4096, FX, FD, ro=ro, z=z,
                                                                            precision="f32_w16")),
           "density": lambda: out.__setitem__("sig", ops.density_field(packed, cb, FX, ro=ro, rd=rd, z=z))}
    ms = alternate(fns, reps)
    assert torch.equal(out["sig"], out["full"][..., 3]), "density kernel's sigma differs from the full field's"
    res = {"shape": {"rays": n, "samples": s, "mode": "ro, rd, z", "codes": 1}, "sigma_bit_equal": True}
    for k, flop in (("full_field", FLOP_FIELD), ("density", FLOP_DENSITY)):
        sp = spread(ms[k])
        tf = n * s * flop / (sp["median_ms"] * 1e-3) / 1e12
        res[k] = dict(sp, flop_per_sample=flop, tflops=tf, of_fp32_mfma_peak=tf / PEAK_FP32_MFMA_TFLOPS)
    res["time_ratio_median"] = res["density"]["median_ms"] / res["full_field"]["median_ms"]
    res["flop_ratio"] = FLOP_DENSITY / FLOP_FIELD
    res["density_faster_beyond_spread"] = separated(res["density"], res["full_field"])
    assert res["density_faster_beyond_spread"], res
    return res


def step_render(dev, reps, nc, nf, near, far, rho):
    """One 128 x 128 view, chunk 4096, unperturbed: render_rays with coarse_rgb True / False alternating."""
    from codenerf.nerf import PointSampler, render_rays
    (mc, mf), emb, zs, zt = setup(dev)
    ro, rd = view_rays(dev, rho)
    n = ro.shape[0]
    ps = PointSampler(nc, nf, near, far, "lindepth", False, torch.float32, dev)
    z_s, z_t = zs.expand(n, -1), zt.expand(n, -1)
    out = {}

    def render(key, coarse_rgb):
        with torch.no_grad():
            out[key] = render_rays(ro, rd, z_s, z_t, ps, emb, mc, mf, chunk_rows=4096, coarse_rgb=coarse_rgb)["rgb_fine"]

    ms = alternate({"coarse_rgb": lambda: render("a", True), "coarse_density": lambda: render("b", False)}, reps)
    assert torch.equal(out["a"], out["b"]), "rgb_fine differs between coarse_rgb=True and False"
    res = {"shape": {"rays": n, "coarse": nc, "fine_pass_samples": nc + nf, "chunk_rows": 4096}, "rgb_fine_bit_equal": True}
    for k in ("coarse_rgb", "coarse_density"):
        sp = spread(ms[k])
        res[k] = dict(sp, rays_per_s=n / (sp["median_ms"] * 1e-3))
    res["speedup_median"] = res["coarse_rgb"]["median_ms"] / res["coarse_density"]["median_ms"]
    res["flop_ratio"] = (nc * FLOP_FIELD + (nc + nf) * FLOP_FIELD) / (nc * FLOP_DENSITY + (nc + nf) * FLOP_FIELD)
    res["density_faster_beyond_spread"] = separated(res["coarse_density"], res["coarse_rgb"])
    return res


def step_grid(dev, reps):
    from codenerf.nerf import density_grid
    (mc, _), emb, zs, _ = setup(dev)
    d = 128
    ms = alternate({"grid": lambda: density_grid(mc, emb, zs, d, 1.0)}, reps)["grid"]
    sp = spread(ms)
    return dict(sp, resolution=d, points=d ** 3, points_per_s=d ** 3 / (sp["median_ms"] * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("kernel", "c3", "chairs", "grid", "all"))
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each variant (>= 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density", "bench_density.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_density.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_density.py: no HIP device -- this benchmark has no CPU fallback")
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    steps = {"kernel": lambda: step_kernel(dev, args.reps),
             "c3": lambda: step_render(dev, args.reps, 64, 64, 0.8, 1.8, 1.3),
             "chairs": lambda: step_render(dev, args.reps, 32, 128, 1.25, 2.75, 2.0),
             "grid": lambda: step_grid(dev, args.reps)}
    results = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results["device"] = torch.cuda.get_device_name(0)
    results["library"] = codenerf.build_info()["version"]
    for name in (steps if args.step == "all" else [args.step]):
        results[name] = steps[name]()
        print(json.dumps({name: results[name]}))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")
    if "c3" in results and args.step in ("c3", "all"):
        assert results["c3"]["density_faster_beyond_spread"], results["c3"]


if __name__ == "__main__":
    main()
