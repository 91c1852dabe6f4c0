"""Measure the fp16 inference field kernel (precision "f16") against the fp32 (folded) and 3xbf16 kernels.
Needs an MI355X: there is no CPU fallback.

    python tools/bench_f16.py [--step launch|render|scene|accuracy|all] [--reps 30] [--out PATH]

Each step merges its section into the JSON at --out (default profiles/f16/bench_f16.json), so the steps can run
as separate commands.  All times are device events around one call; the variants of a comparison alternate
inside one process after a warm-up of all, and every figure carries its spread (min / median / max over the
repetitions).  TFLOP/s are algorithmic: 572,416 FLOP per sample (the unfolded MLP; the folded fp32 kernel
computes 441,344 of them) over the launch's event time; "of_f16_peak" is that over the 2516.6 TFLOP/s dense
f16 matrix peak.  The models are synthetic (no trained checkpoint exists here): the accuracy figures hold for
the trained-magnitude weight sets "t4" and "t3", not for a trained model.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_density import FD, FX, alternate, pose, separated, spread  # noqa: E402

FLOP_FIELD = 572_416
PEAK_F16_MFMA_TFLOPS = 2516.6
PRECISIONS = ("f32", "bf16x3", "f16")
H = W = 128
FOCAL = 131.25


def make_models(dev, precision, weights="synthetic"):
    from codenerf import synthetic
    from codenerf.models import CodeNeRFModel
    out = []
    for seed in (0, 1):
        m = CodeNeRFModel(256, 1, 256, 256, 10, 4)
        if weights == "synthetic":
            m.load_state_dict(synthetic.codenerf_params(seed))
        else:
            m.load_state_dict(synthetic.trained_params(seed + 1, weights))
        m.precision = precision
        out.append(m.to(dev).eval())
    return out


def embedders(dev):
    from codenerf.nerf import PositionalEmbedder
    return PositionalEmbedder(10, True, True, torch.float32, dev), PositionalEmbedder(4, True, True, torch.float32, dev)


def codes(dev, weights="synthetic"):
    from codenerf import synthetic
    if weights == "synthetic":
        return synthetic.latent_codes(5, 1).to(dev), synthetic.latent_codes(6, 1).to(dev)
    return synthetic.trained_codes(5, 1, weights).to(dev), synthetic.trained_codes(6, 1, weights).to(dev)


def view_rays(dev, n_views, rho=1.3):
    from codenerf import synthetic
    from codenerf.nerf import RaySampler
    rs = RaySampler(H, W, synthetic.srn_intrinsics(H, FOCAL), sample_size=4096, device=dev, datatype=torch.float32)
    ros, rds = [], []
    for v in range(n_views):
        ro, rd = rs.get_bundle(pose(0.5, 0.9 + 0.39 * v, rho)[None].to(dev))
        ros.append(ro.reshape(-1, 3))
        rds.append(rd.reshape(-1, 3))
    return torch.cat(ros).contiguous(), torch.cat(rds).contiguous()


def step_launch(dev, reps):
    """The headline coarse launch: 16 views x 128^2 rays x 64 samples, rays and depths, one code."""
    from codenerf import ops
    from codenerf.models.model import inference_pack
    from codenerf.nerf import PointSampler
    ro, rd = view_rays(dev, 16)
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    _, z = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
    n, s = z.shape
    zs, zt = codes(dev)
    fns, out = {}, {}
    for p in PRECISIONS:
        m = make_models(dev, p)[0]
        cb = m.code_bias(zs, zt)
        packed, fmt, fold = inference_pack(m, cb)

        def run(p=p, packed=packed, fmt=fmt, fold=fold, cb=cb):
            out[p] = ops.radiance_field(packed, cb, rd, s, 4096, FX, FD, ro=ro, z=z, precision=fmt, fold_bias=fold)
        fns[p] = run
    ms = alternate(fns, reps)
    res = {"shape": {"rays": n, "samples": s, "mode": "ro, rd, z", "codes": 1, "chunk_rows": 4096}}
    for p in PRECISIONS:
        sp = spread(ms[p])
        tf = n * s * FLOP_FIELD / (sp["median_ms"] * 1e-3) / 1e12
        res[p] = dict(sp, rays_per_s=n / (sp["median_ms"] * 1e-3), tflops=tf)
    res["f16"]["of_f16_peak"] = res["f16"]["tflops"] / PEAK_F16_MFMA_TFLOPS
    res["f16_over_bf16x3_median"] = res["f16"]["median_ms"] / res["bf16x3"]["median_ms"]
    res["f16_over_f32_median"] = res["f16"]["median_ms"] / res["f32"]["median_ms"]
    res["f16_faster_than_bf16x3_beyond_spread"] = separated(res["f16"], res["bf16x3"])
    d = (out["f16"] - out["f32"]).abs()
    res["raw_rgb_abs_diff_vs_f32"] = {"max": float(d[..., :3].max()), "mean": float(d[..., :3].mean())}
    assert res["f16_faster_than_bf16x3_beyond_spread"], res
    return res


def render_fn(dev, precision, ro, rd, zs, zt, ps, emb, out, weights="synthetic"):
    from codenerf.nerf import render_rays
    mc, mf = make_models(dev, precision, weights)
    n = ro.shape[0]
    z_s, z_t = zs.expand(n, -1), zt.expand(n, -1)

    def run():
        with torch.no_grad():
            out[precision] = render_rays(ro, rd, z_s, z_t, ps, emb, mc, mf, chunk_rows=4096)["rgb_fine"]
    return run


def step_render(dev, reps):
    """One 128 x 128 view, 64 + 64 samples, chunk 4096, unperturbed: render_rays per precision."""
    from codenerf.nerf import PointSampler
    ro, rd = view_rays(dev, 1)
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    zs, zt = codes(dev)
    out = {}
    fns = {p: render_fn(dev, p, ro, rd, zs, zt, ps, embedders(dev), out) for p in PRECISIONS}
    ms = alternate(fns, reps)
    res = {"shape": {"rays": ro.shape[0], "coarse": 64, "fine_pass_samples": 128, "chunk_rows": 4096}}
    for p in PRECISIONS:
        sp = spread(ms[p])
        res[p] = dict(sp, rays_per_s=ro.shape[0] / (sp["median_ms"] * 1e-3))
    res["f16_over_bf16x3_median"] = res["f16"]["median_ms"] / res["bf16x3"]["median_ms"]
    res["f16_faster_than_bf16x3_beyond_spread"] = separated(res["f16"], res["bf16x3"])
    d = (out["f16"] - out["f32"]).abs()
    res["rgb_fine_abs_diff_vs_f32"] = {"max": float(d.max()), "mean": float(d.mean())}
    return res


def step_scene(dev, reps):
    """A four-object render_scene (128 x 128, 64 + 64): cube grids of half-width 0.5, fp32 and f16 models."""
    from codenerf import synthetic
    from codenerf.nerf import OccupancyGrid, PointSampler, SceneObject, render_scene
    ro, rd = view_rays(dev, 1, rho=2.0)
    ps = PointSampler(64, 64, 1.0, 3.0, "lindepth", False, torch.float32, dev)
    grid = OccupancyGrid.full(32, 0.5, dev)
    objects = [SceneObject(synthetic.latent_codes(20 + k, 1).to(dev), synthetic.latent_codes(30 + k, 1).to(dev), grid,
                           translation=t) for k, t in enumerate(((-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (-0.5, 0.5, 0.0),
                                                                 (0.5, 0.5, 0.0)))]
    emb, out, fns = embedders(dev), {}, {}
    for p in ("f32", "f16"):
        mc, mf = make_models(dev, p)

        def run(p=p, mc=mc, mf=mf):
            with torch.no_grad():
                out[p] = render_scene(ro, rd, objects, ps, emb, mc, mf)["rgb_fine"]
        fns[p] = run
    ms = alternate(fns, reps)
    res = {"shape": {"rays": ro.shape[0], "objects": 4, "coarse": 64, "fine_pass_samples": 128}}
    for p in fns:
        sp = spread(ms[p])
        res[p] = dict(sp, rays_per_s=ro.shape[0] / (sp["median_ms"] * 1e-3))
    res["f16_over_f32_median"] = res["f16"]["median_ms"] / res["f32"]["median_ms"]
    d = (out["f16"] - out["f32"]).abs()
    res["rgb_fine_abs_diff_vs_f32"] = {"max": float(d.max()), "mean": float(d.mean())}
    return res


def step_accuracy(dev):
    """|rgb_fine - the fp32 render's| of the 128 x 128, 64 + 64 render on the trained-magnitude weight sets."""
    from codenerf.nerf import PointSampler
    ro, rd = view_rays(dev, 1)
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    res = {"note": "synthetic trained-magnitude weights; no trained checkpoint exists here"}
    for weights in ("t4", "t3"):
        zs, zt = codes(dev, weights)
        out = {}
        for p in ("f32", "f16"):
            render_fn(dev, p, ro, rd, zs, zt, ps, embedders(dev), out, weights)()
        d = (out["f16"] - out["f32"]).abs()
        res[weights] = {"max": float(d.max()), "mean": float(d.mean()), "eight_bit_step": 1.0 / 255.0}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("launch", "render", "scene", "accuracy", "all"))
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each variant (>= 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16", "bench_f16.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_f16.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_f16.py: no HIP device -- this benchmark has no CPU fallback")
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    steps = {"launch": lambda: step_launch(dev, args.reps), "render": lambda: step_render(dev, args.reps),
             "scene": lambda: step_scene(dev, args.reps), "accuracy": lambda: step_accuracy(dev)}
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


if __name__ == "__main__":
    main()
