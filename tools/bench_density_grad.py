"""Measure the density-gradient kernel against the composed path it replaces (the field forward writing
ReLU masks, then the whole fused backward on d_raw = (0, 0, 0, 1)) and against the density kernel (the
forward-only floor), and the render and the mesh extraction built on it.  Needs an MI355X: there is no
CPU fallback.

    python tools/bench_density_grad.py [--step points|rays|render|mesh|all] [--reps 30] [--out PATH]

Each step merges its section into the JSON at --out (default profiles/densitygrad/bench_density_grad.json),
so the steps can run as separate commands, each under its own time limit.  All times are device events
around one call; the variants of a comparison alternate inside one process after a warm-up of all of
them, and every figure carries its spread (min / median / max over the repetitions).  TFLOP/s are
algorithmic: 327,680 FLOP per sample (the density's 163,840 forward and as many backward) over the
launch's event time, "of_peak" that over the 157.3 TFLOP/s fp32 matrix peak.  The composed path needs
2 x 572,416 FLOP per sample, so the FLOP ceiling of the time ratio is 0.286.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-nerf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_density import FD, FX, PEAK_FP32_MFMA_TFLOPS, alternate, separated, setup, spread, view_rays  # noqa: E402

FLOP_DENSITY = 2 * (63 * 256 + 256 * 256 + 256)
FLOP_GRAD = 2 * FLOP_DENSITY
FLOP_FIELD = 572_416
FLOP_CEILING = FLOP_GRAD / (2 * FLOP_FIELD)


def same_values(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def compare(dev, reps, geo, n, s):
    """The three launches on one geometry (points (n, s, 3), or rays + depths), one code row."""
    from codenerf import ops
    (mc, _), _, zs, zt = setup(dev)
    packed, packed_t = mc.packed(), mc.packed("f32_w16_t")
    cb = mc.code_bias(zs, zt)
    rd = geo["rd"] if "rd" in geo else torch.tensor([0.0, 0.0, 1.0], device=dev).expand(n, 3).contiguous()
    fgeo = {k: v for k, v in geo.items() if k != "rd"}
    d_raw = torch.zeros(n, s, 4, device=dev)
    d_raw[..., 3] = 1.0
    out = {}

    def composed(fgeo=fgeo):
        raw, masks = ops.radiance_field_masks(packed, cb, rd, s, n, FX, FD, precision="f32", **fgeo)
        rays = "ro" in fgeo
        out["composed"] = (raw, ops.field_backward_x3(packed_t, masks, d_raw, n, s, n, 1, FX, FD, rd, want_pts=not rays,
                                                      want_ro=rays, want_rd=rays, precision="f32", **fgeo))

    fns = {"density_gradient": lambda: out.__setitem__("grad", ops.density_gradient(packed, packed_t, cb, FX, **geo)),
           "composed_path": composed,
           "density_field": lambda: out.__setitem__("sig", ops.density_field(packed, cb, FX, **geo))}
    ms = alternate(fns, reps)
    grad = out["grad"]
    raw, bwd = out["composed"]
    # the equalities of tests/test_gpu_density_grad.py (a, b): sigma bits, gradient values
    assert torch.equal(grad[..., 3], out["sig"]) and torch.equal(grad[..., 3], raw[..., 3]), "sigma bits differ"
    res = {"shape": dict(rays=n, samples=s, mode=", ".join(geo), codes=1), "sigma_bit_equal": True}
    if "ro" in geo:
        # from rays the composed path returns d ro / d rd, not d_pts: the equality is taken (untimed) on the
        # points the kernels form, pts = ro + rd z with each operation rounded
        composed(dict(pts=geo["ro"][:, None, :] + geo["rd"][:, None, :] * geo["z"][..., None]))
        raw, bwd = out["composed"]
        assert torch.equal(grad[..., 3], raw[..., 3]), "sigma bits differ"
    assert same_values(grad[..., :3], bwd["d_pts"]), "gradient differs from the composed path's d_pts"
    res["gradient_equals_composed_d_pts"] = True
    for k, flop in (("density_gradient", FLOP_GRAD), ("composed_path", 2 * FLOP_FIELD), ("density_field", FLOP_DENSITY)):
        sp = spread(ms[k])
        tf = n * s * flop / (sp["median_ms"] * 1e-3) / 1e12
        res[k] = dict(sp, flop_per_sample=flop, tflops=tf, of_fp32_mfma_peak=tf / PEAK_FP32_MFMA_TFLOPS)
    res["time_ratio_vs_composed_median"] = res["density_gradient"]["median_ms"] / res["composed_path"]["median_ms"]
    res["flop_ceiling_vs_composed"] = FLOP_CEILING
    res["time_ratio_vs_density_field_median"] = res["density_gradient"]["median_ms"] / res["density_field"]["median_ms"]
    res["faster_than_composed_beyond_spread"] = separated(res["density_gradient"], res["composed_path"])
    assert res["faster_than_composed_beyond_spread"], res
    return res


def step_points(dev, reps):
    """2^21 points, one sample per row."""
    n = 1 << 21
    pts = torch.randn(n, 1, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    return compare(dev, reps, dict(pts=pts), n, 1)


def step_rays(dev, reps):
    """The 16,384 x 64 ray shape (one 128 x 128 view's coarse depths)."""
    from codenerf import ops
    from codenerf.nerf import PointSampler
    ro, rd = view_rays(dev, 1.3)
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    _, z = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
    return compare(dev, reps, dict(ro=ro, rd=rd, z=z), z.shape[0], z.shape[1])


def step_render(dev, reps):
    """One 128 x 128 view, 64 + 64 samples, chunk 4096, unperturbed: render_rays with and without normals."""
    from codenerf.nerf import PointSampler, render_rays
    (mc, mf), emb, zs, zt = setup(dev)
    ro, rd = view_rays(dev, 1.3)
    n = ro.shape[0]
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    z_s, z_t = zs.expand(n, -1), zt.expand(n, -1)
    out = {}

    def render(key, normals):
        with torch.no_grad():
            out[key] = render_rays(ro, rd, z_s, z_t, ps, emb, mc, mf, chunk_rows=4096, normals=normals)

    ms = alternate({"plain": lambda: render("a", False), "normals": lambda: render("b", True)}, reps)
    for k, t in out["a"].items():
        assert torch.equal(out["b"][k], t), k
    nf = out["b"]["normal_fine"]
    assert nf.shape == (n, 3) and bool((torch.linalg.vector_norm(nf, dim=-1) <= out["b"]["acc_fine"] + 1e-5).all())
    res = {"shape": {"rays": n, "coarse": 64, "fine_pass_samples": 128, "chunk_rows": 4096},
           "other_entries_bit_equal": True}
    for k in ("plain", "normals"):
        sp = spread(ms[k])
        res[k] = dict(sp, rays_per_s=n / (sp["median_ms"] * 1e-3))
    res["cost_of_normals_median"] = res["normals"]["median_ms"] / res["plain"]["median_ms"]
    res["flop_ratio"] = (192 * FLOP_FIELD + 128 * FLOP_GRAD) / (192 * FLOP_FIELD)
    return res


def step_mesh(dev, reps):
    """extract_mesh at 129^3 nodes with and without vertex normals + colours."""
    from codenerf.nerf import density_grid, extract_mesh
    (mc, _), emb, zs, zt = setup(dev)
    d = 129
    level = float(density_grid(mc, emb, zs, 33, 1.0).median())
    out = {}
    fns = {"plain": lambda: out.__setitem__("a", extract_mesh(mc, emb, zs, d, 1.0, level)),
           "normals_colors": lambda: out.__setitem__("b", extract_mesh(mc, emb, zs, d, 1.0, level, normals=True,
                                                                       colors=True, z_t=zt))}
    ms = alternate(fns, reps)
    a, b = out["a"], out["b"]
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)
    res = {"resolution": d, "level": level, "vertices": a.n_vertices, "faces": a.n_faces}
    for k in fns:
        res[k] = spread(ms[k])
    res["cost_of_attributes_median"] = res["normals_colors"]["median_ms"] / res["plain"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("points", "rays", "render", "mesh", "all"))
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each variant (>= 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densitygrad", "bench_density_grad.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_density_grad.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_density_grad.py: no HIP device -- this benchmark has no CPU fallback")
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    steps = {"points": step_points, "rays": step_rays, "render": step_render, "mesh": step_mesh}
    results = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results["device"] = torch.cuda.get_device_name(0)
    results["library"] = codenerf.build_info()["version"]
    for name in (steps if args.step == "all" else [args.step]):
        results[name] = steps[name](dev, args.reps)
        print(json.dumps({name: results[name]}))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
