"""Measure the scene render's backward: the four backward launches around the compact fields, and one fitting
step of render_scene_autograd against single-object steps, in one process.  Needs an MI355X: there is no CPU
fallback.

    python tools/bench_scene_grad.py [--step compose|rays|cull|fit|all] [--reps 30] [--out PATH]

Each step merges its section into the JSON at --out (default profiles/scenegrad/bench_scene_grad.json).  All
times are device events around one call; the variants of a step alternate inside one process after a warm-up of
all of them, and every figure carries its spread (min / median / max over the repetitions).  Every launch's
algorithmic bytes are given beside the 5.86 TB/s the read probe (tools/read_probe.hip) reaches on this part.

``compose``: cn_volume_render_compose_backward at 16,384 rays x 192 samples with all six upstream gradients, for
K = 1 beside cn_volume_render_backward on the same tensor (the same gradients without the masks') and for K = 8
(about half of each object's slots empty, as after a cull).  Bytes per ray: 12 + 4 S + 32 K S (the rows are
staged twice) + 4 S + 24 + 4 K in, 16 K S + 12 out.
``rays``: cn_object_rays_backward at 16,384 rays, K = 1 and 8, every output (two launches).
``cull``: cn_occupancy_gather and cn_occupancy_cull_backward at 16,384 rays x 192 samples under a sphere grid.
``fit``: 2,048 rays of one view, 64 + 64 samples, unperturbed, four copies of one synthetic object translated
along a line under sphere grids (radius 0.4, G = 128): one step = render_scene_autograd + an MSE loss on
rgb_coarse / rgb_fine against a fixed target + backward + Adam (torch.optim) on the four objects' codes and
their 6-number poses (rigid_pose).  Beside it, four single-object steps on the same rays: render_rays on the
object's own rays with gradients to its codes and rays, the same loss, backward, Adam on the codes.  The four
single-object steps do not compute the same image where the objects overlap on a ray and fit no pose.
The models are the synthetic ones: no trained checkpoint ships with the repository, so the share of samples a
trained object's grid would keep -- which sizes every compact field launch -- is not measured here.
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

RAYS, SAMPLES = 16384, 192
READ_PROBE_TB_S = 5.86
EMPTY_ROW = (0.0, 0.0, 0.0, -1.0e4)


def rated(sp, nbytes, **extra):
    tb_s = nbytes / (sp["median_ms"] * 1e-3) / 1e12
    return dict(sp, bytes=nbytes, tb_per_s=tb_s, of_read_probe=tb_s / READ_PROBE_TB_S, **extra)


def compose_backward_bytes(n, s, k):
    return n * (12 + 4 * s + 32 * k * s + 4 * s + 24 + 4 * k + 16 * k * s + 12)


def step_compose(dev, reps):
    from codenerf import ops
    n, s = RAYS, SAMPLES
    g = torch.Generator().manual_seed(s)
    z = torch.sort(1 + torch.rand(n, s, generator=g), -1).values.to(dev)
    rd = torch.randn(n, 3, generator=g).to(dev)
    dense = (torch.randn(n, s, 4, generator=g) * 2).to(dev)
    raws = []
    for _ in range(8):
        raw = torch.randn(n, s, 4, generator=g) * 2
        raw[torch.rand(n, s, generator=g) < 0.5] = torch.tensor(EMPTY_ROW)
        raws.append(raw.to(dev))
    up = dict(g_rgb=torch.randn(n, 3, generator=g).to(dev), g_disp=(1e-2 * torch.randn(n, generator=g)).to(dev),
              g_acc=torch.randn(n, generator=g).to(dev), g_weights=torch.randn(n, s, generator=g).to(dev),
              g_depth=torch.randn(n, generator=g).to(dev))
    g_ao = torch.randn(8, n, generator=g).to(dev)
    out = {}
    fns = {"volume_render_backward": lambda: out.__setitem__("plain", ops.volume_render_backward(dense, z, rd, **up)),
           "compose_backward_k1": lambda: out.__setitem__(1, ops.volume_render_compose_backward([dense], z, rd, **up)),
           "compose_backward_k8": lambda: out.__setitem__(8, ops.volume_render_compose_backward(
               raws, z, rd, g_acc_objects=g_ao, **up))}
    ms = alternate(fns, reps)
    assert torch.equal(out[1][0][0], out["plain"][0]) and torch.equal(out[1][1], out["plain"][1]), \
        "one composed object's gradients differ from cn_volume_render_backward's"
    plain_bytes = n * (12 + 4 * s + 16 * s + 4 * s + 24 + 16 * s + 12)
    sec = {"volume_render_backward": rated(spread(ms["volume_render_backward"]), plain_bytes, objects=1),
           "compose_backward_k1": rated(spread(ms["compose_backward_k1"]), compose_backward_bytes(n, s, 1) - 4 * n,
                                        objects=1),
           "compose_backward_k8": rated(spread(ms["compose_backward_k8"]), compose_backward_bytes(n, s, 8), objects=8)}
    a, b = sec["compose_backward_k1"], sec["volume_render_backward"]
    sec["k1_over_volume_render_backward_median"] = a["median_ms"] / b["median_ms"]
    sec["k1_bit_equal_to_volume_render_backward"] = True
    return {"shape": {"rays": n, "samples": s}, "launches": sec}


def step_rays(dev, reps):
    from codenerf import ops
    n = RAYS
    g = torch.Generator().manual_seed(7)
    ro, rd = torch.randn(n, 3, generator=g).to(dev), torch.randn(n, 3, generator=g).to(dev)
    sec = {}
    fns, out = {}, {}
    for k in (1, 8):
        g_ro, g_rd = torch.randn(k, n, 3, generator=g).to(dev), torch.randn(k, n, 3, generator=g).to(dev)
        poses = [[1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0.1 * j, 0.0, -0.1 * j] for j in range(k)]
        fns[f"object_rays_backward_k{k}"] = lambda k=k, a=(g_ro, g_rd, ro, rd, poses): out.__setitem__(
            k, ops.object_rays_backward(*a))
    ms = alternate(fns, reps)
    for k in (1, 8):
        # the pose pass reads the rays and the gradients a second time
        sec[f"object_rays_backward_k{k}"] = rated(spread(ms[f"object_rays_backward_k{k}"]),
                                                  n * (2 * (24 * k + 24) + 24) + 48 * k, objects=k, launches=2)
    return {"shape": {"rays": n}, "launches": sec}


def step_cull(dev, reps):
    from codenerf import ops
    from codenerf.nerf import PointSampler
    n, s = RAYS, SAMPLES
    ro, rd = view_rays(dev, 1.3)
    assert ro.shape[0] == n
    ps = PointSampler(s, 1, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    _, z = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
    grid = sphere_grid(dev, 1.0, 0.4)
    count, _, _, _, _, state = ops.occupancy_cull(ro, rd, z, n, grid.bits, grid.resolution, grid.bound, want_code=False)
    g = torch.Generator().manual_seed(9)
    g_raw = torch.randn(n, s, 4, generator=g).to(dev)
    g_pts, g_vdir = torch.randn(count, 3, generator=g).to(dev), torch.randn(count, 3, generator=g).to(dev)
    out = {}
    fns = {"occupancy_gather": lambda: out.__setitem__("g", ops.occupancy_gather(g_raw, state)),
           "occupancy_cull_backward": lambda: out.__setitem__("c", ops.occupancy_cull_backward(g_pts, g_vdir, z, n, state))}
    ms = alternate(fns, reps)
    words = (s + 63) // 64
    sec = {"occupancy_gather": rated(spread(ms["occupancy_gather"]), 32 * count + n * (4 + 8 * words)),
           "occupancy_cull_backward": rated(spread(ms["occupancy_cull_backward"]),
                                            count * (24 + 4) + n * (24 + 4 + 8 * words))}
    return {"shape": {"rays": n, "samples": s, "kept_rows": count, "kept_fraction": count / (n * s), "grid": G,
                      "sphere_radius": 0.4}, "launches": sec}


def step_fit(dev, reps):
    from codenerf.nerf import PointSampler, SceneObject, render_rays, render_scene_autograd, rigid_pose
    (mc, mf), emb, zs, zt = setup(dev)
    for m in (mc, mf):
        m.requires_grad_(False)
    ro, rd = view_rays(dev, 1.3)
    ro, rd = ro[::8].contiguous(), rd[::8].contiguous()
    n = ro.shape[0]
    ps = PointSampler(64, 64, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    grid = sphere_grid(dev, 1.0, 0.4)
    k = 4
    shifts = [[0.0, 0.0, 0.35 * (j - (k - 1) / 2)] for j in range(k)]
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(3)).to(dev)

    codes = [(zs.clone().requires_grad_(True), zt.clone().requires_grad_(True)) for _ in range(k)]
    omegas = [torch.zeros(3, device=dev, requires_grad=True) for _ in range(k)]
    trans = [torch.tensor(t, device=dev, requires_grad=True) for t in shifts]
    objects = [SceneObject(a, b, grid) for a, b in codes]
    scene_opt = torch.optim.Adam([t for pair in codes for t in pair] + omegas + trans, lr=1e-4)
    kept = {}

    def scene_step():
        scene_opt.zero_grad(set_to_none=True)
        poses = torch.stack([rigid_pose(w, t) for w, t in zip(omegas, trans)])
        out = render_scene_autograd(ro, rd, objects, ps, emb, mc, mf, poses=poses)
        loss = ((out["rgb_coarse"] - target) ** 2).mean() + ((out["rgb_fine"] - target) ** 2).mean()
        loss.backward()
        scene_opt.step()
        kept["acc"] = out["acc_fine"].detach()

    single = [(zs.clone().requires_grad_(True), zt.clone().requires_grad_(True)) for _ in range(k)]
    single_opt = [torch.optim.Adam(list(pair), lr=1e-4) for pair in single]
    rays = [((ro - torch.tensor(t, device=dev)).requires_grad_(True), rd.clone().requires_grad_(True)) for t in shifts]

    def single_steps():
        for (a, b), opt, (o, d) in zip(single, single_opt, rays):
            opt.zero_grad(set_to_none=True)
            o.grad = d.grad = None
            out = render_rays(o, d, a.expand(n, -1), b.expand(n, -1), ps, emb, mc, mf, chunk_rows=None)
            loss = ((out["rgb_coarse"] - target) ** 2).mean() + ((out["rgb_fine"] - target) ** 2).mean()
            loss.backward()
            opt.step()

    ms = alternate({"scene_fit_step": scene_step, "four_single_object_steps": single_steps}, reps)
    a, b = spread(ms["scene_fit_step"]), spread(ms["four_single_object_steps"])
    return {"shape": {"rays": n, "coarse": 64, "fine_pass_samples": 128, "objects": k, "grid": G, "sphere_radius": 0.4,
                      "translations": shifts, "occupied_fraction": grid.occupied_fraction()},
            "scene_fit_step": dict(a, rays_per_s=n / (a["median_ms"] * 1e-3)),
            "four_single_object_steps": dict(b, rays_per_s=n / (b["median_ms"] * 1e-3)),
            "scene_over_single_median": a["median_ms"] / b["median_ms"],
            "beyond_spread": a["max_ms"] < b["min_ms"] or a["min_ms"] > b["max_ms"],
            "covered_fraction": float((kept["acc"] > 0).float().mean()),
            "note": "the single-object steps run the field over every sample (no grid) and fit no pose; the scene "
                    "step runs it over the kept rows of four grids and reads 8 kept counts and the poses back"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("compose", "rays", "cull", "fit", "all"))
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each variant (>= 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenegrad", "bench_scene_grad.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_scene_grad.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_grad.py: no HIP device -- this benchmark has no CPU fallback")
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    steps = {"compose": step_compose, "rays": step_rays, "cull": step_cull, "fit": step_fit}
    results = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results["device"] = torch.cuda.get_device_name(0)
    results["library"] = codenerf.build_info()["version"]
    results["models"] = "synthetic"
    results["read_probe_tb_per_s"] = READ_PROBE_TB_S
    for name in (steps if args.step == "all" else [args.step]):
        results[name] = steps[name](dev, args.reps)
        print(json.dumps({name: results[name]}))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
