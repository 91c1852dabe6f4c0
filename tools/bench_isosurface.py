"""Measure the on-device iso-surface extraction (cn_isosurface_count, cn_isosurface_emit) beside the
density_grid call that produces its input.  Needs an MI355X: there is no CPU fallback.

    python tools/bench_isosurface.py [--reps 30] [--n 129 257] [--out PATH]

Writes profiles/isosurface/bench_isosurface.json.  All times are device events around one call into
preallocated buffers (the extraction's host read-back of the two totals is not part of either entry
and is not timed); the calls of one resolution alternate inside one process after a warm-up of all of
them, and every figure carries its spread (min / median / max over the repetitions).

Fields: ``model``, the activated density of the synthetic model (no trained checkpoint ships with the
repository) at the median level of its own grid, and ``sphere``, radius - |p| at level 0 with radius
0.7 in [-1, 1]^3.  density_grid is timed once per resolution (it does not depend on the level).

Bytes: what each entry has to move at the least, from the workspace layout of include/codenerf.h, with
N nodes, B workgroups, V vertices and T faces --
  count   4 N (nodes read) + 4 N (words written) + 4 N (words read) + 8 N (offsets written) + 16 B;
  emit    8 N (words read by both launches) + 12 V + 12 T written
(neighbour reads that the caches serve, and the offsets read at the active nodes only, are left out)
-- divided by the median time, beside the HBM peak: 8.0 TB/s by specification, 6.29 TB/s measured for
a float4 copy.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-nerf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_density import alternate, setup, spread  # noqa: E402

HBM_PEAK_SPEC_TBS = 8.0
HBM_PEAK_COPY_TBS = 6.29
BOUND = 1.0


def sphere_grid(dev, n, radius=0.7):
    lin = torch.linspace(-BOUND, BOUND, n, dtype=torch.float32, device=dev)
    return radius - torch.sqrt(lin[:, None, None] ** 2 + lin[None, :, None] ** 2 + lin[None, None, :] ** 2)


class Extraction:
    """One grid's buffers and the two raw calls on them."""

    def __init__(self, nodes, axis, iso):
        from codenerf import _lib
        self.lib, self.L = _lib.load(), _lib
        self.nodes, self.axis, self.iso, self.n = nodes.contiguous(), axis, float(iso), nodes.shape[0]
        dev = nodes.device
        self.workspace = torch.empty((self.lib.cn_isosurface_workspace_bytes(self.n) + 7) // 8, dtype=torch.int64,
                                     device=dev)
        self.counts = torch.zeros(2, dtype=torch.int64, device=dev)
        self.count()
        self.v, self.t = (int(k) for k in self.counts.tolist())
        self.vertices = torch.empty(self.v, 3, dtype=torch.float32, device=dev)
        self.faces = torch.empty(self.t, 3, dtype=torch.int32, device=dev)

    def count(self):
        L = self.L
        L.check(self.lib.cn_isosurface_count(L.ptr(self.nodes), self.n, self.iso, L.ptr(self.workspace),
                                             L.ptr(self.counts), L.stream_of(self.nodes)), "cn_isosurface_count")

    def emit(self):
        L = self.L
        L.check(self.lib.cn_isosurface_emit(L.ptr(self.nodes), L.ptr(self.axis), self.n, self.iso, L.ptr(self.workspace),
                                            self.v, self.t, L.ptr(self.vertices) if self.v else None,
                                            L.ptr(self.faces) if self.t else None, L.stream_of(self.nodes)),
                "cn_isosurface_emit")

    def bytes(self):
        nodes = self.n ** 3
        blocks = (nodes + 255) // 256
        return {"count": 20 * nodes + 16 * blocks, "emit": 8 * nodes + 12 * self.v + 12 * self.t}


def rate(nbytes, sp):
    tbs = nbytes / (sp["median_ms"] * 1e-3) / 1e12
    return {"bytes": nbytes, "tb_per_s": tbs, "of_hbm_spec": tbs / HBM_PEAK_SPEC_TBS, "of_hbm_copy": tbs / HBM_PEAK_COPY_TBS}


def step(dev, n, reps):
    from codenerf import ops
    from codenerf.nerf import density_grid
    (model, _), emb, zs, _ = setup(dev)
    lin = torch.linspace(-BOUND, BOUND, n, dtype=torch.float32, device=dev)
    grid = density_grid(model, emb, zs, n, BOUND)
    fields = {"model": Extraction(grid, lin, float(grid.median())), "sphere": Extraction(sphere_grid(dev, n), lin, 0.0)}
    fns = {"density_grid": lambda: density_grid(model, emb, zs, n, BOUND)}
    for name, ex in fields.items():
        fns[f"{name}/count"] = ex.count
        fns[f"{name}/emit"] = ex.emit
    ms = alternate(fns, reps, warmup=3)
    dg = spread(ms["density_grid"])
    res = {"n": n, "nodes": n ** 3, "density_grid": dict(dg, points_per_s=n ** 3 / (dg["median_ms"] * 1e-3)), "fields": {}}
    for name, ex in fields.items():
        count, emit = spread(ms[f"{name}/count"]), spread(ms[f"{name}/emit"])
        nbytes = ex.bytes()
        v, f = ops.isosurface(ex.nodes, ex.iso, lin)              # the public path gives the same mesh
        assert torch.equal(v.view(torch.int32), ex.vertices.view(torch.int32)) and torch.equal(f, ex.faces)
        total = count["median_ms"] + emit["median_ms"]
        res["fields"][name] = {
            "iso": ex.iso, "vertices": ex.v, "faces": ex.t,
            "count": dict(count, **rate(nbytes["count"], count)), "emit": dict(emit, **rate(nbytes["emit"], emit)),
            "extraction_median_ms": total, "extraction_over_density_grid": total / dg["median_ms"],
            "extraction_is_smaller_beyond_spread": count["max_ms"] + emit["max_ms"] < dg["min_ms"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each call (>= 20)")
    ap.add_argument("--n", type=int, nargs="+", default=[129, 257], help="grid resolutions")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isosurface", "bench_isosurface.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_isosurface.py: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_isosurface.py: no HIP device -- this benchmark has no CPU fallback")
    import codenerf
    codenerf.load_library()
    dev = torch.device("cuda", 0)
    results = {"device": torch.cuda.get_device_name(0), "library": codenerf.build_info()["version"],
               "models": "synthetic", "bound": BOUND, "reps": args.reps,
               "hbm_peak_tb_per_s": {"spec": HBM_PEAK_SPEC_TBS, "float4_copy_measured": HBM_PEAK_COPY_TBS},
               "resolutions": {}}
    for n in args.n:
        results["resolutions"][str(n)] = step(dev, n, args.reps)
        print(json.dumps({n: results["resolutions"][str(n)]}))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
