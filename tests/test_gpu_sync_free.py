"""Sync-free culled renders: the counted field entries (include/codenerf.h, "Counted field calls") against
their parents, render_rays / render_scene with ``sync_free=True`` against ``sync_free=False``, and the
property the flag exists for -- the culled render captured in a graph and replayed on other inputs, and run
under a side stream.  Every comparison is bitwise (NaNs by their bits)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import buffers as B
import occupancy_cases as OC
import streams as S
from test_gpu_parity import dev, embedders, load, models  # noqa: F401

pytestmark = pytest.mark.gpu

FX = [2.0 ** k for k in range(10)]
FD = [2.0 ** k for k in range(4)]
NAN = float("nan")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(B.tensor_bytes(a), B.tensor_bytes(b))


def dev_bits(kind, dev):
    bits = OC.grid_bits(kind, 32, bound=1.0, radius=0.45)
    return torch.from_numpy(np.ascontiguousarray(bits.view(np.int32))).to(dev)


# ---------------------------------------------------------------- 1. the counted entries against their parents

BIG = 128 * 257 + 1       # 258 tiles: more than one round of the persistent loop on 256 CUs
# (capacity C, count k): partial tiles; workgroups without a tile; the loop's second round
COUNTS = [(1, 0), (1, 1), (127, 127), (129, 128), (129, 129), (300, 0), (300, 1), (300, 129),
          (BIG, 128 * 256 + 5), (BIG, BIG)]
KERNELS = ["f32_w16_fold", "f32_w16", "density"]


@pytest.fixture(scope="module")
def field(dev):
    """The coarse synthetic model's packs, one and three code rows' terms, and BIG rows of inputs (read-only)."""
    from codenerf import ops, synthetic
    m, = models(dev, (0,))
    params = [p.detach() for p in m.param_list()]
    gen = torch.Generator().manual_seed(5)
    f = dict(params=params, packs={"f32_w16": m.packed("f32_w16"), "density": m.packed("f32_w16"),
                                   "f32_w16_fold": ops.mlp_pack(params, "f32_w16_fold")}, cb={}, fold={})
    for layout, n in (("one", 1), ("index", 3)):
        zs, zt = synthetic.latent_codes(3, n).to(dev), synthetic.latent_codes(4, n).to(dev)
        f["cb"][layout] = ops.code_bias(params, zs, zt)
        f["fold"][layout] = ops.fold_bias(params, f["cb"][layout])
    f["pts"] = (torch.rand(BIG, 3, generator=gen) * 2.0 - 1.0).to(dev)
    f["rd"] = torch.randn(BIG, 3, generator=gen).to(dev)
    f["index"] = torch.randint(0, 3, (BIG,), generator=gen).to(dev)
    return f


def call(f, kernel, layout, pts, rd, index, count=None):
    """The entry ``kernel`` over the rows of ``pts`` -> its outputs, a tuple of (rows, ..) tensors."""
    from codenerf import ops
    rows, cb = pts.shape[0], f["cb"][layout]
    ci = index if layout == "index" else None
    if kernel == "density":
        return ops.density_field(f["packs"][kernel], cb, FX, pts=pts, code_index=ci, want_sigma=True, want_raw=True,
                                 count=count)
    fold = f["fold"][layout] if kernel == "f32_w16_fold" else None
    return (ops.radiance_field(f["packs"][kernel], cb, rd, 1, rows, FX, FD, pts=pts.view(rows, 1, 3), code_index=ci,
                               precision=kernel, fold_bias=fold, count=count),)


def check_counted(dev, f, kernel, layout, cap, k, count_value):
    """The counted call at capacity ``cap`` with count[0] = ``count_value`` behaves as k rows: rows < k are the
    uncounted call's over the first k rows (n_rays = chunk_rows = k), rows >= k of every output keep their poison,
    and what the inputs hold from row k on -- NaN, code rows 2^40 -- is never used."""
    pts, rd, index = f["pts"][:cap].clone(), f["rd"][:cap].clone(), f["index"][:cap].clone()
    ref = call(f, kernel, layout, pts[:k], rd[:k], index[:k]) if k else None
    pts[k:], rd[k:], index[k:] = NAN, NAN, 1 << 40
    count = torch.tensor([count_value], dtype=torch.int64, device=dev)
    with B.contracts("poison") as arena:                       # a store past any buffer fails on exit
        outs = call(f, kernel, layout, pts, rd, index, count=count)
    assert arena.n_allocations > 0
    for i, o in enumerate(outs):
        o = o.reshape(cap, -1)
        assert torch.isnan(o[k:]).all(), (i, "a row past the count was written")
        if k:
            r = ref[i].reshape(k, -1)
            assert not torch.isnan(r).any()
            assert same_bits(o[:k], r), (i, int((o[:k] != r).any(dim=1).sum()), "rows differ")


@pytest.mark.parametrize("layout", ["one", "index"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("cap,k", COUNTS)
def test_counted_entry_is_its_parent_on_the_first_rows(dev, field, cap, k, kernel, layout):
    check_counted(dev, field, kernel, layout, cap, k, k)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("cap", [1, 129, 300])
def test_count_is_clamped_to_the_capacity(dev, field, cap, kernel):
    check_counted(dev, field, kernel, "index", cap, cap, cap + 7)
    check_counted(dev, field, kernel, "index", cap, 0, -3)


@pytest.mark.parametrize("k", [0, 1, 50])
def test_scatter_rgb_counted(dev, k):
    """cn_scatter_rgb_counted at capacity n_slots: the first k compact rows' colours land, nothing else changes.
    The index rows past k name slots that must stay as they were, their compact rows hold NaN."""
    from codenerf import ops
    n_slots = 50
    gen = torch.Generator().manual_seed(k)
    perm = torch.randperm(n_slots, generator=gen).to(torch.int32).to(dev)
    compact = torch.randn(n_slots, 4, generator=gen).to(dev)
    compact[k:] = NAN
    before = torch.randn(n_slots, 4, generator=gen).to(dev)
    count = torch.tensor([k], dtype=torch.int64, device=dev)
    with B.contracts("poison") as arena:
        raw = arena.empty((n_slots, 4), device=dev)
        raw.copy_(before)
        assert ops.scatter_rgb(compact, perm, raw, count=count) is raw
    expect = before.clone()
    expect[perm[:k].long(), :3] = compact[:k, :3]
    assert same_bits(raw, expect)
    # and the host-count call gives the same
    if k:
        again = before.clone()
        ops.scatter_rgb(compact[:k], perm[:k], again)
        assert same_bits(again, expect)


def test_count_takes_the_points_form_only(dev, field):
    from codenerf import ops
    f = field
    count = torch.tensor([4], dtype=torch.int64, device=dev)
    pts, rd = f["pts"][:8], f["rd"][:8]
    z = torch.rand(8, 2, device=dev)
    cb, fold = f["cb"]["one"], f["fold"]["one"]
    fold_pack, pack = f["packs"]["f32_w16_fold"], f["packs"]["f32_w16"]
    with pytest.raises(ValueError):          # the ray form
        ops.radiance_field(fold_pack, cb, rd, 2, 8, FX, FD, ro=pts, z=z, precision="f32_w16_fold", fold_bias=fold,
                           count=count)
    with pytest.raises(ValueError):          # more than one sample per row
        ops.radiance_field(fold_pack, cb, rd[:4], 2, 4, FX, FD, pts=pts.view(4, 2, 3), precision="f32_w16_fold",
                           fold_bias=fold, count=count)
    with pytest.raises(ValueError):          # the view-rows table
        ops.radiance_field(fold_pack, cb, rd, 1, 8, FX, FD, pts=pts.view(8, 1, 3), precision="f32_w16_fold",
                           fold_bias=fold, view_rows=True, count=count)
    for precision in ("f32", "bf16x3", "bf16x3_w16"):     # another kernel (checked before the pack is looked at)
        with pytest.raises(ValueError):
            ops.radiance_field(pack, cb, rd, 1, 8, FX, FD, pts=pts.view(8, 1, 3), precision=precision, count=count)
    with pytest.raises(ValueError):          # density: the ray form
        ops.density_field(pack, cb, FX, ro=pts, rd=rd, z=z, count=count)
    with pytest.raises(ValueError):          # density: (R, S, 3) points
        ops.density_field(pack, cb, FX, pts=pts.view(4, 2, 3), count=count)
    with pytest.raises(ValueError):          # a count of two values
        ops.density_field(pack, cb, FX, pts=pts, count=torch.zeros(2, dtype=torch.int64, device=dev))


# ---------------------------------------------------------------- 2. renders

VARIANTS = {"plain": {}, "density-coarse": dict(coarse_rgb=False), "tolerance": dict(rgb_tolerance=1e-3),
            "normals": dict(normals=True), "span": dict(span_probes=64)}


def make_scene(dev):
    """The 32 x 32 rays of the render_small.npz camera, the synthetic models, a 16 + 24 unperturbed sampler linear
    in depth and occupancy_cases' four grids at G = 32, bound 1."""
    from codenerf import synthetic
    from codenerf.nerf import OccupancyGrid, PointSampler, RaySampler
    g = load("render_small.npz", dev)
    k = torch.tensor([[28.0, 0, 16.0, 0], [0, 28.0, 16.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    rs = RaySampler(32, 32, k, sample_size=1024, device=dev, datatype=torch.float32)
    ro, rd = (t.reshape(-1, 3) for t in rs.get_bundle(g["pose"]))
    mc, mf = models(dev)
    return dict(ro=ro, rd=rd, mc=mc, mf=mf, zs=g["z_s"], zt=g["z_t"], emb=embedders(dev),
                zs2=synthetic.latent_codes(11, 1).to(dev), zt2=synthetic.latent_codes(12, 1).to(dev),
                zs3=synthetic.latent_codes(21, 3).to(dev), zt3=synthetic.latent_codes(22, 3).to(dev),
                ps=PointSampler(16, 24, 0.8, 1.8, "lindisp", False, torch.float32, dev),
                grids={kind: OccupancyGrid(dev_bits(kind, dev), 32, 1.0) for kind in ("full", "empty", "half", "sphere")})


@pytest.fixture(scope="module")
def scene(dev):
    return make_scene(dev)


def rays(sc, r):
    """``r`` rays spread over the image (copies: the capture tests overwrite theirs in place)."""
    idx = torch.linspace(0, sc["ro"].shape[0] - 1, r).round().long().to(sc["ro"].device)
    return sc["ro"][idx].clone(), sc["rd"][idx].clone()


def render(sc, ro, rd, grid, sync_free, codes="one", **kw):
    from codenerf.nerf import render_rays
    r = ro.shape[0]
    if codes == "one":
        zs, zt = sc["zs"].expand(r, -1), sc["zt"].expand(r, -1)
    else:                                     # three codes, a row per ray
        pick = torch.arange(r, device=ro.device) % 3
        zs, zt = sc["zs3"][pick], sc["zt3"][pick]
    with torch.no_grad():
        return render_rays(ro, rd, zs, zt, sc["ps"], sc["emb"], sc["mc"], sc["mf"], occupancy=grid,
                           sync_free=sync_free, **kw)


def scene_objects(sc, grid0, grid1):
    from codenerf.nerf import SceneObject
    c, s = float(np.cos(0.5)), float(np.sin(0.5))
    return [SceneObject(sc["zs"], sc["zt"], grid0),
            SceneObject(sc["zs2"], sc["zt2"], grid1, rotation=[[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]],
                        translation=[0.1, 0.0, -0.1])]


def render_two(sc, ro, rd, objects, sync_free, **kw):
    from codenerf.nerf import render_scene
    with torch.no_grad():
        return render_scene(ro, rd, objects, sc["ps"], sc["emb"], sc["mc"], sc["mf"], sync_free=sync_free, **kw)


def assert_same_render(out, ref, what):
    assert sorted(out) == sorted(ref), what
    for key in ref:
        assert same_bits(out[key], ref[key]), (what, key)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["full", "empty", "half", "sphere"])
@pytest.mark.parametrize("r", [5, 67])
def test_render_rays_sync_free_is_bitwise_the_synchronising_render(dev, scene, r, kind, variant):
    sc = scene
    ro, rd = rays(sc, r)
    ref = render(sc, ro, rd, sc["grids"][kind], False, **VARIANTS[variant])
    out = render(sc, ro, rd, sc["grids"][kind], True, **VARIANTS[variant])
    assert_same_render(out, ref, (r, kind, variant))
    if (r, kind) == (67, "sphere"):           # the case culls: some rays meet the sphere, some do not
        assert bool((ref["acc_fine"] > 0).any()) and bool((ref["acc_fine"] == 0).any())
    if kind == "empty":
        assert not bool((ref["acc_fine"] > 0).any())


@pytest.mark.parametrize("r", [5, 67])
def test_render_rays_sync_free_tolerance_without_a_grid(dev, scene, r):
    sc = scene
    ro, rd = rays(sc, r)
    ref = render(sc, ro, rd, None, False, rgb_tolerance=1e-3)
    assert_same_render(render(sc, ro, rd, None, True, rgb_tolerance=1e-3), ref, r)
    # nothing culled: the flag changes nothing
    assert_same_render(render(sc, ro, rd, None, True), render(sc, ro, rd, None, False), (r, "no culling"))


@pytest.mark.parametrize("variant", ["plain", "tolerance"])
@pytest.mark.parametrize("r", [5, 67])
def test_render_rays_sync_free_three_codes(dev, scene, r, variant):
    sc = scene
    ro, rd = rays(sc, r)
    ref = render(sc, ro, rd, sc["grids"]["sphere"], False, codes="three", **VARIANTS[variant])
    assert_same_render(render(sc, ro, rd, sc["grids"]["sphere"], True, codes="three", **VARIANTS[variant]), ref, r)


@pytest.mark.parametrize("kw", [{}, dict(coarse_rgb=False), dict(span_probes=64)], ids=["plain", "density-coarse", "span"])
def test_render_scene_sync_free(dev, scene, kw):
    """K = 2, the second object's grid empty."""
    sc = scene
    ro, rd = rays(sc, 67)
    objects = scene_objects(sc, sc["grids"]["sphere"], sc["grids"]["empty"])
    ref = render_two(sc, ro, rd, objects, False, **kw)
    assert_same_render(render_two(sc, ro, rd, objects, True, **kw), ref, kw)
    assert bool((ref["acc_objects_fine"][0] > 0).any()) and not bool(ref["acc_objects_fine"][1].any())


def test_sync_free_needs_fp32_models(dev, scene):
    import inspect
    from codenerf.nerf import parallel_image_render
    sc = scene
    ro, rd = rays(sc, 5)
    slow, = models(dev, (0,), precision="bf16x3")
    keep = sc["mc"]
    try:
        sc["mc"] = slow
        with pytest.raises(ValueError):
            render(sc, ro, rd, sc["grids"]["sphere"], True)
        with pytest.raises(ValueError):
            render_two(sc, ro, rd, scene_objects(sc, sc["grids"]["sphere"], sc["grids"]["empty"]), True)
    finally:
        sc["mc"] = keep
    assert inspect.signature(parallel_image_render).parameters["sync_free"].default is False


# ---------------------------------------------------------------- 3. capture and replay


def replay_on_other_inputs(sc, graph, out, eager, ro, rd, bits):
    """Three replays of ``graph`` (its result ``out``) after overwriting ro, rd and the grid's bits in place: the
    camera turned away under the sphere grid (nothing kept), a moved camera under the empty grid, another under
    the full grid.  After each the outputs equal ``eager()``: the synchronising render of the same inputs."""
    ro0, rd0 = ro.clone(), rd.clone()
    shift = torch.tensor([0.1, 0.05, 0.0], device=ro.device)
    seen = []
    for name, new_ro, new_rd, kind in (("away", ro0, -rd0, "sphere"), ("moved", ro0 + shift, rd0, "empty"),
                                       ("moved back", ro0 - shift, rd0, "full")):
        ro.copy_(new_ro)
        rd.copy_(new_rd)
        bits.copy_(dev_bits(kind, ro.device))
        for t in out.values():
            B.poison_(t)                      # a replay that wrote nothing leaves this behind
        graph.replay()
        torch.cuda.synchronize()
        ref = eager()
        assert_same_render(out, ref, name)
        seen.append(bool((ref["acc_fine"] > 0).any()))
    assert seen == [False, False, True], seen    # the kept count did change, and was 0 twice


def test_culled_render_is_captured_and_replayed(dev, scene):
    from codenerf.nerf import OccupancyGrid
    sc = scene
    ro, rd = rays(sc, 67)
    bits = dev_bits("sphere", dev)
    grid = OccupancyGrid(bits, 32, 1.0)
    assert grid.bits.data_ptr() == bits.data_ptr()
    render(sc, ro, rd, grid, True, rgb_tolerance=1e-3)          # the packs are cached from here on
    graph, out = S.capture(lambda: render(sc, ro, rd, grid, True, rgb_tolerance=1e-3))
    replay_on_other_inputs(sc, graph, out, lambda: render(sc, ro.clone(), rd.clone(),
                                                          OccupancyGrid(bits.clone(), 32, 1.0), False,
                                                          rgb_tolerance=1e-3), ro, rd, bits)


def test_culled_scene_is_captured_and_replayed(dev, scene):
    from codenerf.nerf import OccupancyGrid
    sc = scene
    ro, rd = rays(sc, 67)
    bits = dev_bits("sphere", dev)
    objects = scene_objects(sc, OccupancyGrid(bits, 32, 1.0), sc["grids"]["empty"])
    render_two(sc, ro, rd, objects, True)
    graph, out = S.capture(lambda: render_two(sc, ro, rd, objects, True))
    replay_on_other_inputs(sc, graph, out, lambda: render_two(
        sc, ro.clone(), rd.clone(), scene_objects(sc, OccupancyGrid(bits.clone(), 32, 1.0), sc["grids"]["empty"]),
        False), ro, rd, bits)


# The control -- the same captures with sync_free=False are refused, so the harness does see the read-back --
# runs in a child process: a capture that raised leaves its stream and the allocator's pool in a state the
# rest of the session should not inherit (tests/test_gpu_streams.py does the same).


def refusals_main():
    import codenerf
    codenerf.load_library()
    sc = make_scene(torch.device("cuda", 0))
    ro, rd = rays(sc, 67)
    grid = sc["grids"]["sphere"]
    objects = scene_objects(sc, grid, sc["grids"]["empty"])
    render(sc, ro, rd, grid, True, rgb_tolerance=1e-3)
    render_two(sc, ro, rd, objects, True)

    def outcome(call):
        try:
            S.capture(call)
            return "captured"
        except S.Refused as e:
            return "refused: " + str(e)[:200]

    results = {"render_rays, sync_free=False": outcome(lambda: render(sc, ro, rd, grid, False, rgb_tolerance=1e-3)),
               "render_scene, sync_free=False": outcome(lambda: render_two(sc, ro, rd, objects, False)),
               # and the refusals left the process able to capture
               "render_rays, sync_free=True": outcome(lambda: render(sc, ro, rd, grid, True, rgb_tolerance=1e-3)),
               "render_scene, sync_free=True": outcome(lambda: render_two(sc, ro, rd, objects, True))}
    print("SYNC_FREE_REFUSALS " + json.dumps(results))


def test_the_synchronising_renders_refuse_capture(dev):
    torch.cuda.synchronize()
    here = os.path.dirname(os.path.abspath(__file__))
    done = subprocess.run([sys.executable, "-c", "import conftest, test_gpu_sync_free as M; M.refusals_main()"],
                          cwd=here, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in done.stdout.splitlines() if ln.startswith("SYNC_FREE_REFUSALS ")]
    assert done.returncode == 0 and lines, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    results = json.loads(lines[-1][len("SYNC_FREE_REFUSALS "):])
    print(lines[-1])
    for name, got in results.items():
        want = "refused" if name.endswith("False") else "captured"
        assert got.startswith(want), results


# ---------------------------------------------------------------- 4. under a side stream


def test_culled_render_under_a_side_stream(dev, scene):
    """The sync-free render's every ops call lands on the current stream: its log under a side stream (the
    default stream held busy) equals the default-stream log, bit for bit (unwritten rows: the poison)."""
    sc = scene
    ro, rd = rays(sc, 67)

    def run():
        render(sc, ro, rd, sc["grids"]["sphere"], True, rgb_tolerance=1e-3)

    run()
    with B.contracts("poison", log_returns_of=None), S.plain() as base:
        run()
    with B.contracts("poison", log_returns_of=None), S.side_stream(wall_ms=base.wall_ms) as side:
        run()
    assert base.returns and side.slack_ms and min(side.slack_ms) > 0
    names = [r[0] for r in base.returns]
    assert "weight_cull" in names and "occupancy_cull" in names and "scatter_rgb" in names
    S.compare_logs(base.returns, side.returns, "the side-stream run")
