"""Occupancy-grid sample culling on the device: cn_occupancy_build / _cull / _expand against the numpy
oracle (tests/occupancy_cases.py), the existing field kernels over the compact list against
themselves over every sample, and render_rays / parallel_image_render with ``occupancy=``.

Every comparison is exact: the lookup is stated in fp32 operation by operation, the compact order is
fixed, and a kept sample goes through the same field arithmetic wherever it sits in the launch.
"""
import numpy as np
import pytest
import torch

import occupancy_cases as OC
from test_gpu_parity import dev, embedders, load, models  # noqa: F401

pytestmark = pytest.mark.gpu

FX = [2.0 ** k for k in range(10)]
FD = [2.0 ** k for k in range(4)]
SCAN_PART = 4096     # rays per partition of the cull's offset scan (kScanPart, occupancy.hip)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def dev_bits(bits, dev):
    return T(np.asarray(bits).view(np.int32), dev)


def empty_row(dev):
    return torch.tensor([0.0, 0.0, 0.0, -1.0e4], device=dev)


# ---------------------------------------------------------------- build


def _node_field(g, seed):
    """Random nodes in [0, 1) with ties at the threshold 0.5, NaNs, and a single hot node in a corner
    cell and one in the centre of an otherwise cold region."""
    rng = np.random.default_rng(seed)
    nodes = rng.random((g + 1,) * 3).astype(np.float32)
    nodes[nodes > 0.45] *= 0.5                       # sparse: most cells cold, so dilation shows
    nodes[rng.random(nodes.shape) < 0.01] = 0.5      # ties: not occupied
    nodes[rng.random(nodes.shape) < 0.002] = np.nan  # NaN: occupied
    nodes[rng.random(nodes.shape) < 0.003] = 0.9     # above the threshold
    nodes[:9, :9, :9] = 0.0
    nodes[0, 0, 0] = 0.75                            # the corner node
    h = g // 2
    nodes[h - 4:h + 5, h - 4:h + 5, h - 4:h + 5] = 0.0
    nodes[h, h, h] = 0.75                            # one node in the centre
    nodes[g - 3:, :, :] = 0.0
    nodes[g, 7, g] = np.nextafter(np.float32(0.5), np.float32(1.0))      # on two faces, just above
    return nodes


@pytest.mark.parametrize("dilate", [0, 1, 2])
@pytest.mark.parametrize("g", [32, 64])
def test_build_matches_oracle(dev, g, dilate):
    from codenerf import ops
    nodes = _node_field(g, g + dilate)
    want = OC.build_bits(nodes, 0.5, dilate)
    got = ops.occupancy_build(T(nodes, dev), 0.5, dilate)
    assert got.dtype == torch.int32 and got.shape == (g ** 3 // 32,)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    occ = OC.unpack_cells(want, g)
    assert 0.0 < occ.mean() < 1.0
    assert occ[:1 + dilate, :1 + dilate, :1 + dilate].all() and not occ[2 + dilate, 2 + dilate, 2 + dilate]


def test_grid_constructors(dev):
    from codenerf.nerf import OccupancyGrid
    g = 32
    nodes = _node_field(g, 5)
    grid = OccupancyGrid.from_nodes(T(nodes, dev), 0.5, bound=1.0)          # dilate 1
    assert grid.resolution == g and grid.bound == 1.0
    assert np.array_equal(grid.bits.cpu().numpy().view(np.uint32), OC.build_bits(nodes, 0.5, 1))
    assert grid.occupied_fraction() == OC.build_cells(nodes, 0.5, 1).mean()
    full = OccupancyGrid.full(g, 2.0, dev)
    assert full.occupied_fraction() == 1.0 and full.bits.dtype == torch.int32
    assert np.array_equal(full.bits.cpu().numpy().view(np.uint32), OC.grid_bits("full", g))
    with pytest.raises(ValueError):
        OccupancyGrid(full.bits, 48, 1.0)
    with pytest.raises(ValueError):
        OccupancyGrid(full.bits[:-1], g, 1.0)
    with pytest.raises(ValueError):
        OccupancyGrid(full.bits, g, 0.0)


# ---------------------------------------------------------------- cull


def _check_cull(dev, ro, rd, z, chunk_rows, code_index, bits, g=32, bound=1.0):
    """ops.occupancy_cull against the oracle, every output exact -> (oracle dict, the op's outputs)."""
    from codenerf import ops
    want = OC.cull(ro, rd, z, chunk_rows, code_index, bits, g, bound)
    tro, trd, tz = T(ro, dev), T(rd, dev), T(z, dev)
    ci = None if code_index is None else T(code_index, dev)
    got = ops.occupancy_cull(tro, trd, tz, chunk_rows, dev_bits(bits, dev), g, bound, code_index=ci)
    count, sidx, pts, vdir, code, state = got
    assert isinstance(count, int) and count == want["count"]
    assert sidx.dtype == torch.int32 and code.dtype == torch.int64
    assert sidx.shape == (count,) and pts.shape == (count, 3) and vdir.shape == (count, 3) and code.shape == (count,)
    assert torch.equal(sidx, T(want["sample_index"], dev))
    # the points are ops.ray_points' (the field kernel's own formula), bit for bit (a kept point is finite)
    all_pts = ops.ray_points(tro, trd, tz).reshape(-1, 3)
    assert torch.equal(pts, all_pts[sidx.long()])
    assert torch.equal(pts, T(want["pts"], dev))
    # a copied rd row, NaNs included (a Q1 direction ray may be a NaN ray): the same bits
    assert torch.equal(vdir.view(torch.int32), T(want["vdir"], dev).view(torch.int32))
    assert torch.equal(code, T(want["code_out"], dev))
    return want, got


@pytest.mark.parametrize("grid", ["full", "empty", "half", "sphere"])
@pytest.mark.parametrize("r,s", [(1, 1), (37, 64), (50, 3), (9, 192), (5, 512)])
def test_cull_matches_oracle(dev, r, s, grid):
    bits = OC.grid_bits(grid, 32, radius=0.7)
    ro, rd, z = OC.random_rays(r, s, seed=r * s)
    index = np.random.default_rng(r).integers(0, 3, size=r)
    kept = []
    for chunk_rows in sorted({r, 16, 1}):          # one chunk; a ragged last chunk (r > 16); per-ray
        for code_index in (None, index):
            want, _ = _check_cull(dev, ro, rd, z, chunk_rows, code_index, bits)
            kept.append(want["count"])
    if grid == "empty":
        assert max(kept) == 0
    elif r > 1:
        assert 0 < min(kept) < r * s               # the cube's outside culls under every grid


def test_cull_without_code_output(dev):
    from codenerf import ops
    ro, rd, z = OC.random_rays(20, 7, seed=1)
    out = ops.occupancy_cull(T(ro, dev), T(rd, dev), T(z, dev), 20, dev_bits(OC.grid_bits("sphere", 32), dev), 32, 1.0,
                             want_code=False)
    assert out[4] is None and out[0] == OC.cull(ro, rd, z, 20, None, OC.grid_bits("sphere", 32), 32, 1.0)["count"]


@pytest.mark.parametrize("grid", ["full", "half", "sphere"])
def test_cull_samples_on_faces(dev, grid):
    """Axis-aligned rays with depths k / 16: every sample sits exactly on a cell face, the first / last
    on a face of the cube (u = 0 inside, u = G outside)."""
    ro, rd, z = OC.face_rays(40)
    want, _ = _check_cull(dev, ro, rd, z, 6, None, OC.grid_bits(grid, 32, radius=0.7))
    if grid == "full":
        keep = want["keep"]
        assert keep[0, :32].all() and not keep[0, 32:].any()
        assert not keep[1, 0] and keep[1, 1:33].all() and not keep[1, 33:].any()


def test_cull_nan_and_far_points(dev):
    ro, rd, z = OC.random_rays(12, 70, seed=4, spread=0.8)
    ro[1, 0] = np.nan              # a NaN ray: every sample empty
    rd[2, 1] = np.nan
    z[3, 5] = np.nan               # one NaN sample
    z[4, 9] = np.inf
    ro[5] = [1e30, -1e30, 3e38]    # far outside (the lookup overflows to inf)
    rd[6] *= 1e20
    ro[7] = [5.0, 0.0, 0.0]        # outside, finite
    rd[7] = [1.0, 0.0, 0.0]
    want, _ = _check_cull(dev, ro, rd, z, 5, None, OC.grid_bits("full", 32))
    keep = want["keep"]
    assert not keep[[1, 2, 5, 7]].any() and not keep[3, 5] and not keep[4, 9]
    assert keep[0].any() and keep[3].sum() >= keep[3].size - 40


def test_cull_scan_crosses_partitions(dev):
    """More rays than two partitions of the offset scan (SCAN_PART = 4096 rays each) plus a ragged rest,
    at S = 4: the running total is carried twice."""
    r = 2 * SCAN_PART + 1234
    assert r > 2 * SCAN_PART
    ro, rd, z = OC.random_rays(r, 4, seed=9)
    want, _ = _check_cull(dev, ro, rd, z, 4096, None, OC.grid_bits("sphere", 32, radius=0.7))
    idx = want["sample_index"] // 4
    assert (idx < SCAN_PART).any() and ((idx >= SCAN_PART) & (idx < 2 * SCAN_PART)).any() and \
        (idx >= 2 * SCAN_PART).any()


def test_cull_other_resolution_and_bound(dev):
    ro, rd, z = OC.random_rays(33, 48, seed=11, spread=2.0)
    for g, bound in ((64, 1.5), (128, 0.7)):
        want, _ = _check_cull(dev, ro, rd, z, 33, None, OC.grid_bits("sphere", g, bound=bound, radius=0.6 * bound),
                              g=g, bound=bound)
        assert 0 < want["count"] < 33 * 48


# ---------------------------------------------------------------- expand


@pytest.mark.parametrize("grid", ["empty", "full_inside", "sphere"])
@pytest.mark.parametrize("r,s", [(1, 1), (37, 64), (50, 3), (5, 512)])
def test_expand(dev, r, s, grid):
    """Kept rows bit-equal, culled rows the empty row; M' = 0 (no compact tensor at all) and M' = R S."""
    from codenerf import ops
    ro, rd, z = OC.random_rays(r, s, seed=r + s, spread=0.4 if grid == "full_inside" else 1.3)
    if grid == "full_inside":
        ro = np.clip(ro, -0.3, 0.3)
        rd = np.clip(rd, -1.0, 1.0)              # |p| <= 0.3 + 0.4: inside the cube
    bits = OC.grid_bits("full" if grid == "full_inside" else grid, 32)
    want = OC.cull(ro, rd, z, r, None, bits, 32, 1.0)
    count, sidx, _, _, _, state = ops.occupancy_cull(T(ro, dev), T(rd, dev), T(z, dev), r, dev_bits(bits, dev), 32, 1.0)
    assert count == {"empty": 0, "full_inside": r * s}.get(grid, count)
    compact = torch.randn(count, 4, generator=torch.Generator().manual_seed(r)).to(dev)
    compact[::3, 3] = float("nan")               # bits, not values, are moved
    raw = ops.occupancy_expand(compact if count else None, state)
    assert raw.shape == (r, s, 4)
    expect = empty_row(dev).repeat(r * s, 1)
    expect[sidx.long()] = compact
    assert torch.equal(raw.view(-1, 4).view(torch.int32), expect.view(torch.int32))
    keep = T(want["keep"], dev)
    assert torch.equal(raw[~keep], empty_row(dev).repeat(int((~keep).sum()), 1))
    if count == 0:
        assert torch.equal(ops.occupancy_expand(torch.empty(0, 4, device=dev), state), raw)


def test_expand_refuses_wrong_row_count(dev):
    from codenerf import ops
    ro, rd, z = OC.random_rays(10, 8, seed=2)
    bits = dev_bits(OC.grid_bits("sphere", 32, radius=0.7), dev)
    count, *_, state = ops.occupancy_cull(T(ro, dev), T(rd, dev), T(z, dev), 10, bits, 32, 1.0)
    assert count > 1
    with pytest.raises(AssertionError):
        ops.occupancy_expand(torch.zeros(count - 1, 4, device=dev), state)
    with pytest.raises(AssertionError):
        ops.occupancy_expand(None, state)


def test_empty_row_is_zero_density(dev):
    """CN_EMPTY_SIGMA_RAW composites as exactly nothing: weights 0, acc 0, the other samples' weights
    those of a ray on which the culled samples carry zero density."""
    from codenerf import ops
    r, s = 7, 16
    g = torch.Generator().manual_seed(0)
    raw = torch.randn(r, s, 4, generator=g).to(dev)
    z = torch.sort(0.8 + torch.rand(r, s, generator=g), dim=-1).values.to(dev)
    rd = torch.randn(r, 3, generator=g).to(dev)
    allempty = empty_row(dev).repeat(r, s, 1)
    rgb, _, acc, w, _ = ops.volume_render(allempty, z, rd)
    assert torch.equal(w, torch.zeros_like(w)) and torch.equal(acc, torch.zeros_like(acc))
    assert torch.equal(rgb, torch.zeros_like(rgb))
    mixed = raw.clone()
    mixed[:, 1::2] = empty_row(dev)
    w_mixed = ops.volume_render(mixed, z, rd)[3]
    assert torch.equal(w_mixed[:, 1::2], torch.zeros(r, s // 2, device=dev))
    assert (w_mixed[:, 0::2] > 0).all()


# ---------------------------------------------------------------- field equivalence


@pytest.fixture(scope="module")
def field(dev):
    """The coarse synthetic model: its parameter list, fp32 pack and folded pack (shared, read-only)."""
    from codenerf import ops
    m, = models(dev, (0,))
    params = [p.detach() for p in m.param_list()]
    return params, m.packed("f32_w16"), ops.mlp_pack(params, "f32_w16_fold")


def _codes(dev, layout, r, seed=3):
    from codenerf import synthetic
    n = {"one": 1, "per_ray": r, "index": 3}[layout]
    zs, zt = synthetic.latent_codes(seed, n).to(dev), synthetic.latent_codes(seed + 1, n).to(dev)
    index = None
    if layout == "index":
        index = torch.randint(0, 3, (r,), generator=torch.Generator().manual_seed(r)).to(dev)
    return zs, zt, index


@pytest.mark.parametrize("layout", ["one", "per_ray", "index"])
@pytest.mark.parametrize("kernel", ["f32_w16", "f32_w16_fold", "density"])
@pytest.mark.parametrize("r,s,chunk_rows", [(37, 64, 16), (50, 3, 50)])
def test_field_over_compact_list(dev, field, r, s, chunk_rows, kernel, layout):
    """expand(field(compact)) == where(keep, field over every sample, empty row), bit for bit, for the
    fp32 field, the folded field and the density kernel -- in-range points (|x| 2^9 <= 2^14)."""
    from codenerf import ops
    params, packed, packed_fold = field
    ro, rd, z = OC.random_rays(r, s, seed=r)
    bits = OC.grid_bits("sphere", 32, radius=0.7)
    tro, trd, tz = T(ro, dev), T(rd, dev), T(z, dev)
    zs, zt, index = _codes(dev, layout, r)
    cb = ops.code_bias(params, zs, zt)
    fold = ops.fold_bias(params, cb) if kernel == "f32_w16_fold" else None
    many = cb.shape[0] > 1

    def run(rays, n_samples, rows, ci, **geo):
        if kernel == "density":
            dgeo = dict(geo, rd=rays) if "ro" in geo else geo
            return ops.density_field(packed, cb, FX, code_index=ci, want_sigma=False, want_raw=True, **dgeo)
        return ops.radiance_field(packed_fold if fold is not None else packed, cb, rays, n_samples, rows, FX, FD,
                                  code_index=ci, precision=kernel, fold_bias=fold, **geo)

    full = run(trd, s, chunk_rows, index, ro=tro, z=tz)
    count, sidx, pts, vdir, code, state = ops.occupancy_cull(tro, trd, tz, chunk_rows, dev_bits(bits, dev), 32, 1.0,
                                                             code_index=index)
    assert 0 < count < r * s
    if kernel == "density":
        compact = run(None, 1, count, code if many else None, pts=pts)
    else:
        compact = run(vdir, 1, count, code if many else None, pts=pts.view(count, 1, 3))
    got = ops.occupancy_expand(compact, state)
    keep = T(OC.cull(ro, rd, z, chunk_rows, None, bits, 32, 1.0)["keep"], dev)
    expect = torch.where(keep[..., None], full.view(r, s, 4), empty_row(dev))
    assert torch.equal(got, expect)


# ---------------------------------------------------------------- render


def _image_rays(dev, g, h, w):
    from codenerf.nerf import RaySampler
    k = torch.tensor([[28.0, 0, w / 2, 0], [0, 28.0, h / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    rs = RaySampler(h, w, k, sample_size=min(4096, h * w), device=dev, datatype=torch.float32)
    ro, rd = rs.get_bundle(g["pose"])
    return rs, ro.reshape(-1, 3), rd.reshape(-1, 3)


@pytest.fixture(scope="module")
def scene(dev):
    """32 x 32 rays of the render_small.npz pose, the synthetic coarse and fine models."""
    g = load("render_small.npz", dev)
    _, ro, rd = _image_rays(dev, g, 32, 32)
    n = ro.shape[0]
    mc, mf = models(dev)
    return dict(g=g, ro=ro, rd=rd, n=n, mc=mc, mf=mf, zs=g["z_s"].expand(n, -1), zt=g["z_t"].expand(n, -1))


def _same(a, b, equal_nan=False):
    if equal_nan:      # disp = 1 / max(eps, depth / acc) is NaN where acc = 0: NaN in the same places
        return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
            torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    return torch.equal(a, b)


@pytest.mark.parametrize("coarse_rgb", [True, False])
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("nc,nf", [(64, 64), (32, 128)])
def test_render_full_grid_bitwise(dev, scene, nc, nf, fold, coarse_rgb):
    """A full grid that holds every sample culls nothing: every entry of the result is the unculled
    call's, bit for bit."""
    from codenerf.nerf import OccupancyGrid, PointSampler, render_rays
    sc = scene
    ps = PointSampler(nc, nf, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    grid = OccupancyGrid.full(32, 4.0, dev)
    before = sc["mc"].fold, sc["mf"].fold
    try:
        sc["mc"].fold = sc["mf"].fold = fold
        with torch.no_grad():
            args = (sc["ro"], sc["rd"], sc["zs"], sc["zt"], ps, embedders(dev), sc["mc"], sc["mf"])
            ref = render_rays(*args, chunk_rows=400, coarse_rgb=coarse_rgb)
            out = render_rays(*args, chunk_rows=400, coarse_rgb=coarse_rgb, occupancy=grid)
    finally:
        sc["mc"].fold, sc["mf"].fold = before
    assert sorted(out) == sorted(ref) and ("rgb_coarse" in out) == coarse_rgb
    for k in ref:
        assert torch.equal(out[k], ref[k]), k


@pytest.mark.parametrize("coarse_rgb", [True, False])
@pytest.mark.parametrize("nc,nf", [(64, 64), (32, 128)])
def test_render_sphere_grid_composed(dev, scene, nc, nf, coarse_rgb):
    """With a sphere grid the result is the one composed from the unculled fields, torch.where with the
    empty row, and the existing volume_render / sample_pdf."""
    from codenerf import ops
    from codenerf.nerf import OccupancyGrid, PointSampler, render_rays
    from codenerf.models.model import _field_op
    sc = scene
    ro, rd, n = sc["ro"], sc["rd"], sc["n"]
    ps = PointSampler(nc, nf, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    bound, radius, chunk = 1.0, 0.45, 400
    bits = OC.grid_bits("sphere", 32, bound=bound, radius=radius)
    grid = OccupancyGrid(dev_bits(bits, dev), 32, bound)
    emb = embedders(dev)
    with torch.no_grad():
        out = render_rays(ro, rd, sc["zs"], sc["zt"], ps, emb, sc["mc"], sc["mf"], chunk_rows=chunk,
                          coarse_rgb=coarse_rgb, occupancy=grid)

        def unculled(model, z, density_only):
            if density_only:
                from codenerf.models.model import density_code_bias
                return ops.density_field(model.packed(), density_code_bias(model, sc["g"]["z_s"]), FX, ro=ro, rd=rd,
                                         z=z, want_sigma=False, want_raw=True)
            return _field_op(model, sc["g"]["z_s"], sc["g"]["z_t"], rd, chunk, FX, FD, ro=ro, z=z)

        def keep_of(z):
            k = OC.lookup(OC.ray_points(ro.cpu().numpy(), rd.cpu().numpy(), z.cpu().numpy()), bits, 32, bound)
            return T(k, dev)

        _, z_c = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
        keep_c = keep_of(z_c)
        raw_c = torch.where(keep_c[..., None], unculled(sc["mc"], z_c, not coarse_rgb), empty_row(dev))
        rgb_c, disp_c, acc_c, w_c, depth_c = ops.volume_render(raw_c, z_c, rd)
        _, z_f = ops.sample_pdf(ro, rd, w_c[..., 1:-1], z_c, nf, ps.u_lin, want_pts=False)
        keep_f = keep_of(z_f)
        raw_f = torch.where(keep_f[..., None], unculled(sc["mf"], z_f, False), empty_row(dev))
        rgb_f, disp_f, acc_f, _, depth_f = ops.volume_render(raw_f, z_f, rd)
    expect = {"disp_coarse": disp_c, "acc_coarse": acc_c, "weights_coarse": w_c, "depth_coarse": depth_c,
              "z_coarse": z_c, "rgb_fine": rgb_f, "disp_fine": disp_f, "acc_fine": acc_f, "depth_fine": depth_f,
              "z_fine": z_f}
    if coarse_rgb:
        expect["rgb_coarse"] = rgb_c
    assert sorted(out) == sorted(expect)
    # the grid does cull here, and does not cull everything
    assert 0.02 < keep_c.float().mean() < 0.9 and 0.02 < keep_f.float().mean() < 0.98
    assert (acc_c == 0).any()                       # rays that miss the sphere altogether
    for k, v in expect.items():
        assert _same(out[k], v, equal_nan=k.startswith(("disp", "depth"))), k
    assert torch.equal(out["weights_coarse"][~keep_c], torch.zeros(int((~keep_c).sum()), device=dev))


def test_render_empty_grid(dev, scene):
    from codenerf.nerf import OccupancyGrid, PointSampler, render_rays
    sc = scene
    ps = PointSampler(32, 128, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    grid = OccupancyGrid(dev_bits(OC.grid_bits("empty", 32), dev), 32, 4.0)
    with torch.no_grad():
        out = render_rays(sc["ro"], sc["rd"], sc["zs"], sc["zt"], ps, embedders(dev), sc["mc"], sc["mf"],
                          chunk_rows=400, occupancy=grid)
    for k in ("rgb_coarse", "rgb_fine", "acc_coarse", "acc_fine", "weights_coarse"):
        assert torch.equal(out[k], torch.zeros_like(out[k])), k
    assert out["rgb_fine"].shape == (sc["n"], 3) and out["weights_coarse"].shape == (sc["n"], 32)


def test_parallel_image_render_occupancy(dev, scene):
    from types import SimpleNamespace as NS
    from codenerf.nerf import OccupancyGrid, PointSampler, parallel_image_render, render_rays
    sc = scene
    rs, ro, rd = _image_rays(dev, sc["g"], 32, 32)
    ps = PointSampler(32, 128, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    cfg = NS(is_distributed=False, gpus=1, nerf=NS(validation=NS(chunksize=400)))
    mdls = {"nerf_coarse": sc["mc"], "nerf_fine": sc["mf"]}
    grid = OccupancyGrid(dev_bits(OC.grid_bits("sphere", 32, radius=0.45), dev), 32, 1.0)
    args = (cfg, sc["g"]["pose"], [sc["g"]["z_s"], sc["g"]["z_t"]], mdls, (rs, ps), embedders(dev), dev)
    for coarse_rgb in (True, False):
        img = parallel_image_render(*args, coarse_rgb=coarse_rgb, occupancy=grid)
        with torch.no_grad():
            ref = render_rays(ro, rd, sc["zs"], sc["zt"], ps, embedders(dev), sc["mc"], sc["mf"], chunk_rows=400,
                              coarse_rgb=coarse_rgb, occupancy=grid)
        assert torch.equal(img, ref["rgb_fine"])
    plain = parallel_image_render(*args)
    assert plain.shape == img.shape and not torch.equal(plain, img)      # the grid did cull


def test_render_occupancy_refuses_gradients(dev, scene):
    from codenerf.nerf import OccupancyGrid, PointSampler, render_rays
    sc = scene
    n = 64
    ps = PointSampler(8, 8, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    grid = OccupancyGrid.full(32, 4.0, dev)
    mc, mf = models(dev)
    for m in (mc, mf):
        m.requires_grad_(False)
    zs = sc["g"]["z_s"].clone().requires_grad_(True)
    args = (sc["ro"][:n], sc["rd"][:n], zs.expand(n, -1), sc["g"]["z_t"].expand(n, -1), ps, embedders(dev), mc, mf)
    with pytest.raises(ValueError):          # a code that requires grad, grad mode on
        render_rays(*args, chunk_rows=50, occupancy=grid)
    mc.requires_grad_(True)
    with pytest.raises(ValueError):          # trainable parameters, grad mode on
        render_rays(sc["ro"][:n], sc["rd"][:n], sc["zs"][:n], sc["zt"][:n], ps, embedders(dev), mc, mf, chunk_rows=50,
                    occupancy=grid)
    with torch.no_grad():                    # the same inputs with grad mode off render
        out = render_rays(*args, chunk_rows=50, occupancy=grid)
    assert "rgb_fine" in out and "rgb_coarse" in out


# ---------------------------------------------------------------- from_density


def test_from_density(dev):
    from codenerf import synthetic
    from codenerf.nerf import OccupancyGrid, density_grid
    m, = models(dev, (0,))
    emb, g, bound = embedders(dev), 32, 1.0
    zs = synthetic.latent_codes(5, 1).to(dev)
    nodes = density_grid(m, emb, zs, g + 1, bound, activated=True)
    threshold = float(nodes.median())         # about half the nodes above it: a grid with structure
    for dilate in (0, 1):
        grid = OccupancyGrid.from_density(m, emb, zs, resolution=g, bound=bound, threshold=threshold, dilate=dilate)
        assert grid.resolution == g and grid.bound == bound
        want = OC.build_bits(nodes.cpu().numpy(), threshold, dilate)
        assert np.array_equal(grid.bits.cpu().numpy().view(np.uint32), want)
        assert 0.0 < grid.occupied_fraction() < 1.0 or dilate
