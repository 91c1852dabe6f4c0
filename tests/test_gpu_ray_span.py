"""cn_sample_span on the device against the numpy rule of tests/ray_span_cases.py, bit for bit; the op's buffer,
stream and capture contracts; and the span renders (render_rays / render_scene with ``span_probes``)."""
import numpy as np
import pytest
import torch

import buffers as B
import occupancy_cases as OC
import ray_span_cases as S
import streams as ST
from test_gpu_parity import dev, embedders, load, models  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def dev_grid(grid, dev):
    """A numpy Grid as the (bits, resolution, bound) triple ops.sample_span takes."""
    return T(np.asarray(grid.bits).view(np.int32), dev), grid.g, grid.bound


def _same(a, b):
    """Bitwise equal values, NaN in the same places (disp is NaN where acc is 0)."""
    if not a.is_floating_point():
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def check(dev, ro, rd, grids, near, far, p, nc, t_rand=None):
    """The device's three outputs equal the rule's, bit for bit -> the rule's (z, span, probe_range)."""
    from codenerf import ops
    want = S.sample_span(ro, rd, grids, near, far, p, nc, t_rand)
    dg = dev_grid(grids, dev) if isinstance(grids, S.Grid) else [dev_grid(g, dev) for g in grids]
    got = ops.sample_span(T(ro, dev), T(rd, dev), dg, near, far, p, nc, None if t_rand is None else T(t_rand, dev))
    r = ro.shape[-2]
    assert got[0].shape == (r, nc) and got[1].shape == (r, 2) and got[2].shape == (r, 2)
    assert got[0].dtype == got[1].dtype == torch.float32 and got[2].dtype == torch.int32
    for name, g, w in zip(("z", "span", "probe_range"), got, want):
        g = g.cpu().numpy()
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), \
            (name, int((g.view(np.uint32) != w.view(np.uint32)).sum()), g[:2], w[:2])
    return want


# ---------------------------------------------------------------- 1. the op against the rule


@pytest.mark.parametrize("kind", ["full", "empty", "half", "sphere"])
@pytest.mark.parametrize("nc", [2, 3, 64, 65, 200])
@pytest.mark.parametrize("r", [1, 5, 67])
def test_one_grid_bit_exact(dev, r, nc, kind):
    """A ragged last block (R), the lane loop's second pass and its tail (Nc), with and without t_rand, every P."""
    ro, rd = S.camera_rays(r, seed=100 * r + nc)
    grid = S.Grid.of(kind, 32, radius=0.5)
    t_rand = np.random.default_rng(nc).random((r, nc)).astype(F)
    t_rand[:, ::3] = S.TAU_MAX                                   # ties with the next sample
    for p, tr in ((64, None), (128, t_rand), (1024, None), (1024, t_rand)):
        _, _, pr = check(dev, ro, rd, grid, 0.5, 2.1, p, nc, tr)
    if kind in ("full", "half") and r > 1:
        assert (pr[:, 0] >= 0).any()
    if kind == "empty":
        assert np.all(pr == -1)


@pytest.mark.parametrize("p", [64, 128, 1024])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_posed_objects_bit_exact(dev, k, p):
    """Distinct poses, grids of different G, bound and kind: the union's span."""
    _, _, _, grids, ro_k, rd_k = S.scene_case(k, 67, seed=k)
    t_rand = np.random.default_rng(k + p).random((67, 65)).astype(F)
    _, _, pr = check(dev, ro_k, rd_k, grids, 0.4, 3.0, p, 65, t_rand)
    check(dev, ro_k, rd_k, grids, 0.4, 3.0, p, 3)
    hit = pr[:, 0] >= 0
    assert hit.any() and (k > 1 or (~hit).any())


def test_scene_rays_come_from_object_rays(dev):
    """The rays the scene case states in numpy are ops.object_rays' bits, so the union above is the one
    render_scene probes."""
    from codenerf import ops
    ro, rd, poses, _, ro_k, rd_k = S.scene_case(3, 67, seed=3)
    got_ro, got_rd = ops.object_rays(T(ro, dev), T(rd, dev), poses)
    assert np.array_equal(got_ro.cpu().numpy(), ro_k) and np.array_equal(got_rd.cpu().numpy(), rd_k)


def test_probes_on_cell_faces(dev):
    ro, rd, near, far, p = S.face_case()
    _, _, pr = check(dev, ro, rd, S.Grid.of("full"), near, far, p, 4)
    assert pr[0].tolist() == [0, 31] and pr[1].tolist() == [1, 32]
    _, _, pr = check(dev, ro, rd, S.Grid.of("half"), near, far, p, 4)
    assert pr[0].tolist() == [0, 15] and pr[1].tolist() == [17, 32]


def test_nan_direction_is_a_miss(dev):
    ro, rd = S.camera_rays(5, seed=9)
    rd[1, 2] = np.nan
    rd[3] = np.nan
    _, span, pr = check(dev, ro, rd, S.Grid.of("full"), 0.5, 2.1, 64, 7)
    assert np.all(pr[[1, 3]] == -1) and np.all(span[[1, 3]] == np.array([0.5, 2.1], dtype=F))
    assert np.all(pr[[0, 2, 4], 0] >= 0)


# ---------------------------------------------------------------- 2. the op's contracts


def contract_case(dev):
    _, _, _, grids, ro_k, rd_k = S.scene_case(3, 67, seed=21)
    t_rand = np.random.default_rng(5).random((67, 65)).astype(F)
    args = (T(ro_k, dev), T(rd_k, dev), [dev_grid(g, dev) for g in grids], 0.4, 3.0, 128, 65, T(t_rand, dev))
    want = S.sample_span(ro_k, rd_k, grids, 0.4, 3.0, 128, 65, t_rand)
    return args, want


def test_buffers(dev):
    """Under the poison fill and the guards at ragged sizes: every output is fully written (no NaN, no stale
    integer survives), nothing is stored past an end, no result depends on the fill."""
    from codenerf import ops
    args, want = contract_case(dev)
    logs = {}
    for fill in B.FILLS:
        with B.contracts(fill) as arena:
            out = ops.sample_span(*args)
        assert arena.n_allocations == 3
        for g, w in zip(out, want):
            assert np.array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32))
        logs[fill] = arena.returns
    assert [name for name, _, _ in logs["zero"]] == ["sample_span"]
    B.compare_fills(logs["zero"], logs["poison"])


def test_side_stream_and_capture(dev):
    """The op under a side stream is bit-equal to the default-stream run, and captured alone in a graph and
    replayed it is bit-equal to eager (tests/streams.py): it is capturable."""
    from codenerf import ops
    args, _ = contract_case(dev)
    ops.sample_span(*args)                                       # the kernel's first launch
    with B.contracts("poison", log_returns_of=None), ST.plain(record=True) as base:
        ops.sample_span(*args)
    with B.contracts("poison", log_returns_of=None), ST.side_stream(wall_ms=base.wall_ms) as side:
        ops.sample_span(*args)
    assert [r[0] for r in base.returns] == [r[0] for r in side.returns] == ["sample_span"]
    assert len(side.slack_ms) == 1 and min(side.slack_ms) > 0
    ST.compare_logs(base.returns, side.returns, "the side-stream run")
    records = ST.distinct(base.records)
    assert len(records) == 1
    ST.capture_replay(records[0])


def test_the_cull_never_keeps_a_free_end(dev):
    """ops.occupancy_cull on the span depths never keeps the last sample of a ray with last < P - 1: its depth
    has an unoccupied probe's bits, and the cull forms the same point from them."""
    from codenerf import ops
    _, _, _, grids, ro_k, rd_k = S.scene_case(3, 67, seed=33)
    p, nc = 128, 9
    t_rand = np.random.default_rng(1).random((67, nc)).astype(F)
    z, _, pr = ops.sample_span(T(ro_k, dev), T(rd_k, dev), [dev_grid(g, dev) for g in grids], 0.4, 3.0, p, nc,
                               T(t_rand, dev))
    pr = pr.cpu().numpy()
    free_end = (pr[:, 0] >= 0) & (pr[:, 1] < p - 1)
    assert free_end.sum() >= 10
    kept_any = False
    for k, g in enumerate(grids):
        bits, res, bound = dev_grid(g, dev)
        count, index, _, _, _, _ = ops.occupancy_cull(T(ro_k[k], dev), T(rd_k[k], dev), z, 67, bits, res, bound,
                                                      want_code=False)
        kept = np.zeros(67 * nc, dtype=bool)
        kept[index.cpu().numpy()] = True
        kept = kept.reshape(67, nc)
        kept_any = kept_any or kept.any()
        assert not kept[free_end, nc - 1].any(), k
    assert kept_any


# ---------------------------------------------------------------- 3. the renders


SHARED = ("rgb_coarse", "disp_coarse", "acc_coarse", "weights_coarse", "depth_coarse", "z_coarse", "rgb_fine",
          "disp_fine", "acc_fine", "depth_fine", "z_fine")
PROBES = 128


@pytest.fixture(scope="module")
def scene(dev):
    """50 rays of the render_small.npz camera (a stride through its 32 x 32 image), the synthetic models, an
    8 + 8 unperturbed sampler linear in depth, a G = 32 sphere grid."""
    from codenerf import synthetic
    from codenerf.nerf import OccupancyGrid, PointSampler, RaySampler
    g = load("render_small.npz", dev)
    k = torch.tensor([[28.0, 0, 16.0, 0], [0, 28.0, 16.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    rs = RaySampler(32, 32, k, sample_size=1024, device=dev, datatype=torch.float32)
    ro, rd = (t.reshape(-1, 3)[7::20][:50].contiguous() for t in rs.get_bundle(g["pose"]))
    mc, mf = models(dev)
    return dict(ro=ro, rd=rd, n=50, mc=mc, mf=mf, zs=g["z_s"], zt=g["z_t"], emb=embedders(dev),
                zs2=synthetic.latent_codes(11, 1).to(dev), zt2=synthetic.latent_codes(12, 1).to(dev),
                ps=PointSampler(8, 8, 0.8, 1.8, "lindisp", False, torch.float32, dev),
                sphere=OccupancyGrid(T(OC.grid_bits("sphere", 32, bound=1.0, radius=0.45).view(np.int32), dev), 32, 1.0))


def recomposed(sc, objects, ro_k, rd_k, compose):
    """The span render from its parts: ops.sample_span's depths, each object's culled field, the volume render
    (``compose``: ops.volume_render_compose over the objects, else ops.volume_render of the one), ops.sample_pdf."""
    from codenerf import ops
    from codenerf.nerf import _culled_field
    ps, n = sc["ps"], sc["n"]

    def render(models, z):
        raws = [_culled_field(m, sc["emb"], rd_k[k], zs, zt, n, ro_k[k], z, grid, False)
                for k, ((zs, zt, grid), m) in enumerate(zip(objects, models))]
        if compose:
            return ops.volume_render_compose(raws, z, sc["rd"])
        return ops.volume_render(raws[0], z, sc["rd"]) + (None,)

    with torch.no_grad():
        z_c, span, pr = ops.sample_span(ro_k, rd_k, [grid for _, _, grid in objects], ps.near, ps.far, PROBES,
                                        ps.num_samples_coarse)
        rgb_c, disp_c, acc_c, w_c, depth_c, obj_c = render([sc["mc"]] * len(objects), z_c)
        _, z_f = ops.sample_pdf(sc["ro"], sc["rd"], w_c[..., 1:-1], z_c, ps.num_samples_fine, ps.u_lin, want_pts=False)
        rgb_f, disp_f, acc_f, _, depth_f, obj_f = render([sc["mf"]] * len(objects), z_f)
    out = {"rgb_coarse": rgb_c, "disp_coarse": disp_c, "acc_coarse": acc_c, "weights_coarse": w_c,
           "depth_coarse": depth_c, "z_coarse": z_c, "rgb_fine": rgb_f, "disp_fine": disp_f, "acc_fine": acc_f,
           "depth_fine": depth_f, "z_fine": z_f, "ray_span": span, "ray_hit": pr[:, 0] >= 0}
    if compose:
        out.update({"acc_objects_coarse": obj_c, "acc_objects_fine": obj_f})
    return out, pr


def span_render(sc, **kw):
    from codenerf.nerf import render_rays
    n = sc["n"]
    with torch.no_grad():
        return render_rays(sc["ro"], sc["rd"], sc["zs"].expand(n, -1), sc["zt"].expand(n, -1), sc["ps"], sc["emb"],
                           sc["mc"], sc["mf"], chunk_rows=None, occupancy=sc["sphere"], **kw)


def test_render_rays_is_its_recomposition(scene):
    sc = scene
    out = span_render(sc, span_probes=PROBES)
    ref, _ = recomposed(sc, [(sc["zs"], sc["zt"], sc["sphere"])], sc["ro"][None], sc["rd"][None], compose=False)
    assert sorted(out) == sorted(ref) == sorted(SHARED + ("ray_span", "ray_hit"))
    for key in out:
        assert _same(out[key], ref[key]), key
    hit = out["ray_hit"]
    assert out["ray_hit"].dtype == torch.bool and 0.1 < float(hit.float().mean()) < 1.0    # hits and misses
    plain = span_render(sc)
    assert sorted(plain) == sorted(SHARED)
    # a miss keeps the sampler's range; a hit's span is narrower, and its depths differ from the plain ones
    whole = torch.tensor([sc["ps"].near, sc["ps"].far], device=hit.device)
    assert torch.equal(out["ray_span"][~hit], whole.expand(int((~hit).sum()), 2))
    assert bool(((out["ray_span"][hit, 1] - out["ray_span"][hit, 0]) < 0.999 * (sc["ps"].far - sc["ps"].near)).all())
    assert not torch.equal(out["z_coarse"][hit], plain["z_coarse"][hit])
    assert (out["acc_fine"][hit] > 0).any()


def test_scene_of_one_identity_object_is_render_rays(scene):
    from codenerf.nerf import SceneObject, render_scene
    sc = scene
    ref = span_render(sc, span_probes=PROBES)
    with torch.no_grad():
        out = render_scene(sc["ro"], sc["rd"], [SceneObject(sc["zs"], sc["zt"], sc["sphere"])], sc["ps"], sc["emb"],
                           sc["mc"], sc["mf"], span_probes=PROBES)
    assert sorted(out) == sorted(tuple(ref) + ("acc_objects_coarse", "acc_objects_fine"))
    for key in ref:
        assert _same(out[key], ref[key]), key


def test_two_translated_objects_give_the_union_span(scene):
    from codenerf import ops
    from codenerf.nerf import SceneObject, render_scene
    sc = scene
    t_a, t_b = [0.0, 0.0, -0.3], [0.15, 0.1, 0.35]
    a = SceneObject(sc["zs"], sc["zt"], sc["sphere"], translation=t_a)
    b = SceneObject(sc["zs2"], sc["zt2"], sc["sphere"], translation=t_b)
    with torch.no_grad():
        out = render_scene(sc["ro"], sc["rd"], [a, b], sc["ps"], sc["emb"], sc["mc"], sc["mf"], span_probes=PROBES)
    ro_k, rd_k = ops.object_rays(sc["ro"], sc["rd"], [(a.rotation, t_a), (b.rotation, t_b)])
    ref, pr = recomposed(sc, [(sc["zs"], sc["zt"], sc["sphere"]), (sc["zs2"], sc["zt2"], sc["sphere"])], ro_k, rd_k,
                         compose=True)
    assert sorted(out) == sorted(ref)
    for key in out:
        assert _same(out[key], ref[key]), key
    # the union: first / last over the two objects' own probe ranges
    ps = sc["ps"]
    one = [ops.sample_span(ro_k[k], rd_k[k], sc["sphere"], ps.near, ps.far, PROBES, ps.num_samples_coarse)[2]
           for k in range(2)]
    hit_a, hit_b = one[0][:, 0] >= 0, one[1][:, 0] >= 0
    both = hit_a & hit_b
    assert both.any() and (hit_a ^ hit_b).any()
    assert torch.equal(pr[both, 0], torch.minimum(one[0][both, 0], one[1][both, 0]))
    assert torch.equal(pr[both, 1], torch.maximum(one[0][both, 1], one[1][both, 1]))
    assert torch.equal(pr[hit_a & ~hit_b], one[0][hit_a & ~hit_b]) and torch.equal(pr[~hit_a & hit_b], one[1][~hit_a & hit_b])
    assert torch.equal(out["ray_hit"], hit_a | hit_b)


def test_value_errors(scene):
    from codenerf.nerf import PointSampler, SceneObject, render_rays, render_scene
    sc = scene
    n = sc["n"]
    args = (sc["ro"], sc["rd"], sc["zs"].expand(n, -1), sc["zt"].expand(n, -1))
    rest = (sc["emb"], sc["mc"], sc["mf"])
    disparity = PointSampler(8, 8, 0.8, 1.8, "lindepth", False, torch.float32, sc["ro"].device)
    objects = [SceneObject(sc["zs"], sc["zt"], sc["sphere"])]
    with torch.no_grad():
        with pytest.raises(ValueError, match="occupancy"):
            render_rays(*args, sc["ps"], *rest, span_probes=PROBES)
        for bad in (0, 100, 32, 1088, -64, 128.0, True):
            with pytest.raises(ValueError, match="span_probes"):
                render_rays(*args, sc["ps"], *rest, occupancy=sc["sphere"], span_probes=bad)
            with pytest.raises(ValueError, match="span_probes"):
                render_scene(sc["ro"], sc["rd"], objects, sc["ps"], *rest, span_probes=bad)
        with pytest.raises(ValueError, match="lindisp"):
            render_rays(*args, disparity, *rest, occupancy=sc["sphere"], span_probes=PROBES)
        with pytest.raises(ValueError, match="lindisp"):
            render_scene(sc["ro"], sc["rd"], objects, disparity, *rest, span_probes=PROBES)
        with pytest.raises(ValueError, match="lindisp"):
            disparity.sample_span(sc["ro"], sc["rd"], sc["sphere"])
