"""The scene render's backward on the device: cn_volume_render_compose_backward, cn_object_rays_backward,
cn_occupancy_gather and cn_occupancy_cull_backward against the oracles of tests/scene_grad_cases.py and against
cn_volume_render_backward's own bits, their buffers and streams, and render_scene_autograd end to end."""
import itertools

import numpy as np
import pytest
import torch

import buffers as B
import occupancy_cases as OC
import scene_cases as SC
import scene_grad_cases as GC
import streams as ST
from test_gpu_grad import GRAD_RTOL, close, oracle_params
from test_gpu_parity import dev, embedders, load, models  # noqa: F401
from test_gpu_scene import T, _same, dev_bits, scene  # noqa: F401

pytestmark = pytest.mark.gpu

UPSTREAM = ("rgb", "disp", "acc", "weights", "depth", "acc_objects")


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def np_bits_equal(got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), np.asarray(want, dtype=GC.F).view(np.uint32))


def compose_backward(dev, raws, z, rd, g, without=(), **kw):
    from codenerf import ops
    kwargs = {"g_" + key: T(g[key], dev) for key in UPSTREAM if key not in without}
    return ops.volume_render_compose_backward([T(r, dev) for r in raws], T(z, dev), T(rd, dev), **kwargs, **kw)


# ---------------------------------------------------------------- 1. compose backward against the float64 rule


@pytest.mark.parametrize("s", [2, 7, 64, 65, 129, 300])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_compose_backward_against_the_rule(dev, k, s):
    """All six upstream gradients random, against the float64 autograd of the rule with frozen active sets, within
    the project's bound for volume_render_backward against the same kind of oracle (GRAD_RTOL of the largest
    gradient)."""
    r = 53
    raws, z, rd = SC.overlap_case(k, r, s, seed=11 * k + s)
    g = GC.upstream(k, r, s, seed=s + k)
    want_raws, want_rd = GC.compose_gradients(raws, z, rd, g)
    d_raws, d_rd = compose_backward(dev, raws, z, rd, g)
    active = SC.mix(raws)[3]
    assert (~active).any() and (k == 1 or (active.sum(axis=0) > 1).mean() > 0.05)      # the cases do overlap
    got = torch.stack(d_raws).cpu()
    print(f"k={k} s={s}: d_raws err {np.abs(got.double().numpy() - want_raws).max():.3e} of "
          f"{np.abs(want_raws).max():.3e}, d_rd err {np.abs(d_rd.double().cpu().numpy() - want_rd).max():.3e} of "
          f"{np.abs(want_rd).max():.3e}")
    assert not got[torch.from_numpy(~active)].any()              # an inactive row is exactly zero
    close(got, want_raws, what=f"d raws k={k} s={s}")
    close(d_rd, want_rd, what=f"d rd k={k} s={s}")


@pytest.mark.parametrize("missing", UPSTREAM + ("all",))
def test_compose_backward_null_gradients(dev, missing):
    """Each upstream gradient NULL in turn is that gradient zero; all NULL gives zeros."""
    k, r, s = 3, 53, 65
    raws, z, rd = SC.overlap_case(k, r, s, seed=4)
    g = GC.upstream(k, r, s, seed=5)
    without = UPSTREAM if missing == "all" else (missing,)
    want_raws, want_rd = GC.compose_gradients(raws, z, rd, g, without=without)
    d_raws, d_rd = compose_backward(dev, raws, z, rd, g, without=without)
    if missing == "all":
        assert not torch.stack(d_raws).any() and not d_rd.any()
        return
    close(torch.stack(d_raws), want_raws, what=f"d raws without g_{missing}")
    close(d_rd, want_rd, what=f"d rd without g_{missing}")
    # d rd is optional, and can be added into a running sum
    again, none = compose_backward(dev, raws, z, rd, g, without=without, want_rd=False)
    assert none is None and all(bits_equal(a, b) for a, b in zip(again, d_raws))
    into = torch.full((r, 3), 0.5, device=dev)
    _, summed = compose_backward(dev, raws, z, rd, g, without=without, d_rd_into=into)
    assert summed is into and torch.equal(into, 0.5 + d_rd)


# ---------------------------------------------------------------- 2. compose backward, exact cases


@pytest.mark.parametrize("r", [3, 53])
@pytest.mark.parametrize("s", [1, 2, 7, 64, 65, 128, 192, 300, 512])
def test_one_object_is_volume_render_backward(dev, r, s):
    """K = 1 without g_acc_objects: cn_volume_render_backward's bits (S = 64 and 128 are that kernel's FULL
    instances, 192 and up its 64-lane ones)."""
    from codenerf import ops
    rng = np.random.default_rng(100 * s + r)
    raw = (rng.standard_normal((r, s, 4)) * 2).astype(GC.F)
    raw[0, :, 3] = 30.0                                            # the softplus threshold branch
    z, rd = SC.depths(r, s, rng)
    g = GC.upstream(1, r, s, seed=s)
    args = (T(raw, dev), T(z, dev), T(rd, dev))
    ref_raw, ref_rd = ops.volume_render_backward(*args, T(g["rgb"], dev), T(g["disp"], dev), T(g["acc"], dev),
                                                 T(g["weights"], dev), T(g["depth"], dev))
    d_raws, d_rd = compose_backward(dev, [raw], z, rd, g, without=("acc_objects",))
    assert bits_equal(d_raws[0], ref_raw) and bits_equal(d_rd, ref_rd)
    if s == 1:
        assert not d_raws[0].any() and not d_rd.any()


@pytest.mark.parametrize("s", [17, 64, 192])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_exclusive_activity_backward(dev, k, s):
    """At most one active object per sample: its rows are cn_volume_render_backward's of the tensor holding each
    sample's active row, bit for bit; every other row is exactly zero; the order of the objects only permutes
    the gradients.  (d rd is compared by value: the all-empty ray's is a sum of signed zeros.)"""
    from codenerf import ops
    r = 37
    raws, z, rd, selected, owner = SC.exclusive_case(k, r, s, seed=31 * k + s)
    g = GC.upstream(k, r, s, seed=k + s)
    ref_raw, ref_rd = ops.volume_render_backward(T(selected, dev), T(z, dev), T(rd, dev), T(g["rgb"], dev),
                                                 T(g["disp"], dev), T(g["acc"], dev), T(g["weights"], dev),
                                                 T(g["depth"], dev))
    d_raws, d_rd = compose_backward(dev, raws, z, rd, g, without=("acc_objects",))
    got = torch.stack(d_raws)
    own = T(owner, dev)
    for j in range(k):
        mine = own == j
        assert mine.any() and bits_equal(got[j][mine], ref_raw[mine]), j
        assert not got[j][~mine].any(), j
    assert torch.equal(d_rd, ref_rd)
    perms = list(itertools.permutations(range(k))) if k <= 3 else \
        [tuple(reversed(range(k))), (3, 0, 7, 1, 6, 2, 5, 4), (1, 2, 3, 4, 5, 6, 7, 0)]
    for perm in perms:
        alt, alt_rd = compose_backward(dev, raws[list(perm)], z, rd, g, without=("acc_objects",))
        assert torch.equal(torch.stack(alt), got[list(perm)]) and torch.equal(alt_rd, d_rd), perm


# ---------------------------------------------------------------- 3. object rays backward


def object_rays_case(r, k, seed):
    ro, rd = SC.pose_rays(r, seed=seed)
    rng = np.random.default_rng(seed + 1)
    return ro, rd, SC.poses(k), rng.standard_normal((k, r, 3)).astype(GC.F), rng.standard_normal((k, r, 3)).astype(GC.F)


def within_sum_bound(got, model, name):
    """|got - exact| <= (n_terms + 4) 2^-24 sum |term|: an n-term fp32 sum in any order, plus the rounding of each
    product and of the subtraction ro - t."""
    err = np.abs(got.double().cpu().numpy() - model[name])
    bound = (model["terms_" + name] + 4) * 2.0 ** -24 * model["abs_" + name]
    assert (err <= bound).all(), (name, float((err - bound).max()))


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("r", [1, 255, 1000])
def test_object_rays_backward(dev, r, k):
    from codenerf import ops
    ro, rd, poses, g_ro, g_rd = object_rays_case(r, k, seed=10 * r + k)
    model = GC.object_rays_backward(g_ro, g_rd, ro, rd, poses)
    args = (T(g_ro, dev), T(g_rd, dev), T(ro, dev), T(rd, dev), poses.tolist())
    got = ops.object_rays_backward(*args)
    assert got[0].shape == (r, 3) and got[1].shape == (r, 3) and got[2].shape == (k, 12)
    for t, name in zip(got, ("d_ro", "d_rd", "d_poses")):
        within_sum_bound(t, model, name)
    again = ops.object_rays_backward(*args)
    assert all(bits_equal(a, b) for a, b in zip(got, again))           # a fixed reduction order
    # either upstream gradient alone, a subset of the outputs, and the rays' gradients added into running sums
    for gro, grd in ((g_ro, None), (None, g_rd)):
        part = GC.object_rays_backward(gro, grd, ro, rd, poses)
        out = ops.object_rays_backward(None if gro is None else T(gro, dev), None if grd is None else T(grd, dev),
                                       *args[2:])
        for t, name in zip(out, ("d_ro", "d_rd", "d_poses")):
            within_sum_bound(t, part, name)
    only_poses = ops.object_rays_backward(*args, want_ro=False, want_rd=False)
    assert only_poses[0] is None and only_poses[1] is None and bits_equal(only_poses[2], got[2])
    no_poses = ops.object_rays_backward(*args, want_poses=False)
    assert no_poses[2] is None and bits_equal(no_poses[0], got[0]) and bits_equal(no_poses[1], got[1])
    into = (torch.full((r, 3), 0.25, device=dev), torch.full((r, 3), -2.0, device=dev))
    ops.object_rays_backward(*args, want_poses=False, ray_into=into)
    assert torch.equal(into[0], 0.25 + got[0]) and torch.equal(into[1], -2.0 + got[1])


# ---------------------------------------------------------------- 4. the compact rows' backwards


def culled(dev, kind, r, s, chunk_rows, seed):
    from codenerf import ops
    ro, rd, z, bits, keep = GC.cull_case(kind, r, s, seed)
    count, _, _, _, _, state = ops.occupancy_cull(T(ro, dev), T(rd, dev), T(z, dev), chunk_rows, dev_bits(bits, dev), 32,
                                                  1.0, want_code=False)
    assert count == int(keep.sum())
    return z, keep, count, state


@pytest.mark.parametrize("kind", ["sphere", "empty", "full"])
@pytest.mark.parametrize("chunk_rows", [37, 16, 7])
@pytest.mark.parametrize("s", [1, 5, 64, 130])
def test_gather_and_cull_backward_bit_exact(dev, s, chunk_rows, kind):
    from codenerf import ops
    r = 37
    z, keep, count, state = culled(dev, kind, r, s, chunk_rows, seed=s + chunk_rows)
    assert {"empty": count == 0, "full": count > 0, "sphere": 0 < count < r * s or s == 1}[kind]
    rng = np.random.default_rng(s)
    g_raw = rng.standard_normal((r, s, 4)).astype(GC.F)
    g_pts, g_vdir = rng.standard_normal((count, 3)).astype(GC.F), rng.standard_normal((count, 3)).astype(GC.F)
    got = ops.occupancy_gather(T(g_raw, dev), state)
    assert np_bits_equal(got, GC.gather(g_raw, keep))
    want_ro, want_rd = GC.cull_backward(g_pts, g_vdir, z, keep, chunk_rows)
    d_ro, d_rd = ops.occupancy_cull_backward(T(g_pts, dev), T(g_vdir, dev), T(z, dev), chunk_rows, state)
    assert np_bits_equal(d_ro, want_ro) and np_bits_equal(d_rd, want_rd)
    for gp, gv in ((g_pts, None), (None, g_vdir)):
        want = GC.cull_backward(gp, gv, z, keep, chunk_rows)
        out = ops.occupancy_cull_backward(None if gp is None else T(gp, dev), None if gv is None else T(gv, dev),
                                          T(z, dev), chunk_rows, state)
        assert np_bits_equal(out[0], want[0]) and np_bits_equal(out[1], want[1])
    only_rd = ops.occupancy_cull_backward(T(g_pts, dev), T(g_vdir, dev), T(z, dev), chunk_rows, state, want_ro=False)
    assert only_rd[0] is None and np_bits_equal(only_rd[1], want_rd)


# ---------------------------------------------------------------- 5. buffers and streams


def four_ops_case(dev):
    """Ragged sizes for all four entries -> a runner of the four calls (the cull that leaves the state runs
    here, outside any harness: its padded workspace is not an output)."""
    from codenerf import ops
    r, s, k = 67, 65, 3
    raws, z, rd = SC.overlap_case(k, r, s, seed=3)
    g = GC.upstream(k, r, s, seed=6)
    ro, rdo, poses, g_ro, g_rd = object_rays_case(r, k, seed=8)
    zc, keep, count, state = culled(dev, "sphere", r, s, 16, seed=9)
    rng = np.random.default_rng(10)
    dev_args = dict(
        compose=([T(raws[j], dev) for j in range(k)], T(z, dev), T(rd, dev)) + tuple(T(g[key], dev) for key in UPSTREAM),
        rays=(T(g_ro, dev), T(g_rd, dev), T(ro, dev), T(rdo, dev), poses.tolist()),
        gather=(T(rng.standard_normal((r, s, 4)).astype(GC.F), dev), state),
        cull=(T(rng.standard_normal((count, 3)).astype(GC.F), dev), T(rng.standard_normal((count, 3)).astype(GC.F), dev),
              T(zc, dev), 16, state))

    def run():
        d_raws, d_rd = ops.volume_render_compose_backward(*dev_args["compose"])
        rays = ops.object_rays_backward(*dev_args["rays"])
        compact = ops.occupancy_gather(*dev_args["gather"])
        d_ro, d_rd2 = ops.occupancy_cull_backward(*dev_args["cull"])
        return list(d_raws) + [d_rd, *rays, compact, d_ro, d_rd2]

    return run, k


def test_buffers(dev):
    """All four entries under the poison-fill and guard harness: every output is fully written (no NaN survives
    the poison), nothing is stored past an end, no result depends on the fill."""
    run, k = four_ops_case(dev)
    logs = {}
    for fill in B.FILLS:
        with B.contracts(fill) as arena:
            outs = run()
        assert arena.n_allocations == (k + 1) + 4 + 1 + 2      # d_raws + d_rd; d_ro, d_rd, d_poses, workspace; ...
        for t in outs:
            assert t.numel() and not bool(torch.isnan(t).any())
        logs[fill] = arena.returns
    assert [name for name, _, _ in logs["zero"]] == ["volume_render_compose_backward", "object_rays_backward",
                                                     "occupancy_gather", "occupancy_cull_backward"]
    B.compare_fills(logs["zero"], logs["poison"])


def test_side_stream_and_capture(dev):
    """Each new op under a side stream is bit-equal to the default-stream run, and captured alone in a graph and
    replayed it is bit-equal to eager (tests/streams.py)."""
    run, _ = four_ops_case(dev)
    run()                                                       # the kernels' first launches
    with B.contracts("poison", log_returns_of=None), ST.plain(record=True) as base:
        run()
    with B.contracts("poison", log_returns_of=None), ST.side_stream(wall_ms=base.wall_ms) as side:
        run()
    assert [r[0] for r in base.returns] == [r[0] for r in side.returns] == \
        ["volume_render_compose_backward", "object_rays_backward", "occupancy_gather", "occupancy_cull_backward"]
    assert len(side.slack_ms) == 4 and min(side.slack_ms) > 0
    ST.compare_logs(base.returns, side.returns, "the side-stream run")
    records = ST.distinct(base.records)
    assert len(records) == 4
    for rec in records:
        ST.capture_replay(rec)


# ---------------------------------------------------------------- 6. render_scene_autograd


RAYS = 48
LOSS_KEYS = ("rgb_coarse", "rgb_fine", "depth_fine", "acc_objects_fine")


def frozen_models(dev):
    mc, mf = models(dev)
    for m in (mc, mf):
        m.requires_grad_(False)
    return mc, mf


def ray_subset(sc):
    idx = (torch.arange(RAYS, device=sc["ro"].device) * 21 + 5) % sc["n"]          # spread over the image
    return sc["ro"][idx].contiguous(), sc["rd"][idx].contiguous()


def loss_weights(keys, out, seed):
    g = torch.Generator().manual_seed(seed)
    return {key: torch.randn(out[key].shape, generator=g) for key in keys}


def weighted(out, weights):
    return sum((out[key] * w.to(out[key].device).to(out[key].dtype)).sum() for key, w in weights.items())


def test_one_identity_object_is_render_rays(scene, dev):
    """One identity-posed object under a full grid that holds every sample: the forward entries are bitwise
    render_rays' with gradients on (the same kernel template in points mode: the compact rows' property), and
    d z_s, z_t, ro, rd are within GRAD_RTOL of render_rays' own backward."""
    from codenerf.nerf import OccupancyGrid, SceneObject, render_rays, render_scene_autograd
    sc = scene
    mc, mf = frozen_models(dev)
    ro0, rd0 = ray_subset(sc)
    grid = OccupancyGrid.full(32, 8.0, dev)
    grads, outs = [], []
    for which in ("plain", "scene"):
        zs, zt = sc["zs"].clone().requires_grad_(True), sc["zt"].clone().requires_grad_(True)
        ro, rd = ro0.clone().requires_grad_(True), rd0.clone().requires_grad_(True)
        if which == "plain":
            out = render_rays(ro, rd, zs.expand(RAYS, -1), zt.expand(RAYS, -1), sc["ps"], sc["emb"], mc, mf,
                              chunk_rows=None)
        else:
            out = render_scene_autograd(ro, rd, [SceneObject(zs, zt, grid)], sc["ps"], sc["emb"], mc, mf)
            pts = OC.ray_points(ro0.cpu().numpy(), rd0.cpu().numpy(), out["z_fine"].cpu().numpy())
            assert OC.lookup(pts, OC.grid_bits("full", 32), 32, 8.0).all()          # the grid holds every sample
        weights = loss_weights(("rgb_coarse", "rgb_fine", "depth_fine", "acc_fine"), out, seed=1)
        weighted(out, weights).backward()
        grads.append((zs.grad, zt.grad, ro.grad, rd.grad))
        outs.append(out)
    plain, got = outs
    for key in plain:
        assert _same(got[key].detach(), plain[key].detach()), key
    assert torch.equal(got["acc_objects_fine"][0], got["acc_fine"])
    assert 0.05 < float((got["acc_fine"] > 1e-3).float().mean())                    # the object is in view
    for name, a, b in zip(("d z_s", "d z_t", "d ro", "d rd"), grads[1], grads[0]):
        assert a is not None and b is not None and float(b.abs().max()) > 0, name
        print(f"{name}: err {(a - b).abs().max().item():.3e} of {b.abs().max().item():.3e}")
        close(a, b, what=name)


def torch_object_rays(ro, rd, poses):
    """scene_cases.object_rays' rule in torch: R^T (x - t) -> (K, R, 3) each."""
    rot, t = poses[:, :9].reshape(-1, 3, 3), poses[:, 9:]
    return (torch.einsum("krj,kji->kri", ro[None] - t[:, None, :], rot), torch.einsum("rj,kji->kri", rd, rot))


def test_two_overlapping_objects_against_the_oracle(scene, dev):
    """Two overlapping posed objects with different codes, a sphere grid and a full one.  The oracle (float64, on
    the host): forward_pass per object on its object-frame rays, the rows outside its grid (occupancy_cases'
    lookup on the fp32 points) set to EMPTY_ROW, then the torch rule; the depths are the render's own (they are
    constants of both).  d z_s, d z_t per object and d poses within GRAD_RTOL, the forward within 1e-4."""
    from oracle import codenerf_oracle as O
    from codenerf.nerf import OccupancyGrid, SceneObject, render_scene_autograd
    sc = scene
    mc, mf = frozen_models(dev)
    ro, rd = ray_subset(sc)
    pose_rows = np.stack([SC.pose_row(SC.IDENTITY, [0.0, 0.0, 0.0]),
                          SC.pose_row(SC.rotation([1, 2, 3], 0.5), [0.1, 0.0, -0.1])])
    grids = [(sc["sphere"], OC.grid_bits("sphere", 32, bound=1.0, radius=0.45), 1.0),
             (OccupancyGrid.full(32, 0.35, dev), OC.grid_bits("full", 32), 0.35)]
    codes = [(sc["zs"].clone().requires_grad_(True), sc["zt"].clone().requires_grad_(True)),
             (sc["zs2"].clone().requires_grad_(True), sc["zt2"].clone().requires_grad_(True))]
    poses = T(pose_rows, dev).requires_grad_(True)
    objects = [SceneObject(zs, zt, grid[0]) for (zs, zt), grid in zip(codes, grids)]
    out = render_scene_autograd(ro, rd, objects, sc["ps"], sc["emb"], mc, mf, poses=poses)
    weights = loss_weights(LOSS_KEYS, out, seed=2)
    weighted(out, weights).backward()

    # the oracle
    emb = O.EmbedCfg()
    params = [{key: v.double() for key, v in oracle_params(m).items()} for m in (mc, mf)]
    ro_h, rd_h = ro.cpu().double(), rd.cpu().double()
    p_h = torch.from_numpy(pose_rows).double().requires_grad_(True)
    c_h = [(zs.detach().cpu().double().requires_grad_(True), zt.detach().cpu().double().requires_grad_(True))
           for zs, zt in codes]
    ro_k, rd_k = torch_object_rays(ro_h, rd_h, p_h)
    ro_f, rd_f = SC.object_rays(ro.cpu().numpy(), rd.cpu().numpy(), pose_rows)     # the fp32 rays the grids see
    want, kept = {}, []
    for tag, p in (("coarse", params[0]), ("fine", params[1])):
        z = out["z_" + tag].detach().cpu()
        raws = []
        for j in range(2):
            pts = ro_k[j][:, None, :] + rd_k[j][:, None, :] * z.double()[:, :, None]
            raw = O.forward_pass(p, emb, rd_k[j], pts, c_h[j][0].expand(RAYS, -1), c_h[j][1].expand(RAYS, -1))
            keep = OC.lookup(OC.ray_points(ro_f[j], rd_f[j], z.numpy()), grids[j][1], 32, grids[j][2])
            kept.append(keep.mean())
            raws.append(torch.where(torch.from_numpy(keep)[..., None], raw, torch.from_numpy(SC.EMPTY_ROW).double()))
        res = GC.compose_torch(torch.stack(raws), z, rd_h)
        want.update({key + "_" + tag: v for key, v in res.items()})
    assert 0.0 < kept[0] < 1.0 and 0.0 < kept[2] < 1.0             # the sphere object: both branches
    assert kept[1] > 0 and kept[3] > 0
    weighted(want, weights).backward()
    both = (out["acc_objects_fine"] > 1e-3).all(dim=0)
    assert both.any()                                               # the objects do overlap on some ray
    for key in ("rgb_coarse", "acc_coarse", "depth_coarse", "weights_coarse", "acc_objects_coarse", "rgb_fine",
                "acc_fine", "depth_fine", "acc_objects_fine"):
        err = (out[key].detach().double().cpu() - want[key].detach()).abs().max().item()
        print(f"{key}: forward err {err:.3e}")
        assert err <= 1e-4, (key, err)
    for j in range(2):
        for name, a, b in (("d z_s", codes[j][0].grad, c_h[j][0].grad), ("d z_t", codes[j][1].grad, c_h[j][1].grad)):
            print(f"object {j} {name}: err {(a.double().cpu() - b).abs().max().item():.3e} of {b.abs().max().item():.3e}")
            close(a, b, what=f"object {j} {name}")
    print(f"d poses: err {(poses.grad.double().cpu() - p_h.grad).abs().max().item():.3e} of "
          f"{p_h.grad.abs().max().item():.3e}")
    close(poses.grad, p_h.grad, what="d poses")


def test_two_runs_give_the_same_gradients(scene, dev):
    """Every backward kernel of the path reduces in a fixed order."""
    from codenerf.nerf import OccupancyGrid, SceneObject, render_scene_autograd
    sc = scene
    mc, mf = frozen_models(dev)
    ro, rd = ray_subset(sc)
    runs = []
    for _ in range(2):
        zs, zt = sc["zs"].clone().requires_grad_(True), sc["zt2"].clone().requires_grad_(True)
        poses = T(np.stack([SC.pose_row(SC.rotation([1, 2, 3], 0.5), [0.1, 0.0, -0.1])] * 2), dev).requires_grad_(True)
        objects = [SceneObject(zs, zt, sc["sphere"]), SceneObject(zs, zt, OccupancyGrid.full(32, 0.35, dev))]
        out = render_scene_autograd(ro, rd, objects, sc["ps"], sc["emb"], mc, mf, poses=poses)
        weighted(out, loss_weights(LOSS_KEYS, out, seed=3)).backward()
        runs.append((zs.grad, zt.grad, poses.grad))
    assert all(bits_equal(a, b) for a, b in zip(*runs))


def test_render_scene_autograd_refusals(scene, dev):
    from codenerf.nerf import SceneObject, render_scene_autograd
    sc = scene
    ro, rd = ray_subset(sc)
    zs = sc["zs"].clone().requires_grad_(True)
    objects = [SceneObject(zs, sc["zt"], sc["sphere"])]
    mc, mf = frozen_models(dev)
    out = render_scene_autograd(ro, rd, objects, sc["ps"], sc["emb"], mc, mf, coarse_only=True)
    assert "rgb_fine" not in out and out["rgb_coarse"].requires_grad
    mf.requires_grad_(True)
    with pytest.raises(ValueError, match="frozen"):                 # trainable parameters
        render_scene_autograd(ro, rd, objects, sc["ps"], sc["emb"], mc, mf)
    mc3, mf3 = models(dev, precision="bf16x3")
    for m in (mc3, mf3):
        m.requires_grad_(False)
    with pytest.raises(ValueError, match="f32"):                    # not the fp32 field
        render_scene_autograd(ro, rd, objects, sc["ps"], sc["emb"], mc3, mf3)
    mc, mf = frozen_models(dev)
    with pytest.raises(ValueError, match="1..8"):                   # more than 8 objects
        render_scene_autograd(ro, rd, objects * 9, sc["ps"], sc["emb"], mc, mf)
    with pytest.raises(ValueError, match="poses"):
        render_scene_autograd(ro, rd, objects, sc["ps"], sc["emb"], mc, mf, poses=torch.zeros(2, 12, device=dev))


def test_rigid_pose(dev):
    from codenerf.nerf import rigid_pose
    omega = torch.zeros(3, device=dev, requires_grad=True)
    t = torch.tensor([0.5, -1.0, 2.0], device=dev, requires_grad=True)
    pose = rigid_pose(omega, t)
    assert pose.shape == (12,) and torch.equal(pose[:9].reshape(3, 3), torch.eye(3, device=dev))
    assert torch.equal(pose[9:], t.detach())
    (pose * torch.arange(1.0, 13.0, device=dev)).sum().backward()
    assert bool(torch.isfinite(omega.grad).all()) and bool(torch.isfinite(t.grad).all())
    # d R / d omega at 0 is the skew generator: the weights 1..9 give (w[7] - w[5], w[2] - w[6], w[3] - w[1])
    assert torch.allclose(omega.grad.cpu(), torch.tensor([8.0 - 6.0, 3.0 - 7.0, 4.0 - 2.0]))
    for axis, angle in (([1.0, -2.0, 0.5], 0.4), ([0.3, 1.0, -0.4], 2.1), ([0.0, 0.0, 1.0], 1e-3)):
        a = np.asarray(axis) / np.linalg.norm(axis)
        got = rigid_pose(T((a * angle).astype(GC.F), dev), torch.zeros(3, device=dev))
        assert np.abs(got[:9].reshape(3, 3).cpu().numpy() - SC.rotation(axis, angle)).max() <= 5e-7
