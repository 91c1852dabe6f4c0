"""Uniform scale in the scene render on the GPU (include/codenerf.h, "Scene composition with uniform scale"):
the four scaled entries against the rule (tests/scene_scale_cases.py), unit scale as the unscaled path bit for
bit, a power-of-two world scale reproduced bit for bit through render_scene, the backwards against float64
autograd, and the buffer and stream harnesses."""
import numpy as np
import pytest
import torch

import buffers as B
import occupancy_cases as OC
import scene_cases as SC
import scene_grad_cases as GC
import scene_scale_cases as XC
import streams as ST
from conftest import margin
from test_gpu_grad import GRAD_RTOL, close, oracle_params
from test_gpu_parity import dev, embedders, load, models  # noqa: F401
from test_gpu_scene import T, _pose_pairs, _same, dev_bits, scene  # noqa: F401
from test_gpu_scene_grad import (LOSS_KEYS, RAYS, UPSTREAM, bits_equal, frozen_models, loss_weights, np_bits_equal,
                                 ray_subset, weighted, within_sum_bound)

pytestmark = pytest.mark.gpu

OUT = ("rgb", "disp", "acc", "weights", "depth", "acc_objects")


def compose(dev, raws, z, rd, scales=None, **kw):
    from codenerf import ops
    return ops.volume_render_compose([T(r, dev) for r in raws], T(z, dev), T(rd, dev),
                                     scales=None if scales is None else [float(v) for v in scales], **kw)


def compose_backward(dev, raws, z, rd, g, scales=None, without=(), **kw):
    from codenerf import ops
    kwargs = {"g_" + key: T(g[key], dev) for key in UPSTREAM if key not in without}
    return ops.volume_render_compose_backward([T(r, dev) for r in raws], T(z, dev), T(rd, dev), **kwargs,
                                              scales=None if scales is None else [float(v) for v in scales], **kw)


# ---------------------------------------------------------------- 1. against the rule


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("r", [1, 5, 67])
def test_object_rays_scaled_bit_exact(dev, r, k):
    """Rows of 13 and (rotation, translation, scale) triples, on rays with -0.0 and 1e4 magnitudes."""
    from codenerf import ops
    ro, rd = SC.pose_rays(r, seed=10 * r + k)
    poses = XC.similarity_poses(k, seed=r + k)
    want_ro, want_rd = XC.object_rays(ro, rd, poses)
    triples = [pair + (float(p[12]),) for pair, p in zip(_pose_pairs(poses[:, :12]), poses)]
    for form in (poses.tolist(), triples):
        got_ro, got_rd = ops.object_rays(T(ro, dev), T(rd, dev), form)
        assert got_ro.shape == (k, r, 3) and got_rd.shape == (k, r, 3)
        assert np_bits_equal(got_ro, want_ro) and np_bits_equal(got_rd, want_rd)
    assert not np.array_equal(want_ro, SC.object_rays(ro, rd, poses[:, :12])[0])       # the scales are seen


@pytest.mark.parametrize("s", XC.S_LIST)
@pytest.mark.parametrize("k", XC.K_LIST)
def test_compose_scaled_against_the_rule(dev, k, s):
    """Against the float64 rule on overlap rows.  The bound is test_gpu_scene.test_overlap_against_the_rule's:
    5e-6 max(1, S / 256), plus (K + 2) 1.2e-7 on rgb for the colour mix; the division of each density by its
    scale is one more rounding, 1.2e-7 relative, of every term of the mix, added to the rgb term: (K + 3) 1.2e-7."""
    r = XC.RAYS
    raws, z, rd = SC.overlap_case(k, r, s, seed=7 * k + s)
    scales = XC.scales_for(k, seed=k + s)
    want = XC.compose(raws, scales, z, rd)
    got = dict(zip(OUT, compose(dev, raws, z, rd, scales)))
    base = 5e-6 * max(1.0, s / 256)
    test = f"scene_scale_overlap[k={k},s={s}]"
    active = XC.mix(raws, scales)[3]
    assert (k == 1 or 0.05 < (active.sum(axis=0) > 1).mean()) and (~active).any()       # the cases do overlap
    for key in ("rgb", "acc", "depth", "weights", "acc_objects", "disp"):
        a, b = got[key].double().cpu().numpy(), want[key]
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin), key
        if key == "disp":        # as test_gpu_scene: compared where the ray is not transparent
            fin = fin & (want["acc"] > 1e-6)
        err = np.abs(a[fin] - b[fin]).max() if fin.any() else 0.0
        margin(test, key, err, base + ((k + 3) * 1.2e-7 if key == "rgb" else 0.0), k=k, s=s)
    # the scales matter: the unscaled weights of the same rows differ (acc itself saturates at 1 on a ray whose
    # last sample, with its 1e10 interval, is active)
    assert not torch.equal(got["weights"], compose(dev, raws, z, rd)[3])


# ---------------------------------------------------------------- 2. unit scale is the old path


@pytest.mark.parametrize("s", XC.S_LIST)
@pytest.mark.parametrize("k", XC.K_LIST)
def test_unit_scale_leaf_ops_are_the_unscaled_bits(dev, k, s):
    from codenerf import ops
    r = XC.RAYS
    raws, z, rd = SC.overlap_case(k, r, s, seed=5 * k + s)
    one = [1.0] * k
    for a, b in zip(compose(dev, raws, z, rd, one), compose(dev, raws, z, rd)):
        assert _same(a, b)
    g = GC.upstream(k, r, s, seed=s + k)
    (u_raws, u_rd), (w_raws, w_rd) = compose_backward(dev, raws, z, rd, g, one), compose_backward(dev, raws, z, rd, g)
    assert all(bits_equal(a, b) for a, b in zip(u_raws, w_raws)) and bits_equal(u_rd, w_rd)
    # with d_scales requested the other outputs do not change
    v_raws, v_rd, d_scales = compose_backward(dev, raws, z, rd, g, one, want_scales=True)
    assert all(bits_equal(a, b) for a, b in zip(v_raws, w_raws)) and bits_equal(v_rd, w_rd) and d_scales.shape == (k,)
    # object rays, forward and backward
    ro, rdo = SC.pose_rays(r, seed=s)
    rigid = SC.poses(k)
    unit = np.concatenate([rigid, np.ones((k, 1), dtype=GC.F)], axis=1)
    for a, b in zip(ops.object_rays(T(ro, dev), T(rdo, dev), unit.tolist()),
                    ops.object_rays(T(ro, dev), T(rdo, dev), rigid.tolist())):
        assert bits_equal(a, b)
    rng = np.random.default_rng(s)
    g_ro, g_rd = (T(rng.standard_normal((k, r, 3)).astype(GC.F), dev) for _ in range(2))
    got = ops.object_rays_backward(g_ro, g_rd, T(ro, dev), T(rdo, dev), unit.tolist())
    ref = ops.object_rays_backward(g_ro, g_rd, T(ro, dev), T(rdo, dev), rigid.tolist())
    assert got[2].shape == (k, 13)
    assert bits_equal(got[0], ref[0]) and bits_equal(got[1], ref[1]) and bits_equal(got[2][:, :12], ref[2])


def two_objects(sc, dev, scale=None, codes=None):
    from codenerf.nerf import OccupancyGrid, SceneObject
    kw = [{}, {}] if scale is None else [dict(scale=scale[0]), dict(scale=scale[1])]
    codes = (sc["zs"], sc["zt"], sc["zs2"], sc["zt2"]) if codes is None else codes
    return [SceneObject(codes[0], codes[1], sc["sphere"], **kw[0]),
            SceneObject(codes[2], codes[3], OccupancyGrid.full(32, 0.35, dev), rotation=SC.rotation([1, 2, 3], 0.5).tolist(),
                        translation=[0.1, 0.0, -0.1], **kw[1])]


def test_unit_scale_render_scene(scene, dev):
    sc = scene
    ref = sc["scene_render"](two_objects(sc, dev))
    got = sc["scene_render"](two_objects(sc, dev, scale=(1.0, 1.0)))
    assert sorted(ref) == sorted(got)
    for key in ref:
        assert _same(got[key], ref[key]), key
    other = sc["scene_render"](two_objects(sc, dev, scale=(1.0, 0.5)))
    assert not _same(other["rgb_fine"], ref["rgb_fine"])


def test_unit_scale_render_scene_autograd(scene, dev):
    """(K, 13) poses with every scale 1 (the scaled entries) against (K, 12) poses (the unscaled ones): the
    forward and every gradient, bit for bit."""
    from codenerf.nerf import render_scene_autograd
    sc = scene
    mc, mf = frozen_models(dev)
    ro0, rd0 = ray_subset(sc)
    rows = np.stack([SC.pose_row(SC.IDENTITY, [0.0, 0.0, 0.0]), SC.pose_row(SC.rotation([1, 2, 3], 0.5), [0.1, 0.0, -0.1])])
    runs = []
    for width in (12, 13):
        codes = [t.clone().requires_grad_(True) for t in (sc["zs"], sc["zt"], sc["zs2"], sc["zt2"])]
        ro, rd = ro0.clone().requires_grad_(True), rd0.clone().requires_grad_(True)
        p = rows if width == 12 else np.concatenate([rows, np.ones((2, 1), dtype=GC.F)], axis=1)
        poses = T(p, dev).requires_grad_(True)
        objects = two_objects(sc, dev, codes=codes)
        out = render_scene_autograd(ro, rd, objects, sc["ps"], sc["emb"], mc, mf, poses=poses)
        weighted(out, loss_weights(LOSS_KEYS, out, seed=2)).backward()
        runs.append((out, [c.grad for c in codes] + [ro.grad, rd.grad, poses.grad[:, :12]], poses.grad))
    (out_a, grads_a, _), (out_b, grads_b, full) = runs
    for key in out_a:
        assert _same(out_a[key].detach(), out_b[key].detach()), key
    assert all(g is not None and bool(g.any()) for g in grads_a)
    assert all(bits_equal(a, b) for a, b in zip(grads_a, grads_b))
    assert full.shape == (2, 13) and bool(full[:, 12].any())


# ---------------------------------------------------------------- 3. scale covariance


COVARIANT = dict(equal=("rgb_coarse", "rgb_fine", "acc_coarse", "acc_fine", "weights_coarse", "acc_objects_coarse",
                        "acc_objects_fine", "ray_hit"),
                 times=("z_fine", "depth_coarse", "depth_fine", "ray_span"), over=("disp_coarse", "disp_fine"))


@pytest.mark.parametrize("mode", ["plain", "span_probes", "sync_free"])
@pytest.mark.parametrize("s", [2.0, 0.5])
def test_power_of_two_world_scale_is_bit_exact(scene, dev, s, mode):
    """Scene A: the objects at scale s, poses (R, t), rays (ro, rd), depths in [s near, s far].  Scene B: scale 1
    at (R, t / s), rays (ro / s, rd), depths in [near, far].  Every operation on the way is IEEE-rounded, so the
    power of two commutes with it: A's maps are B's, its depths s times B's."""
    from codenerf.nerf import PointSampler, SceneObject, render_scene
    sc = scene
    n, near, far, bound = 67, 0.5, 4.0, 1.0
    idx = (torch.arange(n, device=dev) * 15 + 3) % sc["n"]
    ro_b, rd = sc["ro"][idx].contiguous(), sc["rd"][idx].contiguous()
    t_b = [[float(np.float32(v)) for v in t] for t in ([0.1, 0.0, -0.1], [-0.05, 0.1, 0.05])]
    rots = [SC.rotation([1, 2, 3], 0.5).tolist(), SC.rotation([0.3, 1.0, -0.4], 1.1).tolist()]
    codes = [(sc["zs"], sc["zt"]), (sc["zs2"], sc["zt2"])]
    # far lies beyond every grid's cube on every ray: |rd| >= 1, so a sample at far is at least far from the camera
    reach = float(ro_b.norm(dim=1).max()) + 3 ** 0.5 * bound + max(np.linalg.norm(t) for t in t_b)
    assert float(rd.norm(dim=1).min()) >= 1.0 and far - (far - near) / 63 > reach
    g = torch.Generator().manual_seed(int(8 * s))
    t_rand, u = torch.rand(n, 64, generator=g).to(dev), torch.rand(n, 64, generator=g).to(dev)
    kw = dict(plain={}, span_probes=dict(span_probes=64), sync_free=dict(sync_free=True))[mode]

    def render(scale, factor):
        objects = [SceneObject(zs, zt, sc["sphere"], rotation=rot, translation=[factor * v for v in t], scale=scale)
                   for (zs, zt), rot, t in zip(codes, rots, t_b)]
        # span depths are linear in depth, which the sampler calls "lindisp" (quirk Q2)
        ps = PointSampler(64, 64, factor * near, factor * far, "lindisp" if mode == "span_probes" else "lindepth", True,
                          torch.float32, dev)
        with torch.no_grad():
            return render_scene(ro_b * factor, rd, objects, ps, sc["emb"], sc["mc"], sc["mf"], t_rand=t_rand, u=u, **kw)

    a, b = render(s, s), render(1.0, 1.0)
    assert torch.equal(a["z_coarse"], s * b["z_coarse"]), "the coarse depths do not scale: the sampler broke it"
    for out in (a, b):
        # the last coarse sample is culled by every grid, and it is the last fine sample too
        assert not out["weights_coarse"][:, -1].any() and torch.equal(out["z_fine"][:, -1], out["z_coarse"][:, -1])
    assert sorted(a) == sorted(b)
    for key in a:
        assert key == "z_coarse" or any(key in keys for keys in COVARIANT.values()), key
    for key in COVARIANT["equal"]:
        if key in a:
            assert torch.equal(a[key], b[key]), key
    for key in COVARIANT["times"]:
        if key in a:
            assert torch.equal(a[key], s * b[key]), key
    for key in COVARIANT["over"]:
        assert _same(a[key], b[key] / s), key
    assert ("ray_span" in a) == (mode == "span_probes")
    both = (a["acc_objects_fine"] > 1e-3).all(dim=0)
    assert both.any() and 0.05 < float((a["acc_fine"] > 1e-3).float().mean())       # in view, and overlapping


# ---------------------------------------------------------------- 4. backward


@pytest.mark.parametrize("s", XC.S_LIST)
@pytest.mark.parametrize("k", XC.K_LIST)
def test_compose_scaled_backward_against_the_rule(dev, k, s):
    """All six upstream gradients random, against float64 autograd of the scaled rule with frozen active sets.
    d_raws and d_rd within GRAD_RTOL of the largest gradient (test_compose_backward_against_the_rule's bound);
    d_scales[k] within scene_scale_cases.d_scales_bound; inactive rows exactly zero; two runs the same bits."""
    r = XC.RAYS
    raws, z, rd = SC.overlap_case(k, r, s, seed=11 * k + s)
    scales = XC.scales_for(k, seed=2 * k + s)
    g = GC.upstream(k, r, s, seed=s + k)
    want_raws, want_rd, want_scales, model = XC.compose_gradients(raws, scales, z, rd, g)
    d_raws, d_rd, d_scales = compose_backward(dev, raws, z, rd, g, scales, want_scales=True)
    active = XC.mix(raws, scales)[3]
    got = torch.stack(d_raws).cpu()
    err = np.abs(d_scales.double().cpu().numpy() - want_scales)
    bound = XC.d_scales_bound(model, GRAD_RTOL)
    print(f"k={k} s={s}: d_raws err {np.abs(got.double().numpy() - want_raws).max():.3e} of "
          f"{np.abs(want_raws).max():.3e}, d_rd err {np.abs(d_rd.double().cpu().numpy() - want_rd).max():.3e} of "
          f"{np.abs(want_rd).max():.3e}, d_scales err/bound {(err / bound).max():.3e} of {np.abs(want_scales).max():.3e}")
    assert not got[torch.from_numpy(~active)].any()              # an inactive row is exactly zero
    close(got, want_raws, what=f"d raws k={k} s={s}")
    close(d_rd, want_rd, what=f"d rd k={k} s={s}")
    for j in range(k):
        margin(f"scene_scale_d_scales[k={k},s={s}]", f"d_scales[{j}]", err[j], bound[j], k=k, s=s)
    again = compose_backward(dev, raws, z, rd, g, scales, want_scales=True)
    assert all(bits_equal(a, b) for a, b in zip(d_raws, again[0])) and bits_equal(d_rd, again[1])
    assert bits_equal(d_scales, again[2])
    # without d_scales: the same rows
    lean = compose_backward(dev, raws, z, rd, g, scales)
    assert len(lean) == 2 and all(bits_equal(a, b) for a, b in zip(d_raws, lean[0])) and bits_equal(d_rd, lean[1])


def test_compose_scaled_backward_all_inactive(dev):
    """Every slot culled: d_scales is exactly 0, as every row."""
    k, r, s = 3, 21, 65
    raws = np.broadcast_to(SC.EMPTY_ROW, (k, r, s, 4)).copy()
    _, z, rd = SC.overlap_case(k, r, s, seed=1)
    d_raws, d_rd, d_scales = compose_backward(dev, raws, z, rd, GC.upstream(k, r, s, seed=2), [0.5, 2.0, 0.37],
                                              want_scales=True)
    assert not torch.stack(d_raws).any() and not d_rd.any() and not d_scales.any()


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("r", [1, 255, 1000])
def test_object_rays_scaled_backward(dev, r, k):
    """d_ro / d_rd and the 13 pose columns within test_gpu_scene_grad.within_sum_bound of the float64 model, whose
    term counts hold one more rounding for the division of the upstream gradients by the scale."""
    from codenerf import ops
    ro, rd = SC.pose_rays(r, seed=10 * r + k)
    poses = XC.similarity_poses(k, seed=r + k)
    rng = np.random.default_rng(r + 7 * k)
    g_ro, g_rd = rng.standard_normal((k, r, 3)).astype(GC.F), rng.standard_normal((k, r, 3)).astype(GC.F)
    model = XC.object_rays_backward(g_ro, g_rd, ro, rd, poses)
    args = (T(g_ro, dev), T(g_rd, dev), T(ro, dev), T(rd, dev), poses.tolist())
    got = ops.object_rays_backward(*args)
    assert got[0].shape == (r, 3) and got[1].shape == (r, 3) and got[2].shape == (k, 13)
    for t, name in zip(got, ("d_ro", "d_rd", "d_poses")):
        within_sum_bound(t, model, name)
    assert bool(got[2][:, 12].any())
    again = ops.object_rays_backward(*args)
    assert all(bits_equal(a, b) for a, b in zip(got, again))           # a fixed reduction order
    for gro, grd in ((g_ro, None), (None, g_rd)):
        part = XC.object_rays_backward(gro, grd, ro, rd, poses)
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


def pose_parameters(device, dtype):
    """Two objects' (omega, t, log_scale) leaves."""
    values = [([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], float(np.log(1.25))),
              ([0.13363062, 0.26726124, 0.40089187], [0.1, 0.0, -0.1], float(np.log(0.8)))]
    return [tuple(torch.tensor(v, dtype=dtype, device=device, requires_grad=True) for v in row) for row in values]


def test_two_scaled_objects_against_the_oracle(scene, dev):
    """test_gpu_scene_grad's end-to-end oracle extended by scale: two overlapping objects with similarity poses
    from nerf.similarity_pose (scales 1.25 and 0.8), a sphere grid and a full one.  The oracle (float64, on the
    host): the same similarity_pose, R^T (x - t) / s, forward_pass per object on its object-frame rays, the rows
    outside its grid (the lookup on the fp32 points of the fp32 rule's rays) set to EMPTY_ROW, then the scaled
    torch rule at the render's own depths.  d log_scale, d omega, d t, d z_s, d z_t per object within GRAD_RTOL
    (that test's bound), the forward within 1e-4."""
    from oracle import codenerf_oracle as O
    from codenerf.nerf import OccupancyGrid, SceneObject, render_scene_autograd, similarity_pose
    sc = scene
    mc, mf = frozen_models(dev)
    ro, rd = ray_subset(sc)
    grids = [(sc["sphere"], OC.grid_bits("sphere", 32, bound=1.0, radius=0.45), 1.0),
             (OccupancyGrid.full(32, 0.35, dev), OC.grid_bits("full", 32), 0.35)]
    codes = [(sc["zs"].clone().requires_grad_(True), sc["zt"].clone().requires_grad_(True)),
             (sc["zs2"].clone().requires_grad_(True), sc["zt2"].clone().requires_grad_(True))]
    leaves = pose_parameters(dev, torch.float32)
    poses = torch.stack([similarity_pose(*row) for row in leaves])
    objects = [SceneObject(zs, zt, grid[0]) for (zs, zt), grid in zip(codes, grids)]
    out = render_scene_autograd(ro, rd, objects, sc["ps"], sc["emb"], mc, mf, poses=poses)
    weights = loss_weights(LOSS_KEYS, out, seed=2)
    weighted(out, weights).backward()

    emb = O.EmbedCfg()
    params = [{key: v.double() for key, v in oracle_params(m).items()} for m in (mc, mf)]
    ro_h, rd_h = ro.cpu().double(), rd.cpu().double()
    leaves_h = pose_parameters("cpu", torch.float64)
    p_h = torch.stack([similarity_pose(*row) for row in leaves_h])
    c_h = [(zs.detach().cpu().double().requires_grad_(True), zt.detach().cpu().double().requires_grad_(True))
           for zs, zt in codes]
    rot, t, s = p_h[:, :9].reshape(-1, 3, 3), p_h[:, 9:12], p_h[:, 12]
    ro_k = torch.einsum("krj,kji->kri", ro_h[None] - t[:, None, :], rot) / s[:, None, None]
    rd_k = torch.einsum("rj,kji->kri", rd_h, rot) / s[:, None, None]
    ro_f, rd_f = XC.object_rays(ro.cpu().numpy(), rd.cpu().numpy(), poses.detach().cpu().numpy())
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
        res = XC.compose_torch(torch.stack(raws), s, z, rd_h)
        want.update({key + "_" + tag: v for key, v in res.items()})
    assert 0.0 < kept[0] < 1.0 and 0.0 < kept[2] < 1.0 and kept[1] > 0 and kept[3] > 0
    weighted(want, weights).backward()
    assert (out["acc_objects_fine"] > 1e-3).all(dim=0).any()          # the objects do overlap on some ray
    for key in ("rgb_coarse", "acc_coarse", "depth_coarse", "weights_coarse", "acc_objects_coarse", "rgb_fine",
                "acc_fine", "depth_fine", "acc_objects_fine"):
        err = (out[key].detach().double().cpu() - want[key].detach()).abs().max().item()
        print(f"{key}: forward err {err:.3e}")
        assert err <= 1e-4, (key, err)
    for j in range(2):
        pairs = [("d z_s", codes[j][0].grad, c_h[j][0].grad), ("d z_t", codes[j][1].grad, c_h[j][1].grad)]
        if j == 1:      # object 0's omega sits at the Taylor branch's 0: its rotation gradient is checked through object 1
            pairs.append(("d omega", leaves[j][0].grad, leaves_h[j][0].grad))
        pairs += [("d t", leaves[j][1].grad, leaves_h[j][1].grad), ("d log_scale", leaves[j][2].grad, leaves_h[j][2].grad)]
        for name, a, b in pairs:
            print(f"object {j} {name}: err {(a.double().cpu() - b).abs().max().item():.3e} of {b.abs().max().item():.3e}")
            assert float(b.abs().max()) > 0, name
            close(a, b, what=f"object {j} {name}")


def test_two_runs_give_the_same_gradients(scene, dev):
    from codenerf.nerf import OccupancyGrid, SceneObject, render_scene_autograd, similarity_pose
    sc = scene
    mc, mf = frozen_models(dev)
    ro, rd = ray_subset(sc)
    runs = []
    for _ in range(2):
        zs, zt = sc["zs"].clone().requires_grad_(True), sc["zt2"].clone().requires_grad_(True)
        leaves = pose_parameters(dev, torch.float32)
        poses = torch.stack([similarity_pose(*row) for row in leaves])
        objects = [SceneObject(zs, zt, sc["sphere"]), SceneObject(zs, zt, OccupancyGrid.full(32, 0.35, dev))]
        out = render_scene_autograd(ro, rd, objects, sc["ps"], sc["emb"], mc, mf, poses=poses)
        weighted(out, loss_weights(LOSS_KEYS, out, seed=3)).backward()
        runs.append([zs.grad, zt.grad] + [leaf.grad for row in leaves for leaf in row])
    assert all(bits_equal(a, b) for a, b in zip(*runs))


def test_host_scales_are_constants_of_render_scene_autograd(scene, dev):
    """poses=None and (K, 12) poses use the objects' host scales: without gradients render_scene's bits; with
    (K, 12) poses the forward and the twelve rigid columns' gradients of the (K, 13) render at the same scales."""
    from codenerf.nerf import render_scene, render_scene_autograd
    sc = scene
    mc, mf = frozen_models(dev)
    ro, rd = ray_subset(sc)
    objects = two_objects(sc, dev, scale=(1.25, 0.8))
    with torch.no_grad():
        ref = render_scene(ro, rd, objects, sc["ps"], sc["emb"], mc, mf)
        rigid = render_scene(ro, rd, two_objects(sc, dev), sc["ps"], sc["emb"], mc, mf)
    out = render_scene_autograd(ro, rd, objects, sc["ps"], sc["emb"], mc, mf)
    for key in ref:
        assert _same(out[key], ref[key]), key
    assert not _same(ref["rgb_fine"], rigid["rgb_fine"])
    rows = np.stack([SC.pose_row(o.rotation, o.translation) for o in objects])
    runs = []
    for width in (12, 13):
        p = rows if width == 12 else np.concatenate([rows, np.array([[1.25], [0.8]], dtype=GC.F)], axis=1)
        poses = T(p, dev).requires_grad_(True)
        got = render_scene_autograd(ro, rd, objects if width == 12 else two_objects(sc, dev), sc["ps"], sc["emb"], mc, mf,
                                    poses=poses)
        weighted(got, loss_weights(LOSS_KEYS, got, seed=4)).backward()
        runs.append((got, poses.grad))
    (out12, g12), (out13, g13) = runs
    for key in out12:
        assert _same(out12[key].detach(), out13[key].detach()), key
    assert g12.shape == (2, 12) and bool(g12.any()) and bits_equal(g12, g13[:, :12])


def test_adam_on_log_scale_alone(scene, dev):
    """A sanity check, not a rate: three Adam steps on one object's log-scale against a target rendered at another
    scale; the loss goes down every step.  A full grid that holds every sample and the coarse pass alone, so that
    the loss is a differentiable function of the scale (no kept set or resampled depth moves under the step), and
    a step small against the field's finest positional frequency."""
    from codenerf.nerf import OccupancyGrid, SceneObject, render_scene_autograd, similarity_pose
    sc = scene
    mc, mf = frozen_models(dev)
    ro, rd = ray_subset(sc)
    obj = [SceneObject(sc["zs"], sc["zt"], OccupancyGrid.full(32, 8.0, dev))]
    omega, t = torch.zeros(3, device=dev), torch.zeros(3, device=dev)

    def render(log_s):
        return render_scene_autograd(ro, rd, obj, sc["ps"], sc["emb"], mc, mf, coarse_only=True,
                                     poses=similarity_pose(omega, t, log_s)[None])

    with torch.no_grad():
        target = render(torch.tensor(float(np.log(1.4)), device=dev))
    log_s = torch.zeros((), device=dev, requires_grad=True)
    opt = torch.optim.Adam([log_s], lr=5e-4)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        out = render(log_s)
        loss = sum(((out[key] - target[key]) ** 2).mean() for key in ("rgb_coarse", "acc_coarse", "depth_coarse"))
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print("losses", losses, "log_scale", float(log_s))
    assert log_s.grad is not None and float(log_s.grad) != 0.0
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


# ---------------------------------------------------------------- 5. buffers and streams


def four_entries_case(dev, optional):
    """R = 67, S = 65, K = 3 for the four scaled entries -> a runner of the four calls, the optional outputs
    (weights, acc_objects; d_rd, d_scales; d_poses) given or omitted."""
    from codenerf import ops
    r, s, k = 67, 65, 3
    raws, z, rd = SC.overlap_case(k, r, s, seed=3)
    raws[:, :, 0] = (1.0, -1.0, 0.5, 2.0)         # no ray is empty: no NaN disp to expect
    scales = [0.5, 3.1, 0.37]
    g = GC.upstream(k, r, s, seed=6)
    ro, rdo = SC.pose_rays(r, seed=8)
    poses = XC.similarity_poses(k, seed=9).tolist()
    rng = np.random.default_rng(10)
    g_ro, g_rd = (T(rng.standard_normal((k, r, 3)).astype(GC.F), dev) for _ in range(2))
    raws_d, z_d, rd_d = [T(raws[j], dev) for j in range(k)], T(z, dev), T(rd, dev)
    ups = tuple(T(g[key], dev) for key in UPSTREAM)
    ro_d, rdo_d = T(ro, dev), T(rdo, dev)

    def run():
        fwd = ops.volume_render_compose(raws_d, z_d, rd_d, want_weights=optional, want_acc_objects=optional, scales=scales)
        rays = ops.object_rays(ro_d, rdo_d, poses)
        bwd = ops.volume_render_compose_backward(raws_d, z_d, rd_d, *ups, want_rd=optional, scales=scales,
                                                 want_scales=optional)
        rays_b = ops.object_rays_backward(g_ro, g_rd, ro_d, rdo_d, poses, want_poses=optional)
        outs = list(fwd) + list(rays) + list(bwd[0]) + list(bwd[1:]) + list(rays_b)
        return [t for t in outs if t is not None]

    n_allocations = (4 + 2 * optional) + 2 + (k + 3 * optional) + (2 + 2 * optional)
    return run, n_allocations


NAMES = ["volume_render_compose", "object_rays", "volume_render_compose_backward", "object_rays_backward"]


@pytest.mark.parametrize("optional", [True, False])
def test_buffers(dev, optional):
    """The four scaled entries under the poison-fill and guard harness: every output is fully written (no NaN
    survives the poison), nothing is stored past an end, no result depends on the fill."""
    run, n_allocations = four_entries_case(dev, optional)
    logs = {}
    for fill in B.FILLS:
        with B.contracts(fill) as arena:
            outs = run()
        assert arena.n_allocations == n_allocations
        for t in outs:
            assert t.numel() and not bool(torch.isnan(t).any())
        logs[fill] = arena.returns
    assert [name for name, _, _ in logs["zero"]] == NAMES
    B.compare_fills(logs["zero"], logs["poison"])


def test_side_stream_and_capture(dev):
    """Each scaled entry under a side stream is bit-equal to the default-stream run; the forwards, captured alone
    in a graph and replayed, are bit-equal to eager (tests/streams.py)."""
    run, _ = four_entries_case(dev, True)
    run()                                                       # the kernels' first launches
    with B.contracts("poison", log_returns_of=None), ST.plain(record=True) as base:
        run()
    with B.contracts("poison", log_returns_of=None), ST.side_stream(wall_ms=base.wall_ms) as side:
        run()
    assert [r[0] for r in base.returns] == [r[0] for r in side.returns] == NAMES
    assert len(side.slack_ms) == 4 and min(side.slack_ms) > 0
    ST.compare_logs(base.returns, side.returns, "the side-stream run")
    records = [rec for rec in ST.distinct(base.records) if rec.name in NAMES[:2]]
    assert len(records) == 2
    for rec in records:
        ST.capture_replay(rec)
