"""The scene backward's oracles without a device (tests/scene_grad_cases.py): the torch rule against the numpy
rule and against the oracle's volume_render under autograd, the numpy model of cn_occupancy_cull_backward
against torch autograd of the rows it differentiates, and the float64 model of cn_object_rays_backward against
torch autograd of scene_cases' rule."""
import numpy as np
import pytest
import torch

import occupancy_cases as OC
import scene_cases as SC
import scene_grad_cases as GC


@pytest.mark.parametrize("s", [1, 2, 17, 64])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_torch_rule_forward_is_the_numpy_rule(k, s):
    """scene_cases.mix rounds every object's density to fp32 (2^-24 relative) before its float64 arithmetic and
    the torch rule does not: a weight moves by at most 2^-24 (sd + sum of earlier sd) e^-(...) <= 2^-23 of
    itself, a mixed colour by 2^-23, so every per-ray sum (of weights that sum to <= 1, times values <= 2) stays
    within 1e-6; disp = acc / depth scales that by 1 / acc."""
    raws, z, rd = SC.overlap_case(k, 19, s, seed=5 * k + s)
    want = SC.compose(raws, z, rd)
    got = GC.compose_torch(*(torch.from_numpy(a) for a in (raws, z, rd)))
    for key in GC.OUTPUTS:
        a, b = got[key].numpy(), want[key]
        assert a.shape == b.shape, key
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin), key
        tol = 1e-6
        if key == "disp":
            fin = fin & (want["acc"] > 1e-3)
            tol = 1e-6 / np.maximum(want["acc"][fin], 1e-3) ** 2
        assert (np.abs(a[fin] - b[fin]) <= tol).all(), key


@pytest.mark.parametrize("s", [2, 7, 64, 129])
def test_one_object_gradient_is_the_oracle_volume_render(s):
    """K = 1 and every density active: the rule is volume_render, so are its gradients (both in float64)."""
    from oracle import codenerf_oracle as O
    rng = np.random.default_rng(s)
    raw = (rng.standard_normal((1, 23, s, 4)) * 2).astype(SC.F)
    z, rd = SC.depths(23, s, rng)
    assert SC.mix(raw)[3].all()
    g = GC.upstream(1, 23, s, seed=s + 1)
    d_raws, d_rd = GC.compose_gradients(raw, z, rd, g, without=("acc_objects",))
    raw_t = torch.from_numpy(raw[0]).double().requires_grad_(True)
    rd_t = torch.from_numpy(rd).double().requires_grad_(True)
    out = dict(zip(("rgb", "disp", "acc", "weights", "depth"), O.volume_render(raw_t, torch.from_numpy(z).double(), rd_t)))
    GC.compose_loss(out, g, without=("acc_objects",)).backward()
    for got, ref in ((d_raws[0], raw_t.grad.numpy()), (d_rd, rd_t.grad.numpy())):
        assert np.abs(got - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    # the object's mask is acc: its gradient counts as g_acc's
    with_mask, _ = GC.compose_gradients(raw, z, rd, dict(g, acc=g["acc"] * 0, acc_objects=g["acc"][None]),
                                        without=())
    plain, _ = GC.compose_gradients(raw, z, rd, g, without=("acc_objects",))
    assert np.abs(with_mask - plain).max() <= 1e-9 * max(1.0, np.abs(plain).max())


def test_frozen_active_sets():
    """An inactive row (the culled slot) gets exactly zero gradient, and with two or more active objects the
    density gradient carries the colour-mix and share terms (it differs from the one-object row's)."""
    raws, z, rd = SC.overlap_case(3, 11, 9, seed=2)
    g = GC.upstream(3, 11, 9, seed=3)
    d_raws, _ = GC.compose_gradients(raws, z, rd, g)
    active = SC.mix(raws)[3]
    assert not d_raws[~active].any() and (~active).any()
    assert (np.abs(d_raws[active]).max(axis=-1) > 0).mean() > 0.9


@pytest.mark.parametrize("chunk_rows", [37, 16, 7])
@pytest.mark.parametrize("s", [1, 5, 64, 130])
def test_cull_backward_model_is_autograd_of_the_rows(s, chunk_rows):
    """pts[j] = ro[r] + rd[r] z[r][s_j] and vdir[j] = rd[Q1 ray of j] in torch float64 under autograd, against
    the float32 model: to 1e-6 relative to the largest gradient (sequential fp32 sums of at most 2 S <= 260 terms of magnitude ~1: an
    error of a few 2^-24 of the running sum)."""
    n = 37
    ro, rd, z, _, keep = GC.cull_case("sphere", n, s, seed=s + chunk_rows)
    assert 0 < keep.sum() < keep.size or s == 1
    rng = np.random.default_rng(s)
    m = int(keep.sum())
    g_pts, g_vdir = rng.standard_normal((m, 3)).astype(GC.F), rng.standard_normal((m, 3)).astype(GC.F)
    d_ro, d_rd = GC.cull_backward(g_pts, g_vdir, z, keep, chunk_rows)
    ro_t = torch.from_numpy(ro).double().requires_grad_(True)
    rd_t = torch.from_numpy(rd).double().requires_grad_(True)
    idx = torch.from_numpy(np.nonzero(keep.reshape(-1))[0])
    pts = (ro_t[:, None, :] + rd_t[:, None, :] * torch.from_numpy(z).double()[:, :, None]).reshape(-1, 3)[idx]
    vdir = rd_t[torch.from_numpy(OC.q1_ray(n, s, chunk_rows).reshape(-1))[idx]]
    loss = (pts * torch.from_numpy(g_pts).double()).sum() + (vdir * torch.from_numpy(g_vdir).double()).sum()
    if m:
        loss.backward()
    ref_ro = ro_t.grad.numpy() if ro_t.grad is not None else np.zeros((n, 3))
    ref_rd = rd_t.grad.numpy() if rd_t.grad is not None else np.zeros((n, 3))
    scale = max(1.0, np.abs(ref_ro).max(), np.abs(ref_rd).max())
    assert np.abs(d_ro - ref_ro).max() <= 1e-6 * scale
    assert np.abs(d_rd - ref_rd).max() <= 1e-6 * scale
    # either gradient alone, and none kept
    only_p = GC.cull_backward(g_pts, None, z, keep, chunk_rows)
    only_v = GC.cull_backward(None, g_vdir, z, keep, chunk_rows)
    assert np.array_equal(only_p[0], d_ro) and not only_v[0].any()
    none = GC.cull_backward(None, None, z, np.zeros_like(keep), chunk_rows)
    assert not none[0].any() and not none[1].any()


def test_gather_model():
    rng = np.random.default_rng(0)
    keep = rng.random((5, 7)) < 0.4
    g_raw = rng.standard_normal((5, 7, 4)).astype(GC.F)
    got = GC.gather(g_raw, keep)
    assert got.shape == (int(keep.sum()), 4)
    k = np.nonzero(keep.reshape(-1))[0]
    assert np.array_equal(got, g_raw.reshape(-1, 4)[k]) and (np.diff(k) > 0).all()


@pytest.mark.parametrize("k", [1, 3, 8])
def test_object_rays_backward_model_is_autograd_of_the_rule(k):
    """The float64 model against torch autograd of R^T (x - t) in float64."""
    n = 29
    rng = np.random.default_rng(k)
    ro, rd = rng.standard_normal((n, 3)).astype(GC.F), rng.standard_normal((n, 3)).astype(GC.F)
    poses = SC.poses(k)
    g_ro, g_rd = rng.standard_normal((k, n, 3)).astype(GC.F), rng.standard_normal((k, n, 3)).astype(GC.F)
    model = GC.object_rays_backward(g_ro, g_rd, ro, rd, poses)
    ro_t = torch.from_numpy(ro).double().requires_grad_(True)
    rd_t = torch.from_numpy(rd).double().requires_grad_(True)
    p_t = torch.from_numpy(poses).double().requires_grad_(True)
    rot, t = p_t[:, :9].reshape(k, 3, 3), p_t[:, 9:]
    ro_k = torch.einsum("krj,kji->kri", ro_t[None] - t[:, None, :], rot)
    rd_k = torch.einsum("rj,kji->kri", rd_t, rot)
    # the forward is scene_cases.object_rays
    want_ro, want_rd = SC.object_rays(ro, rd, poses)
    assert np.abs(ro_k.detach().numpy() - want_ro).max() <= 1e-5 and np.abs(rd_k.detach().numpy() - want_rd).max() <= 1e-5
    ((ro_k * torch.from_numpy(g_ro).double()).sum() + (rd_k * torch.from_numpy(g_rd).double()).sum()).backward()
    for name, ref in (("d_ro", ro_t.grad), ("d_rd", rd_t.grad), ("d_poses", p_t.grad)):
        assert np.abs(model[name] - ref.numpy()).max() <= 1e-12 * max(1.0, ref.abs().max().item()), name
        assert (model["abs_" + name] >= np.abs(model[name]) - 1e-12).all(), name
    only = GC.object_rays_backward(None, g_rd, ro, rd, poses)
    assert not only["d_ro"].any() and not only["d_poses"][:, 9:].any()


def test_rigid_pose_on_the_host():
    """Plain torch ops: the identity with finite gradients at omega = 0, scene_cases.rotation elsewhere (fp32:
    a few 2^-24 of entries <= 1), differentiable through the small-angle switch."""
    from codenerf.nerf import rigid_pose
    omega = torch.zeros(3, requires_grad=True)
    t = torch.tensor([0.5, -1.0, 2.0], requires_grad=True)
    pose = rigid_pose(omega, t)
    assert pose.shape == (12,) and torch.equal(pose[:9].reshape(3, 3), torch.eye(3)) and torch.equal(pose[9:], t.detach())
    (pose * torch.arange(1.0, 13.0)).sum().backward()
    # d R / d omega at 0 is the skew generator: the weights 1..9 give (w8 - w6, w3 - w7, w4 - w2)
    assert torch.allclose(omega.grad, torch.tensor([2.0, -4.0, 2.0])) and torch.equal(t.grad, torch.tensor([10.0, 11.0, 12.0]))
    for axis, angle in (([1.0, -2.0, 0.5], 0.4), ([0.3, 1.0, -0.4], 2.1), ([0.0, 0.0, 1.0], 1e-3), ([1.0, 1.0, 0.0], 5e-5)):
        a = np.asarray(axis) / np.linalg.norm(axis)
        got = rigid_pose(torch.from_numpy((a * angle).astype(GC.F)), torch.zeros(3))
        assert np.abs(got[:9].reshape(3, 3).numpy() - SC.rotation(axis, angle)).max() <= 5e-7, (axis, angle)
    w = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda v: rigid_pose(v, torch.zeros(3, dtype=torch.float64)), (w,))
