"""The scaled scene rule's oracles (tests/scene_scale_cases.py) checked against themselves and against the
unscaled ones, without a device: unit scale is the unscaled rule, a power-of-two world scale commutes with the
rule, the autograd oracle agrees with central differences, and nerf.similarity_pose."""
import numpy as np
import pytest
import torch

import scene_cases as SC
import scene_grad_cases as GC
import scene_scale_cases as XC

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_unit_scale_is_the_unscaled_rule(k):
    ro, rd = SC.pose_rays(67, seed=k)
    rigid = SC.poses(k)
    unit = np.concatenate([rigid, np.ones((k, 1), dtype=F)], axis=1)
    for a, b in zip(XC.object_rays(ro, rd, unit), SC.object_rays(ro, rd, rigid)):
        assert np.array_equal(bits(a), bits(b))
    raws, z, rdc = SC.overlap_case(k, 19, 33, seed=5 + k)
    want, got = SC.compose(raws, z, rdc), XC.compose(raws, np.ones(k, dtype=F), z, rdc)
    for key in want:
        assert np.array_equal(want[key], got[key], equal_nan=True), key


def test_object_rays_keep_the_ray_parameter():
    """ro_out + z rd_out is the world point in the object's canonical frame: R^T (ro + z rd - t) / s."""
    ro, rd = SC.pose_rays(67, seed=2)
    ro, rd = np.clip(ro, -3, 3), np.clip(rd, -3, 3)          # ordinary magnitudes: a value check
    poses = XC.similarity_poses(3, seed=1)
    ro_k, rd_k = XC.object_rays(ro, rd, poses)
    for z in (0.0, 0.8, 2.5):
        for k, p in enumerate(poses.astype(np.float64)):
            world = ro.astype(np.float64) + z * rd.astype(np.float64)
            want = (world - p[9:12]) @ p[:9].reshape(3, 3) / p[12]
            got = ro_k[k].astype(np.float64) + z * rd_k[k].astype(np.float64)
            assert np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("factor", [2.0, 0.5])
def test_power_of_two_world_scale_commutes_with_the_rule(factor):
    """Every object's scale and every depth times a power of two: the densities divide by it exactly, sigma delta
    is unchanged, so weights, colours and masks are equal and depth is the factor times the other."""
    k = 3
    raws, z, rd = SC.overlap_case(k, 19, 33, seed=8)
    scales = XC.scales_for(k, seed=3)
    a = XC.compose(raws, scales * F(factor), z * F(factor), rd)
    b = XC.compose(raws, scales, z, rd)
    for key in ("rgb", "acc", "weights", "acc_objects"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["depth"], factor * b["depth"])
    assert np.array_equal(a["disp"], b["disp"] / factor, equal_nan=True)


def test_chord_opacity_does_not_depend_on_size():
    """One object of constant density over a chord of length s: acc is the same at every scale s."""
    n = 64
    raw = np.zeros((1, 1, n, 4), dtype=F)
    raw[..., 3] = 1.7
    accs = []
    for s in (0.5, 1.0, 3.1):
        z = (1.0 + s * np.linspace(0.0, 1.0, n))[None].astype(F)
        raws = raw.copy()
        raws[0, 0, -1] = SC.EMPTY_ROW                          # the chord ends: nothing in the 1e10 interval
        accs.append(XC.compose(raws, [s], z, np.array([[0.0, 0.0, 1.0]], dtype=F))["acc"][0])
    assert np.abs(np.array(accs) - accs[1]).max() <= 1e-6 and 0.1 < accs[1] < 0.9


@pytest.mark.parametrize("k,s", [(1, 7), (3, 17)])
def test_autograd_oracle_against_central_differences(k, s):
    r = 5
    raws, z, rd = SC.overlap_case(k, r, s, seed=3 * k + s)
    scales = XC.scales_for(k, seed=k)
    g = GC.upstream(k, r, s, seed=s)
    d_raws, d_rd, d_scales, model = XC.compose_gradients(raws, scales, z, rd, g)
    assert np.abs(d_scales - model["d_scales_from_terms"]).max() <= 1e-12 * max(1.0, np.abs(d_scales).max())
    active = XC.mix(raws, scales)[3]
    assert not d_raws[~active].any()

    def loss(sc):
        out = XC.compose_torch(torch.from_numpy(raws), torch.from_numpy(np.asarray(sc)), torch.from_numpy(z),
                               torch.from_numpy(rd))
        return float(GC.compose_loss(out, g))

    for j in range(k):
        h = 1e-6 * float(scales[j])
        up, down = scales.astype(np.float64), scales.astype(np.float64)
        up[j] += h
        down[j] -= h
        fd = (loss(up) - loss(down)) / (2 * h)
        assert abs(fd - d_scales[j]) <= 1e-5 * max(1.0, abs(d_scales[j])), (j, fd, d_scales[j])
    # scale 1: the unscaled oracle's gradients
    w_raws, w_rd = GC.compose_gradients(raws, z, rd, g)
    u_raws, u_rd, _, _ = XC.compose_gradients(raws, np.ones(k, dtype=F), z, rd, g)
    assert np.array_equal(w_raws, u_raws) and np.array_equal(w_rd, u_rd)


def test_object_rays_backward_model_against_autograd():
    r, k = 11, 3
    ro, rd = SC.pose_rays(r, seed=4)
    ro, rd = np.clip(ro, -3, 3), np.clip(rd, -3, 3)
    poses = XC.similarity_poses(k, seed=2)
    rng = np.random.default_rng(6)
    g_ro, g_rd = rng.standard_normal((k, r, 3)).astype(F), rng.standard_normal((k, r, 3)).astype(F)
    model = XC.object_rays_backward(g_ro, g_rd, ro, rd, poses)
    ro_t, rd_t, p_t = (torch.from_numpy(a).double().requires_grad_(True) for a in (ro, rd, poses))
    rot, t, s = p_t[:, :9].reshape(-1, 3, 3), p_t[:, 9:12], p_t[:, 12]
    ro_k = torch.einsum("krj,kji->kri", ro_t[None] - t[:, None, :], rot) / s[:, None, None]
    rd_k = torch.einsum("rj,kji->kri", rd_t, rot) / s[:, None, None]
    ((ro_k * torch.from_numpy(g_ro).double()).sum() + (rd_k * torch.from_numpy(g_rd).double()).sum()).backward()
    for name, ref in (("d_ro", ro_t.grad), ("d_rd", rd_t.grad), ("d_poses", p_t.grad)):
        assert np.abs(model[name] - ref.numpy()).max() <= 1e-12 * max(1.0, float(ref.abs().max())), name
    assert model["d_poses"].shape == (k, 13) and model["terms_d_poses"].shape == (k, 13)
    # unit scale: the rigid model's first 12 columns
    unit = np.concatenate([poses[:, :12], np.ones((k, 1), dtype=F)], axis=1)
    a, b = XC.object_rays_backward(g_ro, g_rd, ro, rd, unit), GC.object_rays_backward(g_ro, g_rd, ro, rd, poses[:, :12])
    assert np.array_equal(a["d_poses"][:, :12], b["d_poses"]) and np.array_equal(a["d_ro"], b["d_ro"])


def test_similarity_pose():
    from codenerf.nerf import rigid_pose, similarity_pose
    omega = torch.tensor([0.3, -0.2, 0.5], requires_grad=True)
    t = torch.tensor([0.5, -1.0, 2.0], requires_grad=True)
    log_s = torch.tensor(0.7, requires_grad=True)
    pose = similarity_pose(omega, t, log_s)
    assert pose.shape == (13,) and torch.equal(pose[:12], rigid_pose(omega, t))
    assert torch.equal(pose[12], log_s.exp())
    (pose * torch.arange(1.0, 14.0)).sum().backward()
    assert torch.allclose(log_s.grad, 13.0 * log_s.exp().detach())
    assert bool(torch.isfinite(omega.grad).all()) and torch.equal(t.grad, torch.tensor([10.0, 11.0, 12.0]))
    one = similarity_pose(torch.zeros(3), torch.zeros(3), torch.zeros(1))          # a (1,) log-scale too
    assert torch.equal(one, torch.cat([torch.eye(3).reshape(9), torch.zeros(3), torch.ones(1)]))
