"""Scene composition without a device: the numpy rule of tests/scene_cases.py against the oracle and
against its own stated consequences, and SceneObject's validation."""
import itertools

import numpy as np
import pytest
import torch

import scene_cases as SC


@pytest.mark.parametrize("s", [1, 2, 17, 64, 192])
def test_one_object_is_the_oracle_volume_render(s):
    """K = 1: the rule is volume_render.  The oracle is torch in fp32 and the rule float64, so they agree to
    the project's bound for an fp32 volume render against the oracle (test_volume_render_sizes: 5e-6 for
    S <= 256), which covers the oracle's own rounding."""
    from oracle import codenerf_oracle as O
    rng = np.random.default_rng(s)
    raw = (rng.standard_normal((1, 23, s, 4)) * 2).astype(SC.F)
    z, rd = SC.depths(23, s, rng)
    got = SC.compose(raw, z, rd)
    if s == 1:      # the reference's sample-free ray
        assert got["weights"].shape == (23, 0) and not got["rgb"].any() and np.isnan(got["disp"]).all()
        return
    ref = O.volume_render(torch.from_numpy(raw[0]), torch.from_numpy(z), torch.from_numpy(rd))
    for key, b in zip(("rgb", "disp", "acc", "weights", "depth"), ref):
        b = b.numpy().astype(np.float64)
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(got[key]), fin), key
        assert np.abs(got[key][fin] - b[fin]).max() <= 5e-6, key
    assert np.array_equal(got["acc_objects"][0], got["acc"])


def test_identity_pose_is_a_bitwise_no_op():
    """The identity returns the rays' bits: x * 1 is x, x * 0 is +-0 and adding a zero to a non-zero x
    leaves it.  (A -0.0 component may come back as +0.0, which the header says; these rays have none.)"""
    rng = np.random.default_rng(5)
    ro = rng.standard_normal((67, 3)).astype(SC.F)
    rd = rng.standard_normal((67, 3)).astype(SC.F)
    ro[3] = (9876.543, -10001.25, 1.0e4)
    ro_k, rd_k = SC.object_rays(ro, rd, SC.pose_row(SC.IDENTITY, [0, 0, 0])[None])
    assert np.array_equal(ro_k[0].view(np.uint32), ro.view(np.uint32))
    assert np.array_equal(rd_k[0].view(np.uint32), rd.view(np.uint32))


def test_object_rays_keep_the_ray_parameter():
    """ro' + z rd' is the world point ro + z rd in the object's frame: R (ro' + z rd') + t gives it back
    (to fp32 rounding of coordinates of size ~1e4), and the half turn leaves rd's squares, so |rd|'s bits."""
    ro, rd = SC.pose_rays(67, 1)
    p = SC.poses(8)
    ro_k, rd_k = SC.object_rays(ro, rd, p)
    for k in range(8):
        rot, t = p[k, :9].reshape(3, 3).astype(np.float64), p[k, 9:].astype(np.float64)
        for zval in (0.0, 1.5):
            world = ro.astype(np.float64) + zval * rd.astype(np.float64)
            back = (ro_k[k].astype(np.float64) + zval * rd_k[k].astype(np.float64)) @ rot.T + t
            assert np.abs(back - world).max() <= 8 * 2.0 ** -24 * 3.0e4
    assert np.array_equal(rd_k[1] * rd_k[1], rd * rd)


@pytest.mark.parametrize("k", [2, 3])
def test_exclusive_samples_do_not_see_the_object_order(k):
    """At most one active object per sample: every permutation of the objects gives identical results (the
    acc_objects rows permuted with them), equal to the render of the selected rows alone."""
    raws, z, rd, selected, owner = SC.exclusive_case(k, 19, 21, seed=k)
    base = SC.compose(raws, z, rd)
    alone = SC.compose(selected[None], z, rd)
    for key in ("rgb", "disp", "acc", "weights", "depth"):
        assert np.array_equal(base[key], alone[key], equal_nan=True), key
    for perm in itertools.permutations(range(k)):
        got = SC.compose(raws[list(perm)], z, rd)
        for key in ("rgb", "disp", "acc", "weights", "depth"):
            assert np.array_equal(got[key], base[key], equal_nan=True), (perm, key)
        assert np.array_equal(got["acc_objects"], base["acc_objects"][list(perm)]), perm
    # the all-empty ray
    assert not base["rgb"][-1].any() and base["acc"][-1] == 0 and base["depth"][-1] == 0
    assert np.isnan(base["disp"][-1]) and not base["acc_objects"][:, -1].any()
    # an object owns what its samples weigh
    for j in range(k):
        assert np.allclose(base["acc_objects"][j], (base["weights"] * (owner == j)).sum(axis=1), rtol=0, atol=1e-14)


def test_instance_masks_sum_to_acc():
    """The shares of a sample sum to 1, so the instance masks sum to acc.  With one active object per
    sample that holds to float64 rounding.  Where objects overlap the shares are sigma_k / sigma with the
    fp32 sum sigma, whose K - 1 additions of positive terms are each within 2^-24 relative: the shares sum
    to 1 within (K - 1) 2^-24, and the masks to acc within that fraction of it."""
    raws, z, rd, _, _ = SC.exclusive_case(3, 19, 33, seed=7)
    got = SC.compose(raws, z, rd)
    assert np.abs(got["acc_objects"].sum(axis=0) - got["acc"]).max() <= 1e-14
    for k in (2, 8):
        raws, z, rd = SC.overlap_case(k, 19, 33, seed=k)
        got = SC.compose(raws, z, rd)
        err = np.abs(got["acc_objects"].sum(axis=0) - got["acc"])
        assert (err <= (k - 1) * 2.0 ** -24 * got["acc"] + 1e-14).all()
        sigma, _, share, active = SC.mix(raws)
        assert np.abs(share.sum(axis=0)[active.any(axis=0)] - 1.0).max() <= (k - 1) * 2.0 ** -24 + 1e-15


def test_overlap_mixes_by_density():
    """Two active objects: the colour is the density-weighted mean, between the two, and the density the sum."""
    raws = np.array([[[[0.5, -1.0, 2.0, 1.0]]], [[[-0.5, 1.0, 2.0, 3.0]]]], dtype=SC.F)
    sigma, colour, share, active = SC.mix(raws)
    s = SC.softplus20(np.array([0.0, 2.0])).astype(SC.F)
    assert active.all() and sigma[0, 0] == SC.F(s[0] + s[1])
    c = SC.widened_sigmoid(raws[:, 0, 0, :3])
    assert np.all(colour[0, 0] <= c.max(axis=0) + 1e-7) and np.all(colour[0, 0] >= c.min(axis=0) - 1e-7)
    assert np.allclose(colour[0, 0, 2], c[0, 2], atol=1e-7)         # equal colours mix to themselves
    assert np.allclose(share[:, 0, 0], s / (s[0] + s[1]), atol=1e-7)


# ---------------------------------------------------------------- SceneObject


def _grid():
    from codenerf.nerf import OccupancyGrid
    return OccupancyGrid.full(32, 1.0, "cpu")


def _codes():
    return torch.zeros(1, 256), torch.zeros(1, 256)


def test_scene_object_defaults_and_pose():
    from codenerf.nerf import SceneObject
    o = SceneObject(*_codes(), _grid())
    assert o.rotation == [[1, 0, 0], [0, 1, 0], [0, 0, 1]] and o.translation == [0, 0, 0]
    o = SceneObject(*_codes(), _grid(), rotation=torch.from_numpy(SC.rotation([1, 2, 3], 0.7)),
                    translation=np.array([0.5, 0.0, -2.0]))
    assert o.translation == [0.5, 0.0, -2.0] and o.coarse_model is None and o.fine_model is None
    z = torch.zeros(1, 256).expand(5, -1)
    assert SceneObject(z, z, _grid()).z_s.shape == (1, 256)


@pytest.mark.parametrize("case", ["scaled", "sheared", "reflected scale", "nan rotation", "inf translation",
                                  "nan translation", "no grid", "grid of the wrong type", "rotation shape",
                                  "translation shape", "code rows"])
def test_scene_object_validation(case):
    from codenerf.nerf import SceneObject
    zs, zt = _codes()
    eye = np.eye(3)
    kw = dict(occupancy=_grid())
    if case == "scaled":
        kw["rotation"] = eye * 1.001
    elif case == "sheared":
        kw["rotation"] = eye + np.array([[0, 1e-4, 0], [0, 0, 0], [0, 0, 0]])
    elif case == "reflected scale":
        kw["rotation"] = np.diag([1.0, 1.0, -2.0])
    elif case == "nan rotation":
        kw["rotation"] = np.array([[1, 0, 0], [0, float("nan"), 0], [0, 0, 1]])
    elif case == "inf translation":
        kw["translation"] = [0.0, float("inf"), 0.0]
    elif case == "nan translation":
        kw["translation"] = [float("nan"), 0.0, 0.0]
    elif case == "no grid":
        kw["occupancy"] = None
    elif case == "grid of the wrong type":
        kw["occupancy"] = torch.zeros(1024, dtype=torch.int32)
    elif case == "rotation shape":
        kw["rotation"] = np.eye(4)
    elif case == "translation shape":
        kw["translation"] = [0.0, 0.0]
    elif case == "code rows":
        zs = torch.zeros(4, 256)
    with pytest.raises(ValueError):
        SceneObject(zs, zt, **kw)


def test_scene_object_needs_its_grid_argument():
    from codenerf.nerf import SceneObject
    with pytest.raises(TypeError):
        SceneObject(*_codes())


def test_render_scene_refuses_bad_scenes():
    from codenerf.nerf import SceneObject, render_scene
    o = SceneObject(*_codes(), _grid())
    ro = torch.zeros(4, 3)
    for objects in ([], [o] * 9, [o, "car"]):
        with pytest.raises(ValueError):
            render_scene(ro, ro, objects, None, None, None)
