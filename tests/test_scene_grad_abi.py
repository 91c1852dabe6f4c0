"""The scene backward entries' host side: the symbols are exported and declared, and every argument rule of
include/codenerf.h is refused before any launch -- with dummy (never dereferenced) pointers and no device."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the HIP runtime must come from torch's copy, as in production)
    from codenerf import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "code-nerf_amd", "csrc"), "-j8"], check=True)
    return _lib.load(_lib.LIB_PATH)


# Dummy device pointers: aligned addresses nothing reads (every case below must return before a launch).
P = ctypes.c_void_p(0x10000)
P_ODD = ctypes.c_void_p(0x10004)      # 4-B aligned only
ADDR, ADDR_ODD = 0x10000, 0x10004
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]

ENTRIES = ("cn_volume_render_compose_backward", "cn_object_rays_backward", "cn_occupancy_gather",
           "cn_occupancy_cull_backward")


def test_scene_grad_symbols_exported_and_declared(lib):
    from codenerf import _lib, autograd, nerf, ops
    header = open(os.path.join(ROOT, "include", "codenerf.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert f"int {name}(" in header, name
    assert "int64_t cn_object_rays_backward_workspace_floats(" in header
    for name in ("volume_render_compose_backward", "object_rays_backward", "occupancy_gather", "occupancy_cull_backward"):
        assert callable(getattr(ops, name)), name
    for name in ("ObjectRays", "CullRows", "ExpandRows", "VolumeRenderCompose"):
        assert issubclass(getattr(autograd, name), __import__("torch").autograd.Function), name
    assert callable(nerf.render_scene_autograd) and callable(nerf.rigid_pose)


def _pointers(addresses):
    return ctypes.cast((ctypes.c_void_p * max(1, len(addresses)))(*addresses), ctypes.POINTER(ctypes.c_void_p))


def _compose_backward(**kw):
    """A valid call (3 objects, 4 rays x 8 samples, every gradient), then ``kw`` over it."""
    a = dict(raws=[ADDR] * 3, n_objects=None, z=P, rd=P, n_rays=4, n_samples=8, g_rgb=P, g_disp=P, g_acc=P,
             g_weights=P, g_depth=P, g_acc_objects=P, d_raws=[ADDR] * 3, d_rd=P, accumulate_rd=0, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    if a["n_objects"] is None:
        a["n_objects"] = len(a["raws"])
    for key in ("raws", "d_raws"):
        if a[key] is not None:
            a[key] = _pointers(a[key])
    return list(a.values())


COMPOSE_BACKWARD_EINVAL = {
    "null raws": dict(raws=None, n_objects=3),
    "null d_raws": dict(d_raws=None),
    "null first raw": dict(raws=[None, ADDR, ADDR]),
    "null last raw": dict(raws=[ADDR, ADDR, None]),
    "null first d_raw": dict(d_raws=[None, ADDR, ADDR]),
    "null last d_raw": dict(d_raws=[ADDR, ADDR, None]),
    "null z": dict(z=None),
    "null rd": dict(rd=None),
    "no objects": dict(raws=[ADDR] * 8, d_raws=[ADDR] * 8, n_objects=0),
    "objects negative": dict(raws=[ADDR] * 8, d_raws=[ADDR] * 8, n_objects=-1),
    "nine objects": dict(raws=[ADDR] * 9, d_raws=[ADDR] * 9),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-4),
    "n_samples 0": dict(n_samples=0),
    "n_samples negative": dict(n_samples=-8),
    "n_samples 513": dict(n_samples=513),
    "first raw misaligned": dict(raws=[ADDR_ODD, ADDR, ADDR]),
    "last raw misaligned": dict(raws=[ADDR, ADDR, ADDR_ODD]),
    "first d_raw misaligned": dict(d_raws=[ADDR_ODD, ADDR, ADDR]),
    "last d_raw misaligned": dict(d_raws=[ADDR, ADDR, ADDR_ODD]),
    "z misaligned": dict(z=P_ODD),
    "accumulate_rd 2": dict(accumulate_rd=2),
    "accumulate_rd negative": dict(accumulate_rd=-1),
}


@pytest.mark.parametrize("case", sorted(COMPOSE_BACKWARD_EINVAL))
def test_compose_backward_argument_errors(lib, case):
    from codenerf import _lib
    kw = COMPOSE_BACKWARD_EINVAL[case]
    assert lib.cn_volume_render_compose_backward(*_compose_backward(**kw)) == _lib.CN_EINVAL, case
    # the optional gradients and d_rd do not rescue a bad call
    none = dict(g_rgb=None, g_disp=None, g_acc=None, g_weights=None, g_depth=None, g_acc_objects=None, d_rd=None)
    assert lib.cn_volume_render_compose_backward(*_compose_backward(**none, **kw)) == _lib.CN_EINVAL, case


def _object_rays_backward(**kw):
    """A valid call (2 identity poses, 4 rays, every output), then ``kw`` over it."""
    a = dict(g_ro_obj=P, g_rd_obj=P, ro=P, rd=P, n_rays=4, poses=IDENTITY * 2, n_objects=None, d_ro=P, d_rd=P,
             accumulate=0, d_poses=P, workspace=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    if a["n_objects"] is None:
        a["n_objects"] = len(a["poses"]) // 12
    if a["poses"] is not None:
        a["poses"] = (ctypes.c_float * max(1, len(a["poses"])))(*a["poses"])
    return list(a.values())


def _with(index, value, n=2):
    p = IDENTITY * n
    p[index] = value
    return p


OBJECT_RAYS_BACKWARD_EINVAL = {
    "null ro": dict(ro=None),
    "null rd": dict(rd=None),
    "null poses": dict(poses=None, n_objects=2),
    "no output": dict(d_ro=None, d_rd=None, d_poses=None),
    "d_poses without a workspace": dict(workspace=None),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-1),
    "no objects": dict(poses=IDENTITY * 8, n_objects=0),
    "objects negative": dict(poses=IDENTITY * 8, n_objects=-2),
    "nine objects": dict(poses=IDENTITY * 9),
    "nan rotation entry": dict(poses=_with(4, float("nan"))),
    "inf translation entry": dict(poses=_with(12 + 9, float("inf"))),
    "nan in the last of eight": dict(poses=_with(12 * 7 + 11, float("nan"), n=8)),
    "accumulate 2": dict(accumulate=2),
    "accumulate negative": dict(accumulate=-1),
}


@pytest.mark.parametrize("case", sorted(OBJECT_RAYS_BACKWARD_EINVAL))
def test_object_rays_backward_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_object_rays_backward(*_object_rays_backward(**OBJECT_RAYS_BACKWARD_EINVAL[case])) == _lib.CN_EINVAL, case


def test_object_rays_backward_workspace_floats(lib):
    f = lib.cn_object_rays_backward_workspace_floats
    assert f(0, 1) == -1 and f(-5, 1) == -1 and f(4, 0) == -1 and f(4, 9) == -1
    assert f(1, 1) == 12 and f(256, 3) == 36 and f(257, 3) == 72
    big = f(1 << 30, 8)
    assert 0 < big <= 256 * 8 * 12                  # the block partials are bounded
    assert f(1000, 8) == 8 * f(1000, 1)


def _gather(**kw):
    a = dict(g_raw=P, workspace=P, n_rays=4, n_samples=8, g_compact=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


GATHER_EINVAL = {
    "null g_raw": dict(g_raw=None),
    "null workspace": dict(workspace=None),
    "null g_compact": dict(g_compact=None),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-4),
    "n_samples 0": dict(n_samples=0),
    "n_samples 513": dict(n_samples=513),
    "rows past int32": dict(n_rays=1 << 23, n_samples=256),
    "g_raw misaligned": dict(g_raw=P_ODD),
    "g_compact misaligned": dict(g_compact=P_ODD),
    "workspace misaligned": dict(workspace=P_ODD),
}


@pytest.mark.parametrize("case", sorted(GATHER_EINVAL))
def test_gather_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_occupancy_gather(*_gather(**GATHER_EINVAL[case])) == _lib.CN_EINVAL, case


def _cull_backward(**kw):
    a = dict(g_pts=P, g_vdir=P, z=P, workspace=P, n_rays=4, n_samples=8, chunk_rows=4, d_ro=P, d_rd=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


CULL_BACKWARD_EINVAL = {
    "null z": dict(z=None),
    "null workspace": dict(workspace=None),
    "no output": dict(d_ro=None, d_rd=None),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-4),
    "n_samples 0": dict(n_samples=0),
    "n_samples 513": dict(n_samples=513),
    "rows past int32": dict(n_rays=1 << 23, n_samples=256),
    "chunk_rows 0": dict(chunk_rows=0),
    "chunk_rows negative": dict(chunk_rows=-4),
    "workspace misaligned": dict(workspace=P_ODD),
}


@pytest.mark.parametrize("case", sorted(CULL_BACKWARD_EINVAL))
def test_cull_backward_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_occupancy_cull_backward(*_cull_backward(**CULL_BACKWARD_EINVAL[case])) == _lib.CN_EINVAL, case
    if "output" not in case:        # the optional gradients do not rescue a bad call
        assert lib.cn_occupancy_cull_backward(*_cull_backward(g_pts=None, g_vdir=None, **CULL_BACKWARD_EINVAL[case])) \
            == _lib.CN_EINVAL, case


def test_wrappers_refuse_host_tensors(lib):
    """The wrappers go through the package's device check: CPU tensors raise, nothing falls back."""
    import torch
    from codenerf import ops
    raw, z, rd = torch.zeros(4, 8, 4), torch.zeros(4, 8), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.volume_render_compose_backward([raw, raw], z, rd)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.object_rays_backward(torch.zeros(1, 4, 3), None, rd, rd, [IDENTITY])
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.occupancy_gather(raw, (None, 4, 8, 0))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.occupancy_cull_backward(None, None, z, 4, (None, 4, 8, 0))


def test_render_scene_autograd_refusals_need_no_device():
    """More than 8 objects and a non-(K, 12) pose tensor are refused before anything touches a device."""
    import torch
    from codenerf.nerf import OccupancyGrid, SceneObject, render_scene_autograd, rigid_pose
    grid = OccupancyGrid(torch.zeros(32 ** 3 // 32, dtype=torch.int32), 32, 1.0)
    obj = SceneObject(torch.zeros(1, 256), torch.zeros(1, 256), grid)
    rays = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="1..8"):
        render_scene_autograd(rays, rays, [obj] * 9, None, None, None, None)
    with pytest.raises(ValueError, match="1..8"):
        render_scene_autograd(rays, rays, [], None, None, None, None)
    with pytest.raises(ValueError):
        rigid_pose(torch.zeros(4), torch.zeros(3))
