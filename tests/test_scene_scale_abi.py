"""The scaled scene entries' host side: the symbols are exported and declared, every argument rule of
include/codenerf.h -- what the unscaled entries refuse, and a scale that is NaN, infinite, 0 or negative -- is
refused before any launch (dummy, never dereferenced pointers and no device), and the Python layer's own
refusals."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from test_scene_grad_abi import ADDR, ADDR_ODD, COMPOSE_BACKWARD_EINVAL, IDENTITY, OBJECT_RAYS_BACKWARD_EINVAL, P, P_ODD
from test_scene_grad_abi import _pointers


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the HIP runtime must come from torch's copy, as in production)
    from codenerf import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "code-nerf_amd", "csrc"), "-j8"], check=True)
    return _lib.load(_lib.LIB_PATH)


ENTRIES = ("cn_object_rays_scaled", "cn_volume_render_compose_scaled", "cn_volume_render_compose_scaled_backward",
           "cn_object_rays_scaled_backward")
SIZES = ("cn_volume_render_compose_scaled_backward_workspace_floats", "cn_object_rays_scaled_backward_workspace_floats")
BAD_SCALES = {"nan": float("nan"), "inf": float("inf"), "zero": 0.0, "minus zero": -0.0, "negative": -2.0,
              "minus inf": float("-inf")}
SIMILARITY = IDENTITY + [1.0]


def test_scene_scale_symbols_exported_and_declared(lib):
    import torch
    from codenerf import _lib, autograd, nerf, ops
    header = open(os.path.join(ROOT, "include", "codenerf.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert f"int {name}(" in header, name
    for name in SIZES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert f"int64_t {name}(" in header, name
    assert callable(nerf.similarity_pose) and "similarity_pose" in nerf.__all__
    for name in ("ObjectRays", "VolumeRenderCompose"):
        assert issubclass(getattr(autograd, name), torch.autograd.Function), name
    import inspect
    assert "scales" in inspect.signature(ops.volume_render_compose).parameters
    assert {"scales", "want_scales"} <= set(inspect.signature(ops.volume_render_compose_backward).parameters)
    assert "scale" in inspect.signature(nerf.SceneObject.__init__).parameters


def _floats(values):
    return None if values is None else (ctypes.c_float * max(1, len(values)))(*values)


# ---------------------------------------------------------------- cn_object_rays_scaled


def _object_rays(**kw):
    """A valid call (2 similarity poses, 4 rays), then ``kw`` over it."""
    a = dict(ro=P, rd=P, n_rays=4, poses=SIMILARITY * 2, n_objects=None, ro_out=P, rd_out=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    if a["n_objects"] is None:
        a["n_objects"] = len(a["poses"]) // 13
    a["poses"] = _floats(a["poses"])
    return list(a.values())


def _with13(index, value, n=2):
    p = SIMILARITY * n
    p[index] = value
    return p


OBJECT_RAYS_EINVAL = {
    "null ro": dict(ro=None),
    "null rd": dict(rd=None),
    "null poses": dict(poses=None, n_objects=2),
    "null ro_out": dict(ro_out=None),
    "null rd_out": dict(rd_out=None),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-1),
    "no objects": dict(poses=SIMILARITY * 8, n_objects=0),
    "objects negative": dict(poses=SIMILARITY * 8, n_objects=-2),
    "nine objects": dict(poses=SIMILARITY * 9),
    "nan rotation entry": dict(poses=_with13(4, float("nan"))),
    "inf translation entry": dict(poses=_with13(13 + 9, float("inf"))),
    "nan in the last of eight": dict(poses=_with13(13 * 7 + 11, float("nan"), n=8)),
}
for _name, _v in BAD_SCALES.items():
    OBJECT_RAYS_EINVAL[f"first scale {_name}"] = dict(poses=_with13(12, _v))
    OBJECT_RAYS_EINVAL[f"last of eight scales {_name}"] = dict(poses=_with13(13 * 7 + 12, _v, n=8))


@pytest.mark.parametrize("case", sorted(OBJECT_RAYS_EINVAL))
def test_object_rays_scaled_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_object_rays_scaled(*_object_rays(**OBJECT_RAYS_EINVAL[case])) == _lib.CN_EINVAL, case


# ---------------------------------------------------------------- cn_volume_render_compose_scaled


def _compose(**kw):
    """A valid call (3 objects, 4 rays x 8 samples, every output), then ``kw`` over it."""
    a = dict(raws=[ADDR] * 3, scales=[1.0, 2.0, 0.5], n_objects=None, z=P, rd=P, n_rays=4, n_samples=8, rgb=P, disp=P,
             acc=P, weights=P, depth=P, acc_objects=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    if a["n_objects"] is None:
        a["n_objects"] = len(a["raws"])
    if a["raws"] is not None:
        a["raws"] = _pointers(a["raws"])
    a["scales"] = _floats(a["scales"])
    return list(a.values())


COMPOSE_EINVAL = {
    "null raws": dict(raws=None, n_objects=3),
    "null scales": dict(scales=None),
    "null first raw": dict(raws=[None, ADDR, ADDR]),
    "null last raw": dict(raws=[ADDR, ADDR, None]),
    "null z": dict(z=None),
    "null rd": dict(rd=None),
    "null rgb": dict(rgb=None),
    "null disp": dict(disp=None),
    "null acc": dict(acc=None),
    "null depth": dict(depth=None),
    "no objects": dict(raws=[ADDR] * 8, scales=[1.0] * 8, n_objects=0),
    "objects negative": dict(raws=[ADDR] * 8, scales=[1.0] * 8, n_objects=-1),
    "nine objects": dict(raws=[ADDR] * 9, scales=[1.0] * 9),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-4),
    "n_samples 0": dict(n_samples=0),
    "n_samples 513": dict(n_samples=513),
    "first raw misaligned": dict(raws=[ADDR_ODD, ADDR, ADDR]),
    "last raw misaligned": dict(raws=[ADDR, ADDR, ADDR_ODD]),
    "z misaligned": dict(z=P_ODD),
    "weights misaligned": dict(weights=P_ODD),
}
for _name, _v in BAD_SCALES.items():
    COMPOSE_EINVAL[f"first scale {_name}"] = dict(scales=[_v, 1.0, 1.0])
    COMPOSE_EINVAL[f"last scale {_name}"] = dict(scales=[1.0, 1.0, _v])


@pytest.mark.parametrize("case", sorted(COMPOSE_EINVAL))
def test_compose_scaled_argument_errors(lib, case):
    from codenerf import _lib
    kw = COMPOSE_EINVAL[case]
    assert lib.cn_volume_render_compose_scaled(*_compose(**kw)) == _lib.CN_EINVAL, case
    if "weights" not in case:       # the optional outputs do not rescue a bad call
        assert lib.cn_volume_render_compose_scaled(*_compose(weights=None, acc_objects=None, **kw)) == _lib.CN_EINVAL, case


# ---------------------------------------------------------------- cn_volume_render_compose_scaled_backward


def _compose_backward(**kw):
    """A valid call (3 objects, 4 rays x 8 samples, every gradient and d_scales), then ``kw`` over it."""
    a = dict(raws=[ADDR] * 3, scales=[1.0, 2.0, 0.5], n_objects=None, z=P, rd=P, n_rays=4, n_samples=8, g_rgb=P,
             g_disp=P, g_acc=P, g_weights=P, g_depth=P, g_acc_objects=P, d_raws=[ADDR] * 3, d_rd=P, accumulate_rd=0,
             d_scales=P, workspace=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    if a["n_objects"] is None:
        a["n_objects"] = len(a["raws"])
    for key in ("raws", "d_raws"):
        if a[key] is not None:
            a[key] = _pointers(a[key])
    a["scales"] = _floats(a["scales"])
    return list(a.values())


SCALED_BACKWARD_EINVAL = dict(COMPOSE_BACKWARD_EINVAL)             # everything the unscaled entry refuses
for _case in ("no objects", "objects negative"):
    SCALED_BACKWARD_EINVAL[_case] = dict(COMPOSE_BACKWARD_EINVAL[_case], scales=[1.0] * 8)
SCALED_BACKWARD_EINVAL["nine objects"] = dict(COMPOSE_BACKWARD_EINVAL["nine objects"], scales=[1.0] * 9)
SCALED_BACKWARD_EINVAL["null scales"] = dict(scales=None)
SCALED_BACKWARD_EINVAL["d_scales without a workspace"] = dict(workspace=None)
for _name, _v in BAD_SCALES.items():
    SCALED_BACKWARD_EINVAL[f"first scale {_name}"] = dict(scales=[_v, 1.0, 1.0])
    SCALED_BACKWARD_EINVAL[f"last scale {_name}"] = dict(scales=[1.0, 1.0, _v])


@pytest.mark.parametrize("case", sorted(SCALED_BACKWARD_EINVAL))
def test_compose_scaled_backward_argument_errors(lib, case):
    from codenerf import _lib
    kw = SCALED_BACKWARD_EINVAL[case]
    assert lib.cn_volume_render_compose_scaled_backward(*_compose_backward(**kw)) == _lib.CN_EINVAL, case
    if "workspace" in case:
        return
    # the optional gradients and outputs do not rescue a bad call
    none = dict(g_rgb=None, g_disp=None, g_acc=None, g_weights=None, g_depth=None, g_acc_objects=None, d_rd=None,
                d_scales=None, workspace=None)
    assert lib.cn_volume_render_compose_scaled_backward(*_compose_backward(**none, **kw)) == _lib.CN_EINVAL, case


def test_compose_scaled_backward_workspace_floats(lib):
    f = lib.cn_volume_render_compose_scaled_backward_workspace_floats
    assert f(0, 8, 1) == -1 and f(-5, 8, 1) == -1 and f(4, 0, 1) == -1 and f(4, 513, 1) == -1
    assert f(4, 8, 0) == -1 and f(4, 8, 9) == -1
    # one partial per wave that holds a ray: 4 rays per wave up to 128 samples, one above
    assert f(1, 8, 1) == 1 and f(4, 128, 1) == 1 and f(5, 128, 3) == 6 and f(5, 129, 3) == 15 and f(67, 512, 8) == 536
    assert f(1000, 64, 8) == 8 * f(1000, 64, 1)


# ---------------------------------------------------------------- cn_object_rays_scaled_backward


def _object_rays_backward(**kw):
    """A valid call (2 similarity poses, 4 rays, every output), then ``kw`` over it."""
    a = dict(g_ro_obj=P, g_rd_obj=P, ro=P, rd=P, n_rays=4, poses=SIMILARITY * 2, n_objects=None, d_ro=P, d_rd=P,
             accumulate=0, d_poses=P, workspace=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    if a["n_objects"] is None:
        a["n_objects"] = len(a["poses"]) // 13
    a["poses"] = _floats(a["poses"])
    return list(a.values())


def _rows13(poses12):
    """Rows of 12 (test_scene_grad_abi's cases) as rows of 13 with scale 1, NaN / inf entries kept in place."""
    return [v for k in range(len(poses12) // 12) for v in poses12[12 * k:12 * k + 12] + [1.0]]


SCALED_RAYS_BACKWARD_EINVAL = {}
for _case, _kw in OBJECT_RAYS_BACKWARD_EINVAL.items():             # everything the unscaled entry refuses
    _kw = dict(_kw)
    if _kw.get("poses") is not None:
        _kw["poses"] = _rows13(_kw["poses"])
    SCALED_RAYS_BACKWARD_EINVAL[_case] = _kw
for _name, _v in BAD_SCALES.items():
    SCALED_RAYS_BACKWARD_EINVAL[f"first scale {_name}"] = dict(poses=_with13(12, _v))
    SCALED_RAYS_BACKWARD_EINVAL[f"last of eight scales {_name}"] = dict(poses=_with13(13 * 7 + 12, _v, n=8))


@pytest.mark.parametrize("case", sorted(SCALED_RAYS_BACKWARD_EINVAL))
def test_object_rays_scaled_backward_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_object_rays_scaled_backward(*_object_rays_backward(**SCALED_RAYS_BACKWARD_EINVAL[case])) \
        == _lib.CN_EINVAL, case


def test_object_rays_scaled_backward_workspace_floats(lib):
    f, rigid = lib.cn_object_rays_scaled_backward_workspace_floats, lib.cn_object_rays_backward_workspace_floats
    assert f(0, 1) == -1 and f(-5, 1) == -1 and f(4, 0) == -1 and f(4, 9) == -1
    assert f(1, 1) == 13 and f(256, 3) == 39 and f(257, 3) == 78
    for n, k in ((1, 1), (1000, 8), (1 << 30, 8)):
        assert f(n, k) * 12 == rigid(n, k) * 13             # the same blocks, 13 sums each


# ---------------------------------------------------------------- the Python layer


def _grid():
    import torch
    from codenerf.nerf import OccupancyGrid
    return OccupancyGrid(torch.zeros(32 ** 3 // 32, dtype=torch.int32), 32, 1.0)


def test_scene_object_scale():
    import torch
    from codenerf.nerf import SceneObject
    codes = (torch.zeros(1, 256), torch.zeros(1, 256))
    assert SceneObject(*codes, _grid()).scale == 1.0
    obj = SceneObject(*codes, _grid(), scale=torch.tensor(2.5))
    assert obj.scale == 2.5 and isinstance(obj.scale, float)
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf"), "big", None, [1.0, 2.0]):
        with pytest.raises(ValueError, match="scale"):
            SceneObject(*codes, _grid(), scale=bad)
    # the rotation stays orthonormal: a scale folded into it is still refused
    with pytest.raises(ValueError, match="orthonormal"):
        SceneObject(*codes, _grid(), rotation=[[2.0, 0, 0], [0, 2.0, 0], [0, 0, 2.0]], scale=2.0)


def test_wrappers_refuse_bad_scales_and_host_tensors(lib):
    import torch
    from codenerf import ops
    raw, z, rd = torch.zeros(4, 8, 4), torch.zeros(4, 8), torch.zeros(4, 3)
    for bad in ([1.0], [1.0, 0.0], [1.0, float("nan")], [float("inf"), 1.0], [1.0, -1.0]):
        with pytest.raises(AssertionError, match="scale"):
            ops.volume_render_compose([raw, raw], z, rd, scales=bad)
        with pytest.raises(AssertionError, match="scale"):
            ops.volume_render_compose_backward([raw, raw], z, rd, scales=bad)
    with pytest.raises(AssertionError, match="want_scales"):
        ops.volume_render_compose_backward([raw, raw], z, rd, want_scales=True)
    eye = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    with pytest.raises(AssertionError, match="scale"):
        ops._pose_rows([(eye, [0, 0, 0], 0.0)])
    with pytest.raises(AssertionError, match="pose"):
        ops._pose_rows([[0.0] * 14])
    # widths: pairs and rows of 12 stay 12; any triple or row of 13 makes every pose 13 floats
    assert ops._pose_rows([(eye, [0, 0, 0]), IDENTITY])[1] == 12
    flat, width = ops._pose_rows([(eye, [1, 2, 3]), (eye, [0, 0, 0], 2.0), IDENTITY + [0.5]])
    assert width == 13 and flat[12::13] == [1.0, 2.0, 0.5] and flat[9:12] == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.volume_render_compose([raw, raw], z, rd, scales=[1.0, 2.0])
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.volume_render_compose_backward([raw, raw], z, rd, scales=[1.0, 2.0], want_scales=True)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.object_rays(rd, rd, [IDENTITY + [2.0]])
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.object_rays_backward(torch.zeros(1, 4, 3), None, rd, rd, [IDENTITY + [2.0]])


def test_render_scene_autograd_refuses_malformed_poses():
    """A pose tensor that is not (K, 12) or (K, 13) float32, and a (K, 13) one with a scale that is not finite and
    > 0, are refused before anything touches a device."""
    import torch
    from codenerf.models import CodeNeRFModel
    from codenerf.nerf import SceneObject, render_scene_autograd, similarity_pose
    model = CodeNeRFModel(hidden_size=256, shape_code_size=256, texture_code_size=256, num_encoding_fn_xyz=10,
                          num_encoding_fn_dir=4).requires_grad_(False)
    obj = SceneObject(torch.zeros(1, 256), torch.zeros(1, 256), _grid())
    rays = torch.zeros(4, 3)
    row = similarity_pose(torch.zeros(3), torch.zeros(3), torch.zeros(()))
    for bad in (torch.zeros(2, 14), torch.zeros(2, 11), torch.zeros(3, 13), torch.zeros(26), torch.zeros(2, 13, 1),
                torch.zeros(2, 13, dtype=torch.float64), [[0.0] * 13] * 2):
        with pytest.raises(ValueError, match="poses"):
            render_scene_autograd(rays, rays, [obj, obj], None, None, model, model, poses=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        poses = torch.stack([row, row]).clone()
        poses[1, 12] = bad
        with pytest.raises(ValueError, match="scale"):
            render_scene_autograd(rays, rays, [obj, obj], None, None, model, model, poses=poses)
    with pytest.raises(ValueError):
        similarity_pose(torch.zeros(3), torch.zeros(3), torch.zeros(2))
