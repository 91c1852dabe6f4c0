"""The scene entries' host side: both symbols are exported and declared, and every argument rule of
include/codenerf.h is refused before any launch -- with dummy (never dereferenced) pointers and no
device."""
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

ENTRIES = ("cn_volume_render_compose", "cn_object_rays")


def test_scene_symbols_exported_and_declared(lib):
    from codenerf import _lib, ops
    header = open(os.path.join(ROOT, "include", "codenerf.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert f"int {name}(" in header, name
    assert "#define CN_MAX_SCENE_OBJECTS 8" in header and _lib.CN_MAX_SCENE_OBJECTS == 8
    assert callable(ops.volume_render_compose) and callable(ops.object_rays)


def _raws(addresses):
    return (ctypes.c_void_p * max(1, len(addresses)))(*addresses)


def _compose(**kw):
    """A valid call (3 objects, 4 rays x 8 samples, every output), then ``kw`` over it."""
    a = dict(raws=[ADDR] * 3, n_objects=None, z=P, rd=P, n_rays=4, n_samples=8, rgb=P, disp=P, acc=P, weights=P,
             depth=P, acc_objects=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    if a["n_objects"] is None:
        a["n_objects"] = len(a["raws"])
    if a["raws"] is not None:
        a["raws"] = ctypes.cast(_raws(a["raws"]), ctypes.POINTER(ctypes.c_void_p))
    return list(a.values())


COMPOSE_EINVAL = {
    "null raws": dict(raws=None, n_objects=3),
    "null first entry": dict(raws=[None, ADDR, ADDR]),
    "null last entry": dict(raws=[ADDR, ADDR, None]),
    "null only entry": dict(raws=[None]),
    "null z": dict(z=None),
    "null rd": dict(rd=None),
    "null rgb": dict(rgb=None),
    "null disp": dict(disp=None),
    "null acc": dict(acc=None),
    "null depth": dict(depth=None),
    "no objects": dict(raws=[ADDR] * 8, n_objects=0),
    "objects negative": dict(raws=[ADDR] * 8, n_objects=-1),
    "nine objects": dict(raws=[ADDR] * 9),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-4),
    "n_samples 0": dict(n_samples=0),
    "n_samples negative": dict(n_samples=-8),
    "n_samples 513": dict(n_samples=513),
    "first raw misaligned": dict(raws=[ADDR_ODD, ADDR, ADDR]),
    "last raw misaligned": dict(raws=[ADDR, ADDR, ADDR_ODD]),
    "z misaligned": dict(z=P_ODD),
    "weights misaligned": dict(weights=P_ODD),
}


@pytest.mark.parametrize("case", sorted(COMPOSE_EINVAL))
def test_compose_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_volume_render_compose(*_compose(**COMPOSE_EINVAL[case])) == _lib.CN_EINVAL, case
    if "weights" not in case:       # the optional outputs do not rescue a bad call
        assert lib.cn_volume_render_compose(*_compose(weights=None, acc_objects=None, **COMPOSE_EINVAL[case])) \
            == _lib.CN_EINVAL, case


def test_compose_refuses_what_volume_render_refuses(lib):
    """The sizes and alignments cn_volume_render refuses, with one object."""
    from codenerf import _lib
    for kw in (dict(n_rays=0), dict(n_samples=0), dict(n_samples=513), dict(z=P_ODD), dict(weights=P_ODD)):
        v = dict(raw=P, z=P, rd=P, n_rays=4, n_samples=8, rgb=P, disp=P, acc=P, weights=P, depth=P, stream=None)
        v.update(kw)
        assert lib.cn_volume_render(*v.values()) == _lib.CN_EINVAL, kw
        assert lib.cn_volume_render_compose(*_compose(raws=[ADDR], **kw)) == _lib.CN_EINVAL, kw
    assert lib.cn_volume_render_compose(*_compose(raws=[ADDR_ODD])) == _lib.CN_EINVAL


IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


def _object_rays(**kw):
    """A valid call (2 identity poses, 4 rays), then ``kw`` over it."""
    a = dict(ro=P, rd=P, n_rays=4, poses=IDENTITY * 2, n_objects=None, ro_out=P, rd_out=P, stream=None)
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


OBJECT_RAYS_EINVAL = {
    "null ro": dict(ro=None),
    "null rd": dict(rd=None),
    "null poses": dict(poses=None, n_objects=2),
    "null ro_out": dict(ro_out=None),
    "null rd_out": dict(rd_out=None),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-1),
    "no objects": dict(poses=IDENTITY * 8, n_objects=0),
    "objects negative": dict(poses=IDENTITY * 8, n_objects=-2),
    "nine objects": dict(poses=IDENTITY * 9),
    "nan rotation entry": dict(poses=_with(4, float("nan"))),
    "inf rotation entry": dict(poses=_with(12 + 8, float("inf"))),
    "nan translation entry": dict(poses=_with(12 + 9, float("nan"))),
    "-inf translation entry": dict(poses=_with(11, float("-inf"))),
    "nan in the last of eight": dict(poses=_with(12 * 7 + 11, float("nan"), n=8)),
}


@pytest.mark.parametrize("case", sorted(OBJECT_RAYS_EINVAL))
def test_object_rays_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_object_rays(*_object_rays(**OBJECT_RAYS_EINVAL[case])) == _lib.CN_EINVAL, case


def test_wrappers_refuse_host_tensors(lib):
    """Both wrappers go through the package's device check: CPU tensors raise, nothing falls back."""
    import torch
    from codenerf import ops
    raw, z, rd = torch.zeros(4, 8, 4), torch.zeros(4, 8), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.volume_render_compose([raw, raw], z, rd)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.object_rays(rd, rd, [([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [0, 0, 0])])
