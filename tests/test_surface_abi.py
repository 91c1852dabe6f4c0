"""The surface entries' host side: the symbols are exported, declared and typed, and every argument rule of
include/codenerf.h is refused before any launch -- with dummy (never dereferenced) device pointers and no device."""
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


P = 0x10000                           # a dummy device address nothing reads, 16-byte aligned
INF, NAN = float("inf"), float("nan")
N_ARGS = {"cn_surface_bracket": 9, "cn_surface_step": 12, "cn_surface_shade": 9}


def test_surface_symbols_exported(lib):
    from codenerf import _lib, nerf, ops
    header = open(os.path.join(ROOT, "include", "codenerf.h")).read()
    for name, n in N_ARGS.items():
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
        assert f"int {name}(" in header, name
        assert callable(getattr(ops, name[3:])), name
    assert "Iso-surface ray casting" in header
    assert callable(nerf.render_surface) and "render_surface" in nerf.__all__


def _bracket(**kw):
    dev = ctypes.c_void_p(P)
    a = dict(sigma=dev, sigma_stride=1, z=dev, n_rays=5, n_samples=64, level=0.5, bracket=dev, hit=dev, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


def _step(**kw):
    dev = ctypes.c_void_p(P)
    a = dict(ro=dev, rd=dev, hit=dev, probe_sigma=dev, probe_stride=1, level=0.5, finish=0, n_rays=5, bracket=dev,
             t=dev, pts=dev, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


def _shade(host_null=False, **kw):
    dev = ctypes.c_void_p(P)
    bg = None if host_null else (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    a = dict(raw=dev, hit=dev, t=dev, background=bg, n_rays=5, rgb=dev, depth=dev, pts=dev, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


BRACKET_EINVAL = {
    "null sigma": dict(sigma=None),
    "null z": dict(z=None),
    "null bracket": dict(bracket=None),
    "null hit": dict(hit=None),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-3),
    "n_samples 1": dict(n_samples=1),
    "n_samples 0": dict(n_samples=0),
    "n_samples negative": dict(n_samples=-64),
    "n_samples 1025": dict(n_samples=1025),
    "level NaN": dict(level=NAN),
    "level inf": dict(level=INF),
    "level -inf": dict(level=-INF),
    "stride 0": dict(sigma_stride=0),
    "stride 2": dict(sigma_stride=2),
    "stride 3": dict(sigma_stride=3),
    "stride 8": dict(sigma_stride=8),
    "stride negative": dict(sigma_stride=-1),
}

STEP_EINVAL = {
    "null ro": dict(ro=None),
    "null rd": dict(rd=None),
    "null hit": dict(hit=None),
    "null bracket": dict(bracket=None),
    "null t": dict(t=None),
    "null pts": dict(pts=None),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-1),
    "finish 2": dict(finish=2),
    "finish -1": dict(finish=-1),
    "stride 0": dict(probe_stride=0),
    "stride 2": dict(probe_stride=2),
    "stride 5": dict(probe_stride=5),
    "level NaN": dict(level=NAN),
    "level inf": dict(level=INF),
    "bracket misaligned": dict(bracket=ctypes.c_void_p(P + 4)),
}

SHADE_EINVAL = {
    "null raw": dict(raw=None),
    "null hit": dict(hit=None),
    "null t": dict(t=None),
    "null background": dict(host_null=True),
    "null rgb": dict(rgb=None),
    "null depth": dict(depth=None),
    "null pts": dict(pts=None),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-7),
    "raw misaligned": dict(raw=ctypes.c_void_p(P + 8)),
}


@pytest.mark.parametrize("case", sorted(BRACKET_EINVAL))
def test_surface_bracket_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_surface_bracket(*_bracket(**BRACKET_EINVAL[case])) == _lib.CN_EINVAL, case
    if "stride" not in case:          # the other valid stride does not rescue a bad call
        assert lib.cn_surface_bracket(*_bracket(sigma_stride=4, **BRACKET_EINVAL[case])) == _lib.CN_EINVAL, case


@pytest.mark.parametrize("case", sorted(STEP_EINVAL))
def test_surface_step_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_surface_step(*_step(**STEP_EINVAL[case])) == _lib.CN_EINVAL, case
    # neither does the first call's form (no probe), nor a finishing call
    assert lib.cn_surface_step(*_step(**{"probe_sigma": None, **STEP_EINVAL[case]})) == _lib.CN_EINVAL, case
    if "finish" not in case:
        assert lib.cn_surface_step(*_step(**{"finish": 1, **STEP_EINVAL[case]})) == _lib.CN_EINVAL, case


@pytest.mark.parametrize("case", sorted(SHADE_EINVAL))
def test_surface_shade_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_surface_shade(*_shade(**SHADE_EINVAL[case])) == _lib.CN_EINVAL, case


def test_ops_refuse_cpu_tensors():
    import torch
    from codenerf import ops
    z = torch.zeros(3, 4)
    with pytest.raises(ValueError):
        ops.surface_bracket(z, z, 0.5)
    with pytest.raises(ValueError):
        ops.surface_step(torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3, dtype=torch.int32), z, 0.5)
    with pytest.raises(ValueError):
        ops.surface_shade(z, torch.zeros(3, dtype=torch.int32), torch.zeros(3), torch.zeros(3, 3))


def test_render_surface_refusals_need_no_device():
    """What render_surface refuses before it touches a tensor: refine, level."""
    import torch
    from codenerf.nerf import render_surface
    x = torch.zeros(2, 3)
    c = torch.zeros(1, 256)
    for refine in (-1, 25, 2.0, True, None):
        with pytest.raises(ValueError, match="refine"):
            render_surface(x, x, c, c, None, None, None, 1.0, refine=refine)
    for level, activated in ((0.0, True), (-1.0, True), (NAN, True), (INF, False), (NAN, False), (None, False)):
        with pytest.raises(ValueError, match="level"):
            render_surface(x, x, c, c, None, None, None, level, activated=activated)
