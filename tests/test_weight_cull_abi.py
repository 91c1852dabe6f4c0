"""The weight-culling entries' host side: the symbols are exported and every argument rule of
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
P_ODD8 = ctypes.c_void_p(0x10008)     # 8-B aligned, not 16-B
NAN, INF = float("nan"), float("inf")


def test_weight_cull_symbols_exported(lib):
    from codenerf import _lib
    for name in ("cn_weight_cull", "cn_scatter_rgb"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "codenerf.h")).read()
    assert "int cn_weight_cull(const float* weights," in header and "int cn_scatter_rgb(" in header
    # eps_weight travels as a float, eps_tail as a double
    args = _lib.SIGNATURES["cn_weight_cull"][1]
    assert args[8] is ctypes.c_float and args[9] is ctypes.c_double and len(args) == 17


def _cull(**kw):
    """A valid call (4 rays x 8 samples, one chunk, every output), then ``kw`` over it."""
    a = dict(weights=P, ro=P, rd=P, z=P, n_rays=4, n_samples=8, chunk_rows=4, code_index=None, eps_weight=1e-4,
             eps_tail=5e-4, workspace=P, count=P, sample_index=P, pts=P, vdir=P, code_out=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


CULL_EINVAL = {
    "null weights": dict(weights=None),
    "null ro": dict(ro=None),
    "null rd": dict(rd=None),
    "null z": dict(z=None),
    "null workspace": dict(workspace=None),
    "null count": dict(count=None),
    "null sample_index": dict(sample_index=None),
    "null pts": dict(pts=None),
    "null vdir": dict(vdir=None),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-4),
    "n_samples 0": dict(n_samples=0),
    "n_samples negative": dict(n_samples=-1),
    "n_samples 513": dict(n_samples=513),
    "rows past int32": dict(n_rays=1 << 23, n_samples=256),
    "chunk_rows 0": dict(chunk_rows=0),
    "chunk_rows negative": dict(chunk_rows=-4),
    "workspace misaligned": dict(workspace=P_ODD),
    "count misaligned": dict(count=P_ODD),
    "eps_weight negative": dict(eps_weight=-1e-6),
    "eps_weight NaN": dict(eps_weight=NAN),
    "eps_weight -inf": dict(eps_weight=-INF),
    "eps_tail negative": dict(eps_tail=-1e-300),
    "eps_tail NaN": dict(eps_tail=NAN),
    "eps_tail -inf": dict(eps_tail=-INF),
}


@pytest.mark.parametrize("case", sorted(CULL_EINVAL))
def test_weight_cull_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_weight_cull(*_cull(**CULL_EINVAL[case])) == _lib.CN_EINVAL, case
    # the optional pointers do not rescue a bad call
    assert lib.cn_weight_cull(*_cull(code_out=None, **CULL_EINVAL[case])) == _lib.CN_EINVAL, case
    assert lib.cn_weight_cull(*_cull(code_index=P, **CULL_EINVAL[case])) == _lib.CN_EINVAL, case


def _scatter(**kw):
    a = dict(raw_compact=P, sample_index=P, n_rows=8, raw=P, n_slots=32, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


SCATTER_EINVAL = {
    "null raw_compact": dict(raw_compact=None),
    "null sample_index": dict(sample_index=None),
    "null raw": dict(raw=None),
    "n_rows 0": dict(n_rows=0),
    "n_rows negative": dict(n_rows=-8),
    "n_rows above n_slots": dict(n_rows=33),
    "n_slots 0": dict(n_slots=0),
    "n_slots past int32": dict(n_slots=1 << 31),
    "both past int32": dict(n_rows=1 << 31, n_slots=1 << 31),
    "raw misaligned": dict(raw=P_ODD),
    "raw 8-B aligned only": dict(raw=P_ODD8),
    "raw_compact misaligned": dict(raw_compact=P_ODD),
    "raw_compact 8-B aligned only": dict(raw_compact=P_ODD8),
}


@pytest.mark.parametrize("case", sorted(SCATTER_EINVAL))
def test_scatter_rgb_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_scatter_rgb(*_scatter(**SCATTER_EINVAL[case])) == _lib.CN_EINVAL, case
