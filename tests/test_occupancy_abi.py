"""The occupancy entries' host side: the symbols are exported and every argument rule of
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

ENTRIES = ("cn_occupancy_build", "cn_occupancy_cull_workspace_bytes", "cn_occupancy_cull", "cn_occupancy_expand")


def test_occupancy_symbols_exported(lib):
    from codenerf import _lib
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.CN_EMPTY_SIGMA_RAW == -1.0e4
    header = open(os.path.join(ROOT, "include", "codenerf.h")).read()
    assert "#define CN_EMPTY_SIGMA_RAW (-1.0e4f)" in header


def _build(**kw):
    a = dict(nodes=P, g=32, threshold=0.5, dilate=1, bits=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


BUILD_EINVAL = {
    "null nodes": dict(nodes=None),
    "null bits": dict(bits=None),
    "g 0": dict(g=0),
    "g negative": dict(g=-32),
    "g 16": dict(g=16),
    "g not a multiple of 32": dict(g=48),
    "g 33": dict(g=33),
    "g above 512": dict(g=544),
    "g 1024": dict(g=1024),
    "dilate 3": dict(dilate=3),
    "dilate negative": dict(dilate=-1),
}


@pytest.mark.parametrize("case", sorted(BUILD_EINVAL))
def test_build_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_occupancy_build(*_build(**BUILD_EINVAL[case])) == _lib.CN_EINVAL, case


def _cull(**kw):
    """A valid call (4 rays x 8 samples, one chunk, a 32^3 grid, every output), then ``kw`` over it."""
    a = dict(ro=P, rd=P, z=P, n_rays=4, n_samples=8, chunk_rows=4, code_index=None, bits=P, g=32, lo=-1.0,
             inv_cell=16.0, workspace=P, count=P, sample_index=P, pts=P, vdir=P, code_out=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


CULL_EINVAL = {
    "null ro": dict(ro=None),
    "null rd": dict(rd=None),
    "null z": dict(z=None),
    "null bits": dict(bits=None),
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
    "g 0": dict(g=0),
    "g 48": dict(g=48),
    "g 544": dict(g=544),
    "workspace misaligned": dict(workspace=P_ODD),
    "count misaligned": dict(count=P_ODD),
}


@pytest.mark.parametrize("case", sorted(CULL_EINVAL))
def test_cull_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_occupancy_cull(*_cull(**CULL_EINVAL[case])) == _lib.CN_EINVAL, case
    # the optional pointers do not rescue a bad call
    assert lib.cn_occupancy_cull(*_cull(code_out=None, **CULL_EINVAL[case])) == _lib.CN_EINVAL, case


def _expand(**kw):
    a = dict(raw_compact=P, workspace=P, n_rays=4, n_samples=8, raw=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


EXPAND_EINVAL = {
    "null workspace": dict(workspace=None),
    "null raw": dict(raw=None),
    "raw misaligned": dict(raw=P_ODD),
    "raw misaligned, no compact rows": dict(raw=P_ODD, raw_compact=None),
    "raw_compact misaligned": dict(raw_compact=P_ODD),
    "workspace misaligned": dict(workspace=P_ODD),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-1),
    "n_samples 0": dict(n_samples=0),
    "n_samples 513": dict(n_samples=513),
    "rows past int32": dict(n_rays=1 << 23, n_samples=256),
}


@pytest.mark.parametrize("case", sorted(EXPAND_EINVAL))
def test_expand_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_occupancy_expand(*_expand(**EXPAND_EINVAL[case])) == _lib.CN_EINVAL, case


def test_workspace_query(lib):
    """Offsets (int32 per ray, padded to 16 B) and ceil(S / 64) 64-bit mask words per ray; -1 for the
    sizes cn_occupancy_cull refuses."""
    for n, s in ((1, 1), (37, 64), (50, 3), (9, 192), (5, 512), (16384, 64), (10000, 65)):
        want = (4 * n + 15) // 16 * 16 + n * ((s + 63) // 64) * 8
        assert lib.cn_occupancy_cull_workspace_bytes(n, s) == want, (n, s)
    for n, s in ((0, 64), (-1, 64), (16, 0), (16, -3), (16, 513), (1 << 23, 256), (1 << 31, 1)):
        assert lib.cn_occupancy_cull_workspace_bytes(n, s) == -1, (n, s)
    assert lib.cn_occupancy_cull_workspace_bytes((1 << 31) - 1, 1) > 0
