"""The iso-surface entries' host side: the symbols are exported and every argument rule of
include/codenerf.h is refused before any launch -- with dummy (never dereferenced) pointers and no
device."""
import ctypes
import os
import subprocess

import pytest

import isosurface_cases as IC
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

ENTRIES = ("cn_isosurface_workspace_bytes", "cn_isosurface_count", "cn_isosurface_emit")


def test_isosurface_symbols_exported(lib):
    from codenerf import _lib
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "codenerf.h")).read()
    for name in ENTRIES:
        assert name + "(" in header, name


def _count(**kw):
    a = dict(nodes=P, n=33, iso=0.5, workspace=P, counts=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


COUNT_EINVAL = {
    "null nodes": dict(nodes=None),
    "null workspace": dict(workspace=None),
    "null counts": dict(counts=None),
    "n 0": dict(n=0),
    "n 1": dict(n=1),
    "n negative": dict(n=-33),
    "n 514": dict(n=514),
    "n 2^31": dict(n=1 << 31),
    "iso nan": dict(iso=float("nan")),
    "iso inf": dict(iso=float("inf")),
    "iso -inf": dict(iso=float("-inf")),
    "workspace misaligned": dict(workspace=P_ODD),
    "counts misaligned": dict(counts=P_ODD),
}


@pytest.mark.parametrize("case", sorted(COUNT_EINVAL))
def test_count_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_isosurface_count(*_count(**COUNT_EINVAL[case])) == _lib.CN_EINVAL, case


def _emit(**kw):
    a = dict(nodes=P, axis=P, n=33, iso=0.5, workspace=P, max_vertices=100, max_faces=200, vertices=P, faces=P,
             stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


EMIT_EINVAL = {
    "null nodes": dict(nodes=None),
    "null axis": dict(axis=None),
    "null workspace": dict(workspace=None),
    "null vertices with a capacity": dict(vertices=None),
    "null faces with a capacity": dict(faces=None),
    "n 1": dict(n=1),
    "n negative": dict(n=-2),
    "n 514": dict(n=514),
    "iso nan": dict(iso=float("nan")),
    "iso inf": dict(iso=float("inf")),
    "max_vertices negative": dict(max_vertices=-1),
    "max_faces negative": dict(max_faces=-1),
    "max_vertices negative, no output": dict(max_vertices=-1, vertices=None),
    "max_faces negative, no output": dict(max_faces=-1, faces=None),
    "workspace misaligned": dict(workspace=P_ODD),
}


@pytest.mark.parametrize("case", sorted(EMIT_EINVAL))
def test_emit_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_isosurface_emit(*_emit(**EMIT_EINVAL[case])) == _lib.CN_EINVAL, case
    # a skipped output does not rescue a bad call
    if "vertices" not in case:
        assert lib.cn_isosurface_emit(*_emit(max_vertices=0, vertices=None, **EMIT_EINVAL[case])) == _lib.CN_EINVAL, case


def test_workspace_query(lib):
    """Three 32-bit words per node and two per workgroup of 256 nodes, each array padded to 16 B; -1
    outside 2..513."""
    pad16 = lambda b: (b + 15) // 16 * 16
    for n in (2, 33, 513):
        want = 3 * pad16(4 * n ** 3) + 2 * pad16(4 * ((n ** 3 + 255) // 256))
        assert lib.cn_isosurface_workspace_bytes(n) == want == IC.workspace_bytes(n), n
    for n in (1, 514, 0, -5):
        assert lib.cn_isosurface_workspace_bytes(n) == -1, n
