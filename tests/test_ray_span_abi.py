"""cn_sample_span's host side: the symbol is exported and every argument rule of include/codenerf.h is refused
before any launch -- with dummy (never dereferenced) device pointers and no device."""
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


P = 0x10000                           # a dummy device address nothing reads
INF, NAN = float("inf"), float("nan")


def test_sample_span_symbol_exported(lib):
    from codenerf import _lib
    assert hasattr(lib, "cn_sample_span") and "cn_sample_span" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cn_sample_span"][1]) == 17
    header = open(os.path.join(ROOT, "include", "codenerf.h")).read()
    assert "int cn_sample_span(" in header


def _span(k=1, bits=None, g=None, lo=None, inv_cell=None, host_null=(), **kw):
    """A valid call (4 rays, K grids of 32^3, 64 probes, 8 samples, every output), then the overrides: ``bits``,
    ``g``, ``lo``, ``inv_cell`` lists of K host values, ``host_null`` names of host arrays passed as NULL."""
    host = dict(bits=(ctypes.c_void_p * 8)(*(bits if bits is not None else [P] * k)),
                g=(ctypes.c_int64 * 8)(*(g if g is not None else [32] * k)),
                lo=(ctypes.c_float * 8)(*(lo if lo is not None else [-1.0] * k)),
                inv_cell=(ctypes.c_float * 8)(*(inv_cell if inv_cell is not None else [16.0] * k)))
    host["bits"] = ctypes.cast(host["bits"], ctypes.POINTER(ctypes.c_void_p))
    host["g"] = ctypes.cast(host["g"], ctypes.POINTER(ctypes.c_int64))
    host["lo"] = ctypes.cast(host["lo"], ctypes.POINTER(ctypes.c_float))
    host["inv_cell"] = ctypes.cast(host["inv_cell"], ctypes.POINTER(ctypes.c_float))
    for name in host_null:
        host[name] = None
    dev = ctypes.c_void_p(P)
    a = dict(ro=dev, rd=dev, n_rays=4, bits=host["bits"], g=host["g"], lo=host["lo"], inv_cell=host["inv_cell"],
             n_objects=k, near=0.5, far=2.0, n_probes=64, nc=8, t_rand=None, z_out=dev, span=dev, probe_range=dev,
             stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


EINVAL = {
    "null ro": dict(ro=None),
    "null rd": dict(rd=None),
    "null z_out": dict(z_out=None),
    "null span": dict(span=None),
    "null probe_range": dict(probe_range=None),
    "null bits array": dict(host_null=("bits",)),
    "null g array": dict(host_null=("g",)),
    "null lo array": dict(host_null=("lo",)),
    "null inv_cell array": dict(host_null=("inv_cell",)),
    "null bits entry": dict(bits=[None]),
    "null bits entry of the third object": dict(k=3, bits=[P, P, None]),
    "no objects": dict(n_objects=0),
    "negative objects": dict(n_objects=-1),
    "nine objects": dict(n_objects=9),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-4),
    "n_probes 0": dict(n_probes=0),
    "n_probes 32": dict(n_probes=32),
    "n_probes 100": dict(n_probes=100),
    "n_probes 1088": dict(n_probes=1088),
    "n_probes negative": dict(n_probes=-64),
    "nc 1": dict(nc=1),
    "nc 0": dict(nc=0),
    "nc 513": dict(nc=513),
    "g 0": dict(g=[0]),
    "g 16": dict(g=[16]),
    "g 48": dict(g=[48]),
    "g 544": dict(g=[544]),
    "g 48 of the second object": dict(k=2, g=[32, 48]),
    "near NaN": dict(near=NAN),
    "near inf": dict(near=INF, far=INF),
    "far NaN": dict(far=NAN),
    "far inf": dict(far=INF),
    "near negative": dict(near=-0.5),
    "far equal to near": dict(near=1.0, far=1.0),
    "far below near": dict(near=1.0, far=0.5),
    "inv_cell NaN": dict(inv_cell=[NAN]),
    "inv_cell inf": dict(inv_cell=[INF]),
    "inv_cell inf of the eighth object": dict(k=8, inv_cell=[16.0] * 7 + [INF]),
    "lo NaN": dict(lo=[NAN]),
    "lo -inf": dict(lo=[-INF]),
}


@pytest.mark.parametrize("case", sorted(EINVAL))
def test_sample_span_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_sample_span(*_span(**EINVAL[case])) == _lib.CN_EINVAL, case
    # the optional t_rand does not rescue a bad call
    assert lib.cn_sample_span(*_span(t_rand=ctypes.c_void_p(P), **EINVAL[case])) == _lib.CN_EINVAL, case
