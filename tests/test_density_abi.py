"""cn_density_field's host side: the symbol is exported and every argument rule of include/codenerf.h
is refused before any launch -- with dummy (never dereferenced) pointers and no device."""
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
FREQS = (ctypes.c_float * 10)(*[2.0 ** k for k in range(10)])
F32_W16 = 3


def _args(**kw):
    """A valid points-mode call (one code row, 4 rays x 8 samples, both outputs), then ``kw`` over it."""
    a = dict(packed=P, fmt=F32_W16, code_bias=P, code_index=None, n_codes=1, pts=P, ro=None, rd=None, z=None,
             x=None, x_stride=0, n_rays=4, n_samples=8, freqs_xyz=FREQS, sigma=P, raw=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


def test_density_symbol_exported(lib):
    from codenerf import _lib
    assert hasattr(lib, "cn_density_field")
    assert _lib.CN_FMT_F32_W16 == F32_W16 and "cn_density_field" in _lib.SIGNATURES


EINVAL_CASES = {
    "null packed": dict(packed=None),
    "null code_bias": dict(code_bias=None),
    "null freqs_xyz": dict(freqs_xyz=None),
    "no input mode": dict(pts=None),
    "pts and rays": dict(ro=P, rd=P, z=P),
    "pts and x": dict(x=P, x_stride=63),
    "rays and x": dict(pts=None, ro=P, rd=P, z=P, x=P, x_stride=90),
    "all three modes": dict(ro=P, rd=P, z=P, x=P, x_stride=63),
    "rays without z": dict(pts=None, ro=P, rd=P),
    "rays without rd": dict(pts=None, ro=P, z=P),
    "rays without ro": dict(pts=None, rd=P, z=P),
    "both outputs null": dict(sigma=None, raw=None),
    "raw misaligned": dict(raw=P_ODD),
    "raw misaligned, no sigma": dict(sigma=None, raw=P_ODD),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-4),
    "n_samples 0": dict(n_samples=0),
    "n_codes 0": dict(n_codes=0),
    "x_stride 62": dict(pts=None, x=P, x_stride=62),
    "x_stride 0": dict(pts=None, x=P, x_stride=0),
    "codes neither 1 nor n_rays": dict(n_codes=3),
    "codes per sample, not per ray": dict(n_codes=32),
}


@pytest.mark.parametrize("case", sorted(EINVAL_CASES))
def test_density_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_density_field(*_args(**EINVAL_CASES[case])) == _lib.CN_EINVAL, case


@pytest.mark.parametrize("fmt", ["f32", "bf16x3", "bf16x3_w16"])
@pytest.mark.parametrize("mode", ["pts", "rays", "x"])
def test_density_other_formats_unsupported(lib, fmt, mode):
    """Valid arguments in a format without a density kernel: CN_EUNSUPPORTED, before any launch."""
    from codenerf import _lib
    geo = {"pts": {}, "rays": dict(pts=None, ro=P, rd=P, z=P), "x": dict(pts=None, x=P, x_stride=90)}[mode]
    assert lib.cn_density_field(*_args(fmt=_lib.FORMATS[fmt], **geo)) == _lib.CN_EUNSUPPORTED
    # a sigma-only call (raw NULL counts as aligned) and per-ray / indexed codes are valid too
    assert lib.cn_density_field(*_args(fmt=_lib.FORMATS[fmt], raw=None, n_codes=4, **geo)) == _lib.CN_EUNSUPPORTED
    assert lib.cn_density_field(*_args(fmt=_lib.FORMATS[fmt], sigma=None, n_codes=3, code_index=P, **geo)) \
        == _lib.CN_EUNSUPPORTED


def test_density_unknown_format_is_invalid(lib):
    from codenerf import _lib
    assert lib.cn_density_field(*_args(fmt=99)) == _lib.CN_EINVAL
    # the transposed packs are the backward's: not a forward format
    assert lib.cn_density_field(*_args(fmt=_lib.CN_FMT_F32_W16_T)) == _lib.CN_EINVAL
