"""cn_density_gradient's host side: the symbol is exported, declared and in the ctypes table, and every
argument rule of include/codenerf.h is refused before any launch -- with dummy (never dereferenced)
pointers and no device."""
import ctypes
import os
import re
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
F32_W16, F32_W16_T = 3, 4


def _args(**kw):
    """A valid points-mode call (one code row, 4 rays x 8 samples), then ``kw`` over it."""
    a = dict(packed=P, packed_t=P, fmt=F32_W16, fmt_t=F32_W16_T, code_bias=P, code_index=None, n_codes=1, pts=P,
             ro=None, rd=None, z=None, n_rays=4, n_samples=8, freqs_xyz=FREQS, grad_sigma=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


def test_density_gradient_symbol(lib):
    from codenerf import _lib
    assert hasattr(lib, "cn_density_gradient")
    assert (_lib.CN_FMT_F32_W16, _lib.CN_FMT_F32_W16_T) == (F32_W16, F32_W16_T)
    assert "cn_density_gradient" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cn_density_gradient"][1]) == len(_args())
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "codenerf.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+cn_density_gradient\s*\(([^)]*)\)\s*;", header)
    assert decl, "include/codenerf.h does not declare cn_density_gradient"
    names = [p.split()[-1].lstrip("*") for p in decl.group(1).split(",")]
    assert names == ["packed", "packed_t", "fmt", "fmt_t", "code_bias", "code_index", "n_codes", "pts", "ro", "rd",
                     "z", "n_rays", "n_samples", "freqs_xyz", "grad_sigma", "stream"]


RAYS = dict(pts=None, ro=P, rd=P, z=P)
EINVAL_CASES = {
    "null packed": dict(packed=None),
    "null packed_t": dict(packed_t=None),
    "null code_bias": dict(code_bias=None),
    "null freqs_xyz": dict(freqs_xyz=None),
    "null grad_sigma": dict(grad_sigma=None),
    "no input mode": dict(pts=None),
    "pts and rays": dict(ro=P, rd=P, z=P),
    "pts and a lone z": dict(z=P),
    "rays without z": dict(pts=None, ro=P, rd=P),
    "rays without rd": dict(pts=None, ro=P, z=P),
    "rays without ro": dict(pts=None, rd=P, z=P),
    "grad_sigma misaligned": dict(grad_sigma=P_ODD),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-4),
    "n_samples 0": dict(n_samples=0),
    "n_samples negative": dict(n_samples=-1),
    "n_codes 0": dict(n_codes=0),
    "codes neither 1 nor n_rays": dict(n_codes=3),
    "codes per sample, not per ray": dict(n_codes=32),
    "sample count overflows": dict(n_rays=1 << 40, n_samples=1 << 40),
    "unknown fmt": dict(fmt=99),
    "unknown fmt_t": dict(fmt_t=99),
    "negative fmt": dict(fmt=-1),
    "the two packs swapped": dict(fmt=F32_W16_T, fmt_t=F32_W16),
    "two forward formats": dict(fmt_t=F32_W16),
    "two transposed formats": dict(fmt=F32_W16_T),
    "swapped in the 3xbf16 formats": dict(fmt=2, fmt_t=1),
}


# every case from the points call; those that say nothing about the geometry from the ray call too
_GEOMETRY_KEYS = ("pts", "ro", "rd", "z")
EINVAL_PARAMS = [(c, "pts") for c in sorted(EINVAL_CASES)] + \
    [(c, "rays") for c in sorted(EINVAL_CASES) if not any(k in EINVAL_CASES[c] for k in _GEOMETRY_KEYS)]


@pytest.mark.parametrize("case,mode", EINVAL_PARAMS)
def test_density_gradient_argument_errors(lib, case, mode):
    from codenerf import _lib
    kw = dict(EINVAL_CASES[case])
    if mode == "rays":
        kw.update(RAYS)
    assert lib.cn_density_gradient(*_args(**kw)) == _lib.CN_EINVAL, case


@pytest.mark.parametrize("mode", ["pts", "rays"])
@pytest.mark.parametrize("fmt,fmt_t", [("f32", "f32_w16_t"), ("bf16x3", "bf16x3_t"), ("bf16x3_w16", "bf16x3_t"),
                                       ("f32_w16", "bf16x3_t"), ("bf16x3", "f32_w16_t"),
                                       ("f32_w16_fold", "f32_w16_t")])
def test_density_gradient_other_pairs_unsupported(lib, fmt, fmt_t, mode):
    """Valid arguments with a forward / transposed pair that has no gradient kernel: CN_EUNSUPPORTED."""
    from codenerf import _lib
    geo = RAYS if mode == "rays" else {}
    f = dict(fmt=_lib.FORMATS[fmt], fmt_t=_lib.FORMATS[fmt_t])
    assert lib.cn_density_gradient(*_args(**f, **geo)) == _lib.CN_EUNSUPPORTED
    # per-ray and indexed codes are valid too
    assert lib.cn_density_gradient(*_args(n_codes=4, **f, **geo)) == _lib.CN_EUNSUPPORTED
    assert lib.cn_density_gradient(*_args(n_codes=3, code_index=P, **f, **geo)) == _lib.CN_EUNSUPPORTED


def test_density_gradient_argument_errors_come_first(lib):
    """A bad argument in an unsupported pair is still an invalid argument."""
    from codenerf import _lib
    assert lib.cn_density_gradient(*_args(fmt=_lib.CN_FMT_BF16X3, fmt_t=_lib.CN_FMT_BF16X3_T, n_rays=0)) \
        == _lib.CN_EINVAL
