"""The counted entries' host side (include/codenerf.h, "Counted field calls"): the four symbols are exported
and declared, and every argument rule is refused with CN_EINVAL before any launch -- with dummy (never
dereferenced) pointers and no device."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

COUNTED = ("cn_radiance_field_counted", "cn_radiance_field_fold_counted", "cn_density_field_counted",
           "cn_scatter_rgb_counted")


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
FX = (ctypes.c_float * 10)(*[2.0 ** k for k in range(10)])
FD = (ctypes.c_float * 4)(*[2.0 ** k for k in range(4)])
F32, BF16X3, BF16X3_T, F32_W16, F32_W16_T, BF16X3_W16, F32_W16_FOLD = range(7)


def test_counted_symbols_exported(lib):
    from codenerf import _lib
    header = open(os.path.join(ROOT, "include", "codenerf.h")).read()
    for name in COUNTED:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert f"int {name}(" in header, name
    # the count travels as a pointer: right after n_samples (fields), after sample_index (scatter)
    for name, at in (("cn_radiance_field_counted", 11), ("cn_radiance_field_fold_counted", 12),
                     ("cn_density_field_counted", 11), ("cn_scatter_rgb_counted", 2)):
        assert _lib.SIGNATURES[name][1][at] is ctypes.c_void_p, name
    assert "k = min(max(count[0], 0), n_rows_max)" in header


def _radiance(**kw):
    """A valid call (300 rows at capacity, one code row), then ``kw`` over it."""
    a = dict(packed=P, fmt=F32_W16, code_bias=P, code_index=None, n_codes=1, pts=P, ro=None, rd=P, z=None,
             n_rows_max=300, n_samples=1, count=P, freqs_xyz=FX, freqs_dir=FD, raw=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


def _fold(**kw):
    a = dict(packed=P, fmt=F32_W16_FOLD, code_bias=P, fold_bias=P, code_index=None, n_codes=1, pts=P, ro=None, rd=P,
             z=None, n_rows_max=300, n_samples=1, count=P, freqs_xyz=FX, freqs_dir=FD, raw=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


def _density(**kw):
    a = dict(packed=P, fmt=F32_W16, code_bias=P, code_index=None, n_codes=1, pts=P, ro=None, rd=None, z=None,
             n_rows_max=300, n_samples=1, count=P, freqs_xyz=FX, sigma=P, raw=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


# the rules the three field entries share
FIELD_EINVAL = {
    "null count": dict(count=None),
    "count misaligned": dict(count=P_ODD),
    "n_samples 0": dict(n_samples=0),
    "n_samples 2": dict(n_samples=2),
    "ro given": dict(ro=P),
    "z given": dict(z=P),
    "ro and z given": dict(ro=P, z=P),
    "null pts": dict(pts=None),
    "capacity 0": dict(n_rows_max=0),
    "capacity negative": dict(n_rows_max=-300),
    "format f32": dict(fmt=F32),
    "format bf16x3": dict(fmt=BF16X3),
    "format bf16x3_w16": dict(fmt=BF16X3_W16),
    "format f32_w16_t": dict(fmt=F32_W16_T),
    "format unknown": dict(fmt=99),
    "one code row per row": dict(n_codes=300),
    "null packed": dict(packed=None),
    "null code_bias": dict(code_bias=None),
    "null freqs_xyz": dict(freqs_xyz=None),
    "raw misaligned": dict(raw=P_ODD8),
}


@pytest.mark.parametrize("case", sorted(FIELD_EINVAL))
def test_field_counted_argument_errors(lib, case):
    from codenerf import _lib
    kw = FIELD_EINVAL[case]
    assert lib.cn_radiance_field_counted(*_radiance(**kw)) == _lib.CN_EINVAL, case
    assert lib.cn_radiance_field_fold_counted(*_fold(**kw)) == _lib.CN_EINVAL, case
    assert lib.cn_density_field_counted(*_density(**kw)) == _lib.CN_EINVAL, case
    if "code_index" not in kw and "n_codes" not in kw:      # a code_index does not rescue a bad call
        assert lib.cn_radiance_field_counted(*_radiance(code_index=P, n_codes=3, **kw)) == _lib.CN_EINVAL, case


def test_each_entry_takes_its_own_format_only(lib):
    from codenerf import _lib
    assert lib.cn_radiance_field_counted(*_radiance(fmt=F32_W16_FOLD)) == _lib.CN_EINVAL
    assert lib.cn_radiance_field_fold_counted(*_fold(fmt=F32_W16)) == _lib.CN_EINVAL
    assert lib.cn_density_field_counted(*_density(fmt=F32_W16_FOLD)) == _lib.CN_EINVAL


RADIANCE_ONLY_EINVAL = {
    "null rd": dict(rd=None),
    "null freqs_dir": dict(freqs_dir=None),
    "null raw": dict(raw=None),
}


@pytest.mark.parametrize("case", sorted(RADIANCE_ONLY_EINVAL))
def test_radiance_counted_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_radiance_field_counted(*_radiance(**RADIANCE_ONLY_EINVAL[case])) == _lib.CN_EINVAL, case
    assert lib.cn_radiance_field_fold_counted(*_fold(**RADIANCE_ONLY_EINVAL[case])) == _lib.CN_EINVAL, case


def test_fold_and_density_own_argument_errors(lib):
    from codenerf import _lib
    assert lib.cn_radiance_field_fold_counted(*_fold(fold_bias=None)) == _lib.CN_EINVAL
    assert lib.cn_radiance_field_fold_counted(*_fold(fold_bias=P_ODD8)) == _lib.CN_EINVAL
    assert lib.cn_density_field_counted(*_density(rd=P)) == _lib.CN_EINVAL               # no view direction
    assert lib.cn_density_field_counted(*_density(sigma=None, raw=None)) == _lib.CN_EINVAL


def _scatter(**kw):
    a = dict(raw_compact=P, sample_index=P, count=P, n_rows_max=8, raw=P, n_slots=32, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


SCATTER_EINVAL = {
    "null count": dict(count=None),
    "count misaligned": dict(count=P_ODD),
    "null raw_compact": dict(raw_compact=None),
    "null sample_index": dict(sample_index=None),
    "null raw": dict(raw=None),
    "capacity 0": dict(n_rows_max=0),
    "capacity negative": dict(n_rows_max=-8),
    "capacity above n_slots": dict(n_rows_max=33),
    "n_slots past int32": dict(n_slots=1 << 31),
    "raw 8-B aligned only": dict(raw=P_ODD8),
    "raw_compact 8-B aligned only": dict(raw_compact=P_ODD8),
}


@pytest.mark.parametrize("case", sorted(SCATTER_EINVAL))
def test_scatter_rgb_counted_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_scatter_rgb_counted(*_scatter(**SCATTER_EINVAL[case])) == _lib.CN_EINVAL, case
