"""cn_view_rows_bytes / cn_view_rows / cn_radiance_field_fold_rows, host side: the symbols are exported and
every argument rule of include/codenerf.h is refused before any launch -- with dummy (never dereferenced)
pointers and no device."""
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
FX = (ctypes.c_float * 10)(*[2.0 ** k for k in range(10)])
FD = (ctypes.c_float * 4)(*[2.0 ** k for k in range(4)])
FOLD = 6
ENTRIES = ("cn_view_rows_bytes", "cn_view_rows", "cn_radiance_field_fold_rows")


def _rows_args(**kw):
    """A valid cn_view_rows call (4 rays), then ``kw`` over it."""
    a = dict(packed=P, fmt=FOLD, fold_bias=P, rd=P, n_rays=4, freqs_dir=FD, view_rows=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


def _field_args(**kw):
    """A valid ray-mode cn_radiance_field_fold_rows call (one code row, 4 rays x 8 samples), then ``kw``."""
    a = dict(packed=P, fmt=FOLD, code_bias=P, fold_bias=P, view_rows=P, code_index=None, n_codes=1, pts=None, ro=P,
             rd=P, z=P, n_rays=4, n_samples=8, chunk_rows=4, freqs_xyz=FX, freqs_dir=FD, raw=P, stream=None)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return list(a.values())


def test_symbols_exported(lib):
    from codenerf import _lib
    assert _lib.CN_FMT_F32_W16_FOLD == FOLD
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_view_rows_bytes(lib):
    """1 KiB per ray; -1 for a count the entries refuse or a size past int64."""
    for n in (1, 37, 262144, (1 << 31) - 1):
        assert lib.cn_view_rows_bytes(n) == 1024 * n, n
    assert lib.cn_view_rows_bytes(262144) == 256 << 20
    for n in (0, -1, (1 << 63) - 1, ((1 << 63) - 1) // 1024 + 1):
        assert lib.cn_view_rows_bytes(n) == -1, n
    assert lib.cn_view_rows_bytes(((1 << 63) - 1) // 1024) > 0


ROWS_EINVAL = {
    "null packed": dict(packed=None),
    "null fold_bias": dict(fold_bias=None),
    "null rd": dict(rd=None),
    "null freqs_dir": dict(freqs_dir=None),
    "null view_rows": dict(view_rows=None),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-4),
    "n_rays past int64 bytes": dict(n_rays=(1 << 62)),
    "view_rows misaligned": dict(view_rows=P_ODD),
    "fold_bias misaligned": dict(fold_bias=P_ODD),
    "packed misaligned": dict(packed=P_ODD),
    "unknown fmt": dict(fmt=99),
    "a backward pack": dict(fmt=4),
}


@pytest.mark.parametrize("case", sorted(ROWS_EINVAL))
def test_view_rows_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_view_rows(*_rows_args(**ROWS_EINVAL[case])) == _lib.CN_EINVAL, case


FIELD_EINVAL = {
    "null packed": dict(packed=None),
    "null code_bias": dict(code_bias=None),
    "null fold_bias": dict(fold_bias=None),
    "null view_rows": dict(view_rows=None),
    "null rd": dict(rd=None),
    "null raw": dict(raw=None),
    "null freqs_xyz": dict(freqs_xyz=None),
    "null freqs_dir": dict(freqs_dir=None),
    "no points": dict(ro=None, z=None),
    "rays without z": dict(z=None),
    "rays without ro": dict(ro=None),
    "n_rays 0": dict(n_rays=0),
    "n_rays negative": dict(n_rays=-4),
    "n_samples 0": dict(n_samples=0),
    "n_samples negative": dict(n_samples=-8),
    "n_rays n_samples past int64": dict(n_rays=1 << 40, n_samples=1 << 40),
    "more tiles than a grid": dict(n_rays=1 << 31, n_samples=1 << 8),
    "chunk_rows 0": dict(chunk_rows=0),
    "chunk_rows negative": dict(chunk_rows=-1),
    "n_codes 0": dict(n_codes=0),
    "one code row per ray": dict(n_codes=4),
    "two code rows": dict(n_codes=2),
    "a code_index": dict(code_index=P),
    "a code_index over several rows": dict(code_index=P, n_codes=3),
    "raw misaligned": dict(raw=P_ODD),
    "view_rows misaligned": dict(view_rows=P_ODD),
    "fold_bias misaligned": dict(fold_bias=P_ODD),
    "unknown fmt": dict(fmt=99),
    "a backward pack": dict(fmt=4),
}


@pytest.mark.parametrize("case", sorted(FIELD_EINVAL))
def test_field_rows_argument_errors(lib, case):
    from codenerf import _lib
    assert lib.cn_radiance_field_fold_rows(*_field_args(**FIELD_EINVAL[case])) == _lib.CN_EINVAL, case
    if "pts" not in FIELD_EINVAL[case] and "no points" != case and "rays without" not in case:
        # the same rule with the points given
        assert lib.cn_radiance_field_fold_rows(*_field_args(pts=P, ro=None, z=None, **{
            k: v for k, v in FIELD_EINVAL[case].items() if k not in ("ro", "z")})) == _lib.CN_EINVAL, case


@pytest.mark.parametrize("fmt", ["f32", "bf16x3", "f32_w16", "bf16x3_w16"])
def test_other_formats_unsupported(lib, fmt):
    """Valid arguments in a forward format that is not the folded pack: CN_EUNSUPPORTED, before any other
    check and without a launch (as cn_radiance_field_fold)."""
    from codenerf import _lib
    f = _lib.FORMATS[fmt]
    assert lib.cn_view_rows(*_rows_args(fmt=f)) == _lib.CN_EUNSUPPORTED
    assert lib.cn_radiance_field_fold_rows(*_field_args(fmt=f)) == _lib.CN_EUNSUPPORTED
    assert lib.cn_radiance_field_fold_rows(*_field_args(fmt=f, n_codes=4)) == _lib.CN_EUNSUPPORTED
    assert lib.cn_view_rows(*_rows_args(fmt=f, n_rays=0)) == _lib.CN_EUNSUPPORTED
