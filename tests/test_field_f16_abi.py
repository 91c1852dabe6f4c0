"""CN_FMT_F16 at the C ABI, with no device: the format number, the pack size, the argument errors of the two
forward entries that run it and the refusal of every entry that does not -- called through ctypes with dummy
(never dereferenced) pointers as tests/test_field_api_status.py does, every case breaking a rule before any
launch.  The refusals are those an inference-only forward format (CN_FMT_BF16X3_W16) already gets."""
import os
import re

import pytest

from conftest import ROOT
from test_field_api_status import BASE, E, P, P_ODD, U, _call, lib  # noqa: F401

F16 = 7
BF16X3_W16, F32_W16_T = 5, 4


def test_format_number_header_and_binding_agree():
    from codenerf import _lib
    header = open(os.path.join(ROOT, "include", "codenerf.h")).read()
    assert re.search(r"^#define CN_FMT_F16 7$", header, flags=re.M)
    assert _lib.CN_FMT_F16 == _lib.FORMATS["f16"] == F16
    assert _lib.kernel_format("f16") == "f16"
    assert not any(k.endswith("_t") for k, v in _lib.FORMATS.items() if v == F16)
    assert sorted(_lib.FORMATS.values()) == list(range(8))


def test_packed_floats(lib):
    n = lib.cn_mlp_packed_floats(F16)
    # 36 chunks of 2 k-steps x 8 blocks x 64 lanes x 8 fp16 (16 KiB), then 1024 fp32 constants
    assert n == 36 * 4096 + 1024
    assert lib.cn_mlp_packed_floats(8) == -1


def test_inference_format_never_folds():
    from codenerf.models.model import inference_format

    class M:
        precision, fold = "f16", True

        def kernel_format(self):
            from codenerf._lib import kernel_format
            return kernel_format(self.precision)
    assert inference_format(M()) == "f16"


RAY = dict(fmt=F16)
FORWARD_ERRORS = {
    "cn_radiance_field": [
        ("null packed", dict(packed=None)), ("null code_bias", dict(code_bias=None)), ("null rd", dict(rd=None)),
        ("null raw", dict(raw=None)), ("raw off by 4 bytes", dict(raw=P_ODD)), ("null freqs_xyz", dict(freqs_xyz=None)),
        ("null freqs_dir", dict(freqs_dir=None)), ("n_rays = 0", dict(n_rays=0)), ("n_samples = -1", dict(n_samples=-1)),
        ("chunk_rows = 0", dict(chunk_rows=0)), ("n_codes = 0", dict(n_codes=0)),
        ("no geometry", dict(pts=None, ro=None)), ("two code rows, three rays, no index", dict(n_codes=2)),
        ("m over the tile bound", dict(n_rays=2 ** 31, n_samples=128)),
        ("sample count overflows", dict(n_rays=2 ** 62, n_samples=4))],
    "cn_mlp_forward": [
        ("null packed", dict(packed=None)), ("null code_bias", dict(code_bias=None)), ("null x", dict(x=None)),
        ("null raw", dict(raw=None)), ("raw off by 4 bytes", dict(raw=P_ODD)), ("m = 0", dict(m=0)),
        ("n_codes = -1", dict(n_codes=-1)), ("two code rows for 48 rows, no index", dict(n_codes=2)),
        ("m over the tile bound", dict(m=2 ** 38))],
}


@pytest.mark.parametrize("fn,case", [(fn, name) for fn, rows in FORWARD_ERRORS.items() for name, _ in rows])
def test_forward_argument_errors(lib, fn, case):
    (kw,), = [(kw,) for name, kw in FORWARD_ERRORS[fn] if name == case]
    assert _call(lib, fn, RAY, kw) == E, (fn, case)


def test_pack_argument_errors(lib):
    assert _call(lib, "cn_mlp_pack", RAY, dict(packed=None)) == E
    assert _call(lib, "cn_mlp_pack", RAY, dict(params=None)) == E


# entry -> (base arguments, status): what CN_FMT_BF16X3_W16 gets there today
REFUSALS = {
    "cn_mlp_forward_fold": ({}, U), "cn_radiance_field_fold": ({}, U), "cn_radiance_field_fold_rows": ({}, U),
    "cn_view_rows": ({}, U),
    "cn_radiance_field_counted": (dict(pts=P, ro=None, z=None, n_samples=1, n_rows_max=3, count=P), E),
    "cn_radiance_field_fold_counted": (dict(pts=P, ro=None, z=None, n_samples=1, n_rows_max=3, count=P), E),
    "cn_density_field_counted": (dict(pts=P, ro=None, rd=None, z=None, n_samples=1, n_rows_max=3, count=P), E),
    "cn_density_field": (dict(x=None), U),
    "cn_density_gradient": (dict(fmt_t=F32_W16_T), U),
    "cn_radiance_field_masks_fmt": ({}, E), "cn_radiance_field_train_fmt": ({}, E),
}


@pytest.mark.parametrize("fn", sorted(REFUSALS))
def test_other_entries_refuse_the_format(lib, fn):
    base, want = REFUSALS[fn]
    assert _call(lib, fn, base, dict(fmt=F16)) == want
    assert _call(lib, fn, base, dict(fmt=BF16X3_W16)) == want, "the inference-only 3xbf16 format's status"


def test_backward_and_size_entries_refuse_the_format(lib):
    for fn in ("cn_field_backward_fused", "cn_field_backward_fused_ws"):
        assert _call(lib, fn, {}, dict(fmt_t=F16)) == E
    assert lib.cn_field_mask_words_fmt(F16, 128) == -1
    assert lib.cn_field_train_saved_floats(F16, 128) == -1
    assert lib.cn_field_backward_fused_workspace_floats(F16, 3, 16) == lib.cn_field_backward_fused_workspace_floats(
        BF16X3_W16, 3, 16)
    # cn_fold_bias takes no format: the folded rows exist for the fp32 folded pack alone
    assert _call(lib, "cn_fold_bias", {}, dict(code_bias=None)) == E
