"""The status every field entry point returns for a broken argument rule (csrc/field_api.hip's field_args,
encoded_args and fused_backward_args, and the entries' own rules), called through ctypes with dummy
(never dereferenced) pointers and no device: every case breaks at least one rule, so none reaches a launch.

The expected statuses are written out by hand from include/codenerf.h and the entry points as they stood
before their checks moved into one place; the rows that name two broken rules pin where CN_EUNSUPPORTED
sits among the CN_EINVAL checks.  test_sample_count_overflow_is_invalid is the one intended difference:
n_rays * n_samples past int64 was undefined behaviour in the entries that multiplied first."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

E, U = -1, -2          # CN_EINVAL, CN_EUNSUPPORTED
F32, BF16X3, BF16X3_T, F32_W16, F32_W16_T, BF16X3_W16, FOLD = range(7)


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the HIP runtime must come from torch's copy, as in production)
    from codenerf import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "code-nerf_amd", "csrc"), "-j8"], check=True)
    assert (_lib.CN_EINVAL, _lib.CN_EUNSUPPORTED) == (E, U)
    assert [_lib.FORMATS[k] for k in ("f32", "bf16x3", "bf16x3_t", "f32_w16", "f32_w16_t", "bf16x3_w16",
                                      "f32_w16_fold")] == list(range(7))
    return _lib.load(_lib.LIB_PATH)


# Dummy device pointers: aligned addresses nothing reads.  The frequency tables and the parameter table are
# read on the host once the checks pass, so they are real arrays.
P = ctypes.c_void_p(0x10000)
P_ODD = ctypes.c_void_p(0x10004)      # 4-B aligned only
FX = (ctypes.c_float * 10)(*[2.0 ** k for k in range(10)])
FD = (ctypes.c_float * 4)(*[2.0 ** k for k in range(4)])
PARAMS = (ctypes.c_void_p * 18)(*[0x10000] * 18)
PARAMS_HOLE = (ctypes.c_void_p * 18)(*([0x10000] * 17 + [None]))

# Every argument any of the entries takes: rays + depths, one code row, n_rays=3, n_samples=16, chunk_rows=2.
BASE = dict(packed=P, packed_t=P, code_bias=P, fold_bias=P, view_rows=P, code_index=None, n_codes=1, pts=None, ro=P,
            rd=P, z=P, x=P, x_stride=90, m=48, n_rays=3, n_samples=16, chunk_rows=2, freqs_xyz=FX, freqs_dir=FD,
            raw=P, save=P, saved=P, x_enc=P, masks=P, sigma=P, grad_sigma=P, d_raw=P, g_code=P, d_pts=None, d_ro=P,
            d_rd=P, workspace=P, params=PARAMS, grads=None, stream=None)

_HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "codenerf.h")).read(), flags=re.S)


def _names(fn):
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % fn, _HEADER)
    assert decl, f"include/codenerf.h does not declare {fn}"
    return [p.split()[-1].lstrip("*") for p in decl.group(1).split(",")]


def _call(lib, fn, base, kw):
    from codenerf import _lib
    a = dict(BASE, **base)
    a.update(kw)
    struct = {"cn_field_backward_fused_multi": _lib.FieldFusedBwd,
              "cn_field_backward_train_multi": _lib.FieldTrainBwd}.get(fn)
    if struct is None:
        return getattr(lib, fn)(*[a[n] for n in _names(fn)])
    # one field, its arguments in the struct
    vals = []
    for name, ct in struct._fields_:
        v = a[name]
        vals.append(ctypes.cast(v, ct) if isinstance(v, ctypes.Array) else v)
    fields = (struct * 1)(struct(*vals))
    tail = (None, None) if fn == "cn_field_backward_fused_multi" else (None,)
    return getattr(lib, fn)(a["fmt_t"], fields, 1, *tail)


# ---------------------------------------------------------------- the rules, entry by entry

def _rows(ptrs, sizes, misaligned=(), codes=True, geometry=True, tile=True, extra=()):
    """The rows most entries share: each required pointer null, each size 0 and -1, no geometry form, two
    code rows for three rays without code_index, each vector-accessed buffer 4 B off, m over the tile bound."""
    r = [(f"null {p}", {p: None}, E) for p in ptrs]
    r += [(f"{s} = {v}", {s: v}, E) for s in sizes for v in (0, -1)]
    if geometry:
        r += [("no geometry: neither pts nor ro", dict(pts=None, ro=None), E),
              ("no geometry: neither pts nor z", dict(pts=None, z=None), E)]
    if codes:
        r += [("two code rows, three rays, no code_index", dict(n_codes=2), E)]
    r += [(f"{p} off by 4 bytes", {p: P_ODD}, E) for p in misaligned]
    if tile:
        r += [("m over the tile bound", dict(n_rays=2 ** 31, n_samples=128), E)]
    return r + list(extra)


RAY_PTRS = ("packed", "code_bias", "rd", "raw", "freqs_xyz", "freqs_dir")
RAY_SIZES = ("n_rays", "n_samples", "chunk_rows", "n_codes")

# the forward formats' rule: the fold entries take CN_FMT_F32_W16_FOLD alone, the others every forward
# format but that one (CN_EUNSUPPORTED), before every other check; a transposed or unknown format is invalid
FWD_FMT = [("a transposed format", dict(fmt=F32_W16_T), E), ("the other transposed format", dict(fmt=BF16X3_T), E),
           ("an unknown format", dict(fmt=99), E), ("a negative format", dict(fmt=-1), E),
           ("the folded pack at a plain entry", dict(fmt=FOLD), U),
           ("the folded pack, and n_rays = 0 as well", dict(fmt=FOLD, n_rays=0, m=0), U),
           ("the folded pack, and a null output as well", dict(fmt=FOLD, raw=None), U)]
FOLD_FMT = [("a transposed format", dict(fmt=F32_W16_T), E), ("an unknown format", dict(fmt=99), E),
            ("a plain pack at a fold entry", dict(fmt=F32_W16), U),
            ("a plain pack, and n_rays = 0 as well", dict(fmt=F32, n_rays=0, m=0), U),
            ("a plain pack, and a misaligned fold_bias as well", dict(fmt=BF16X3, fold_bias=P_ODD), U)]
# the training / mask forwards run in two formats; anything else is invalid
TWO_FMT = [("a transposed format", dict(fmt=F32_W16_T), E), ("another forward format", dict(fmt=F32), E),
           ("the folded pack", dict(fmt=FOLD), E), ("an unknown format", dict(fmt=99), E)]

# the fused backwards: one code row per wave (32 samples 3xbf16, 16 fp32), refused as CN_EUNSUPPORTED after the
# pointer and size checks and before the tile bound and d_raw's alignment
BWD_PTRS = ("packed_t", "masks", "d_raw", "rd", "g_code", "freqs_xyz", "freqs_dir")
PER_RAY = dict(n_codes=3)      # = n_rays: the code rule itself holds
BWD = [("d_pts without pts", dict(d_pts=P), E),
       ("d_ro with pts", dict(pts=P), E),
       ("d_ro without z", dict(z=None, pts=P), E),
       ("a forward format", dict(fmt_t=F32_W16), E), ("the other forward format", dict(fmt_t=BF16X3), E),
       ("an unknown format", dict(fmt_t=99), E)] + \
      [(f"a code row per ray, {s} samples, fmt_t {f}", dict(PER_RAY, n_samples=s, fmt_t=f), U)
       for s in (8, 24) for f in (BF16X3_T, F32_W16_T)] + \
      [("a code row per ray, 16 samples in 32-sample waves", dict(PER_RAY, fmt_t=BF16X3_T), U),
       ("waves across rays, and a null g_code as well", dict(PER_RAY, n_samples=8, g_code=None), E),
       ("waves across rays, and n_rays = 0 as well", dict(n_codes=3, code_index=P, n_samples=8, n_rays=0), E),
       ("waves across rays, and d_pts without pts as well", dict(PER_RAY, n_samples=8, d_pts=P), E),
       ("waves across rays, and d_raw off by 4 bytes as well", dict(PER_RAY, n_samples=8, d_raw=P_ODD), U),
       ("waves across rays, and m over the tile bound as well",
        dict(n_codes=3, code_index=P, n_rays=2 ** 31, n_samples=136), U)]
BWD_ROWS = _rows(BWD_PTRS, RAY_SIZES, misaligned=("d_raw",), extra=BWD)

# the density entries: exactly one of pts, (ro, rd, z) and x; the format's CN_EUNSUPPORTED after every argument check
DENSITY = [("pts and rays", dict(pts=P), E), ("rays without rd", dict(rd=None), E), ("rays without z", dict(z=None), E),
           ("rays without ro", dict(ro=None), E), ("no input mode", dict(ro=None, rd=None, z=None), E),
           ("sample count overflows", dict(n_rays=1 << 40, n_samples=1 << 40), E)]

ENTRIES = {
    "cn_radiance_field": (dict(fmt=F32_W16), _rows(RAY_PTRS, RAY_SIZES, misaligned=("raw",), extra=FWD_FMT)),
    "cn_radiance_field_fold": (dict(fmt=FOLD), _rows(RAY_PTRS + ("fold_bias",), RAY_SIZES,
                                                     misaligned=("raw", "fold_bias"), extra=FOLD_FMT)),
    "cn_radiance_field_fold_rows": (dict(fmt=FOLD), _rows(
        RAY_PTRS + ("fold_bias", "view_rows"), RAY_SIZES, misaligned=("raw", "fold_bias", "view_rows"), codes=False,
        extra=FOLD_FMT + [("two code rows", dict(n_codes=2), E), ("a code row per ray", dict(n_codes=3), E),
                          ("a code_index", dict(code_index=P), E),
                          ("sample count overflows", dict(n_rays=1 << 40, n_samples=1 << 40), E)])),
    "cn_radiance_field_train": ({}, _rows(RAY_PTRS + ("save",), RAY_SIZES, misaligned=("raw",))),
    "cn_radiance_field_masks_fmt": (dict(fmt=BF16X3), _rows(RAY_PTRS + ("masks",), RAY_SIZES, misaligned=("raw",),
                                                            extra=TWO_FMT)),
    "cn_radiance_field_train_fmt": (dict(fmt=F32_W16), _rows(RAY_PTRS + ("save", "masks"), RAY_SIZES,
                                                             misaligned=("raw",), extra=TWO_FMT)),
    "cn_density_field": (dict(fmt=F32_W16, x=None), _rows(
        ("packed", "code_bias", "freqs_xyz"), ("n_rays", "n_samples", "n_codes"), misaligned=("raw",), geometry=False,
        extra=DENSITY + [("neither sigma nor raw", dict(sigma=None, raw=None), E),
                         ("rays and x", dict(x=P), E),
                         ("x rows shorter than 63", dict(ro=None, rd=None, z=None, x=P, x_stride=62), E),
                         ("a transposed format", dict(fmt=F32_W16_T), E), ("an unknown format", dict(fmt=99), E),
                         ("a format without a density kernel", dict(fmt=F32), U),
                         ("the folded pack", dict(fmt=FOLD), U),
                         ("no density kernel, and n_rays = 0 as well", dict(fmt=F32, n_rays=0), E),
                         ("no density kernel, and a misaligned raw as well", dict(fmt=BF16X3, raw=P_ODD), E)])),
    "cn_density_gradient": (dict(fmt=F32_W16, fmt_t=F32_W16_T), _rows(
        ("packed", "packed_t", "code_bias", "freqs_xyz", "grad_sigma"), ("n_rays", "n_samples", "n_codes"),
        misaligned=("grad_sigma",), geometry=False,
        extra=DENSITY + [("a transposed format as fmt", dict(fmt=F32_W16_T), E),
                         ("a forward format as fmt_t", dict(fmt_t=F32_W16), E),
                         ("the two packs swapped", dict(fmt=F32_W16_T, fmt_t=F32_W16), E),
                         ("an unknown fmt", dict(fmt=99), E), ("an unknown fmt_t", dict(fmt_t=99), E),
                         ("a pair without a gradient kernel", dict(fmt=BF16X3, fmt_t=BF16X3_T), U),
                         ("no gradient kernel, and n_samples = 0 as well", dict(fmt=F32, n_samples=0), E),
                         ("no gradient kernel, and the tile bound as well",
                          dict(fmt=F32, n_rays=2 ** 31, n_samples=128), E)])),
    "cn_encode_inputs": ({}, _rows(("rd", "x", "freqs_xyz", "freqs_dir"), ("n_rays", "n_samples", "chunk_rows"),
                                   codes=False, tile=False)),
    "cn_field_backward_fused": (dict(fmt_t=F32_W16_T), BWD_ROWS),
    "cn_field_backward_fused_ws": (dict(fmt_t=F32_W16_T), BWD_ROWS),
    "cn_field_backward_fused_multi": (dict(fmt_t=F32_W16_T), BWD_ROWS),
    "cn_field_backward_train_multi": (dict(fmt_t=F32_W16_T), BWD_ROWS + [
        ("null params", dict(params=None), E), ("a null parameter", dict(params=PARAMS_HOLE), E),
        ("null saved", dict(saved=None), E), ("null workspace", dict(workspace=None), E),
        ("waves across rays, and a null parameter as well", dict(PER_RAY, n_samples=8, params=PARAMS_HOLE), E),
        ("waves across rays, and a null workspace as well", dict(PER_RAY, n_samples=8, workspace=None), E)]),
    "cn_mlp_forward": (dict(fmt=F32_W16), _rows(
        ("packed", "code_bias", "x", "raw"), ("m", "n_codes"), misaligned=("raw",), geometry=False, tile=False,
        extra=FWD_FMT + [("m over the tile bound", dict(m=2 ** 38), E)])),
    "cn_mlp_forward_fold": (dict(fmt=FOLD), _rows(
        ("packed", "code_bias", "fold_bias", "x", "raw"), ("m", "n_codes"), misaligned=("raw", "fold_bias"),
        geometry=False, tile=False, extra=FOLD_FMT + [("m over the tile bound", dict(m=2 ** 38), E)])),
    "cn_mlp_forward_train": ({}, _rows(
        ("packed", "code_bias", "x", "raw", "save"), ("m", "n_codes"), misaligned=("raw",), geometry=False, tile=False,
        extra=[("m over the tile bound", dict(m=2 ** 38), E)])),
}

# encoded rows: the code rule is against m (48 rows here)
for _fn in ("cn_mlp_forward", "cn_mlp_forward_fold", "cn_mlp_forward_train"):
    ENTRIES[_fn][1][:] = [r for r in ENTRIES[_fn][1] if r[0] != "two code rows, three rays, no code_index"] + \
        [("two code rows for 48 rows without code_index", dict(n_codes=2), E)]

CASES = [(fn, name) for fn, (_, rows) in ENTRIES.items() for name, _, _ in rows]


def test_case_names_are_unique():
    assert len(set(CASES)) == len(CASES)


@pytest.mark.parametrize("fn,case", CASES)
def test_status(lib, fn, case):
    base, rows = ENTRIES[fn]
    (kw, want), = [(kw, want) for name, kw, want in rows if name == case]
    assert _call(lib, fn, base, kw) == want, (fn, case)


@pytest.mark.parametrize("fn", ["cn_field_backward_fused", "cn_field_backward_fused_ws",
                                "cn_field_backward_fused_multi", "cn_field_backward_train_multi"])
@pytest.mark.parametrize("fmt_t", [BF16X3_T, F32_W16_T])
def test_backward_points_form_rules(lib, fn, fmt_t):
    """The same two gradient rules from the points form: d_pts is then allowed, d_ro is not."""
    pts = dict(ENTRIES[fn][0], fmt_t=fmt_t, pts=P, ro=None, z=None, d_ro=None, d_pts=P)
    assert _call(lib, fn, pts, dict(d_ro=P)) == E
    assert _call(lib, fn, pts, dict(rd=None)) == E
    assert _call(lib, fn, pts, dict(PER_RAY, n_samples=8)) == U


# The entries that formed n_rays * n_samples before any bound on it.  Every other entry already refused this.
OVERFLOW_ENTRIES = ["cn_radiance_field", "cn_radiance_field_fold", "cn_radiance_field_train",
                    "cn_radiance_field_masks_fmt", "cn_radiance_field_train_fmt", "cn_encode_inputs",
                    "cn_field_backward_fused", "cn_field_backward_fused_ws", "cn_field_backward_fused_multi",
                    "cn_field_backward_train_multi"]


@pytest.mark.parametrize("fn", OVERFLOW_ENTRIES)
def test_sample_count_overflow_is_invalid(lib, fn):
    """n_rays = 2^62, n_samples = 4: the product does not fit int64 -> CN_EINVAL (new with field_args: the
    product used to be formed first, which is signed overflow)."""
    assert _call(lib, fn, ENTRIES[fn][0], dict(n_rays=2 ** 62, n_samples=4)) == E
