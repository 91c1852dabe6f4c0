"""The folded fp32 inference kernel (CN_FMT_F32_W16_FOLD: fc_out's feature rows folded into layer_dir1,
W_f = W_dir1[:, :256] W_out[1:, :256], c_v1 = W_dir1[:, :256] c_feat + b_dir1).

Integer-exact: on every forward probe of tests/exact_cases.py the folded kernel returns the float64
reference bit for bit (tests/test_fold_cases_cpu.py proves that it must).  sigma keeps the unfolded
kernel's bits on any weights.  rgb is held to the tolerances of the existing inference tests of the same
quantities (test_gpu_parity.test_mlp_forward_rows, test_gpu_configs.test_trained_mlp,
test_gpu_parity.test_field_large_arguments_inference), none widened.  With CN_FOLD_PARITY=<path> the
rgb parity test also writes its figures there as JSON (the folded and the unfolded kernel's largest
error against a float64 evaluation, recorded, not asserted)."""
import json
import os

import pytest
import torch

import exact_cases as E
from conftest import margin
from test_fold_cases_cpu import fold_cases, fold_terms
from test_gpu_field_exact import FD, FX, code_bias, geo_inputs, ident, on_dev, packed, same
from test_gpu_grad import dev  # noqa: F401
from test_gpu_parity import LARGE_ARG_RTOL, _large_arg_case, embedders, load, maxdiff

pytestmark = pytest.mark.gpu

FOLD = "f32_w16_fold"
RAW_RTOL = 1e-5          # test_gpu_configs.RAW_RTOL: trained-magnitude raw, relative to the largest |raw|
RAW_ATOL = 1e-4          # test_gpu_parity.test_mlp_forward_rows: hash-initialised weights, absolute


def field(dev, params, cb, fmt, d, case_like):
    """The field in ``fmt`` ("f32_w16" or the folded format) on device inputs ``d`` -> raw (m, 4)."""
    from codenerf import ops
    fb = ops.fold_bias(params, cb) if fmt == FOLD else None
    pk = ops.mlp_pack(params, fmt)
    if case_like["mode"] == "enc":
        return ops.mlp_forward(pk, cb, d["x"], d.get("code_index"), precision=fmt, fold_bias=fb)
    raw = ops.radiance_field(pk, cb, d["rd"], case_like["s"], case_like["chunk"], FX, FD,
                             code_index=d.get("code_index"), precision=fmt, fold_bias=fb, **geo_inputs(case_like, d))
    return raw.reshape(-1, 4)


# ---------------------------------------------------------------- integer-exact


def run_exact(dev, case):
    from codenerf import ops
    d, ref = on_dev(dev, case), E.reference(case)
    cb = code_bias(dev, case)
    fb = ops.fold_bias(d["params"], cb)
    same(fb, fold_terms(case)["c_v1"], "fold_bias")
    pk = packed(dev, case, FOLD)
    if case["mode"] == "enc":
        raw = ops.mlp_forward(pk, cb, d["x"], d["code_index"], precision=FOLD, fold_bias=fb)
    else:
        raw = ops.radiance_field(pk, cb, d["rd"], case["s"], case["chunk"], FX, FD, code_index=d["code_index"],
                                 precision=FOLD, fold_bias=fb, **geo_inputs(case, d))
    same(raw.reshape(-1, 4), ref["raw"], "raw")


@pytest.mark.parametrize("case", fold_cases()[:-1], ids=ident)
def test_fold_exact(dev, case):
    """Encoded rows (the model set, the dense models, every size around the wave and the tile with the three
    code layouts) and geometry from points and from rays + depths (short last chunks, chunks that are no
    multiple of the tile, a second tile): raw and the fold bias equal the float64 reference."""
    run_exact(dev, case)


def test_fold_exact_second_tile_of_every_workgroup(dev):
    """m = 128 (CUs + 3) + 5: every persistent workgroup takes a second tile, the last tile is ragged."""
    m = E.persistent_rows(torch.cuda.get_device_properties(dev).multi_processor_count)
    case = E.encoded_case(0, m, "index")
    E.check_exact(case, backward=False)
    run_exact(dev, case)


# ---------------------------------------------------------------- sigma bits


@pytest.mark.parametrize("mode", ["enc", "pts", "rayz"])
@pytest.mark.parametrize("r,s,chunk,layout", [(37, 8, 10, "per_row"), (3, 64, 2, "one")])
def test_fold_sigma_bits(dev, mode, r, s, chunk, layout):
    """raw[..., 3] of the folded kernel is the unfolded "f32_w16" kernel's, every bit, on hash-initialised
    weights and random geometry (the same chunks 0..9, ReLU, sigma_partial, butterfly and bias add)."""
    from codenerf import ops, synthetic
    g = torch.Generator().manual_seed(1000 * r + s)
    params = [t.to(dev) for t in synthetic.codenerf_params(0).values()]
    m = r * s
    owners = m if mode == "enc" else r
    n = 1 if layout == "one" else owners
    cb = ops.code_bias(params, synthetic.latent_codes(5, n).to(dev), synthetic.latent_codes(6, n).to(dev))
    d = dict(x=torch.randn(m, 90, generator=g).to(dev), rd=torch.randn(r, 3, generator=g).to(dev),
             ro=torch.randn(r, 3, generator=g).to(dev), z=(0.8 + torch.rand(r, s, generator=g)).to(dev),
             pts=torch.randn(r, s, 3, generator=g).to(dev))
    like = dict(mode=mode, s=s, chunk=chunk)
    a, b = field(dev, params, cb, FOLD, d, like), field(dev, params, cb, "f32_w16", d, like)
    assert bool(torch.isfinite(a).all()) and bool(a[:, 3].any())
    assert torch.equal(a[:, 3], b[:, 3])


# ---------------------------------------------------------------- rgb parity


def _rows_case(dev, kind):
    """-> (state dict, z_s, z_t, x (M, 90), fp32 reference raw, bound on max |raw - reference|)."""
    from codenerf import synthetic
    from oracle import codenerf_oracle as O
    if kind == "hash":
        # test_gpu_parity.test_mlp_forward_rows at 1000 rows
        torch.manual_seed(1000)
        x = torch.randn(1000, 90)
        p = synthetic.codenerf_params(0)
        zs, zt = synthetic.latent_codes(1, 1).expand(1000, -1), synthetic.latent_codes(2, 1).expand(1000, -1)
        return p, zs, zt, x, O.codenerf_mlp(p, zs, zt, x, 63), RAW_ATOL
    # test_gpu_configs.test_trained_mlp: the reference's own outputs on trained-magnitude weights
    g = load("render_trained.npz", "cpu")
    p = synthetic.trained_params(0, kind)
    ref = g[kind + "_mlp_raw"]
    return (p, synthetic.trained_codes(7, 1000, kind), synthetic.trained_codes(8, 1000, kind), g["x"], ref,
            RAW_RTOL * ref.abs().max().item())


@pytest.mark.parametrize("kind", ["hash", "t4", "t3"])
def test_fold_rgb_parity(dev, kind):
    """The folded kernel's raw against the fp32 reference at the existing tests' tolerance; its and the
    unfolded kernel's largest error against a float64 evaluation are recorded next to it."""
    from codenerf import ops
    from oracle import codenerf_oracle as O
    p, zs, zt, x, ref, bound = _rows_case(dev, kind)
    params = [t.to(dev) for t in p.values()]
    if zs.stride(0) == 0:
        zs, zt = zs[:1], zt[:1]
    cb = ops.code_bias(params, zs.contiguous().to(dev), zt.contiguous().to(dev))
    d, like = dict(x=x.to(dev)), dict(mode="enc")
    got = {fmt: field(dev, params, cb, fmt, d, like).cpu() for fmt in (FOLD, "f32_w16")}
    rows = x.shape[0]
    ref64 = O.codenerf_mlp({k: v.double() for k, v in p.items()}, zs.expand(rows, -1).double(),
                           zt.expand(rows, -1).double(), x.double(), 63)
    rec = {"case": kind, "rows": rows, "max_abs_raw": ref.abs().max().item(), "bound_vs_fp32_reference": bound,
           "fold_vs_fp32_reference": maxdiff(got[FOLD], ref), "unfolded_vs_fp32_reference": maxdiff(got["f32_w16"], ref),
           "fold_vs_float64": maxdiff(got[FOLD], ref64), "unfolded_vs_float64": maxdiff(got["f32_w16"], ref64),
           "fp32_reference_vs_float64": maxdiff(ref, ref64)}
    print("FOLD_PARITY " + json.dumps(rec))
    path = os.environ.get("CN_FOLD_PARITY")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert torch.equal(got[FOLD][:, 3], got["f32_w16"][:, 3])
    margin(f"fold_rgb_parity[{kind}]", "raw", rec["fold_vs_fp32_reference"], bound)


# ---------------------------------------------------------------- the sincosf path


def fold_model(dev, params, fold=True):
    from codenerf.models import CodeNeRFModel
    m = CodeNeRFModel(256, 1, 256, 256, 10, 4)
    m.load_state_dict(params)
    m.precision, m.fold = "f32", fold
    return m.to(dev).eval()


@pytest.mark.parametrize("case", ["far", "mixed"])
def test_fold_large_arguments(dev, case):
    """|x| 2^9 > 2^14 in every wave ("far") or in one ("mixed"): the folded instantiation's up-front sincosf
    encodings, as test_gpu_parity.test_field_large_arguments_inference checks the unfolded kernel's."""
    from codenerf import synthetic
    from codenerf.nerf import forward_pass
    from oracle import codenerf_oracle as O
    r, s = 300, 64
    rd, pts = _large_arg_case(case, r, s, 11)
    assert float(pts.abs().max()) * 2 ** 9 > 2 ** 14
    zs, zt = synthetic.latent_codes(3, r), synthetic.latent_codes(4, r)
    ref = O.forward_pass(synthetic.codenerf_params(0), O.EmbedCfg(), rd, pts, zs, zt)
    mdl = fold_model(dev, synthetic.codenerf_params(0))
    assert mdl.inference_format() == FOLD
    with torch.no_grad():
        got = forward_pass(mdl, embedders(dev), rd.to(dev), pts.to(dev), (zs.to(dev), zt.to(dev)))
    margin(f"fold_large_args_{case}", "raw rel", maxdiff(got, ref) / ref.abs().max().item(), LARGE_ARG_RTOL["f32"],
           max_abs_x=float(pts.abs().max()))


# ---------------------------------------------------------------- pack and bias units


def test_fold_bias_against_float64(dev):
    """ops.fold_bias on real weights: W_dir1[:, :256] c_feat + b_dir1 in float64 rounded to fp32, within one
    ulp (the kernel's double sums run in another order)."""
    from codenerf import ops, synthetic
    p = synthetic.trained_params(0, "t3")
    params = [t.to(dev) for t in p.values()]
    cb = ops.code_bias(params, synthetic.trained_codes(7, 33, "t3").to(dev), synthetic.trained_codes(8, 33, "t3").to(dev))
    got = ops.fold_bias(params, cb).cpu()
    want = (cb.cpu().double()[:, 256:512] @ p["layer_dir1.weight"].double()[:, :256].t()
            + p["layer_dir1.bias"].double()).float()
    lo = torch.nextafter(want, torch.full_like(want, -float("inf")))
    hi = torch.nextafter(want, torch.full_like(want, float("inf")))
    assert got.shape == (33, 256) and bool(((got >= lo) & (got <= hi)).all())


def test_fold_pack_follows_weight_changes(dev):
    """After an in-place change of one fc_out weight and of one layer_dir1 weight the model's next inference
    output is that of a fresh model with those weights: the cached folded pack is not reused."""
    from codenerf import synthetic
    p = synthetic.codenerf_params(0)
    torch.manual_seed(5)
    x = torch.randn(200, 90).to(dev)
    zs, zt = synthetic.latent_codes(1, 1).to(dev).expand(200, -1), synthetic.latent_codes(2, 1).to(dev).expand(200, -1)
    m = fold_model(dev, p)
    with torch.no_grad():
        before = m(zs, zt, x)
        assert FOLD in m._packs
        m.fc_out.weight[5, 7] += 0.25
        m.layer_dir1.weight[9, 11] -= 0.5
        after = m(zs, zt, x)
        p2 = {k: v.clone() for k, v in p.items()}
        p2["fc_out.weight"][5, 7] += 0.25
        p2["layer_dir1.weight"][9, 11] -= 0.5
        fresh = fold_model(dev, p2)(zs, zt, x)
    assert not torch.equal(after, before)
    assert torch.equal(after, fresh)


def test_fold_packs_are_cached_per_format(dev):
    """A model that alternates density and forward keeps both packs (no repack per call)."""
    from codenerf import synthetic
    m = fold_model(dev, synthetic.codenerf_params(0))
    x = torch.randn(64, 90).to(dev)
    zs, zt = synthetic.latent_codes(1, 1).to(dev).expand(64, -1), synthetic.latent_codes(2, 1).to(dev).expand(64, -1)
    with torch.no_grad():
        raw, sigma = m(zs, zt, x), m.density(zs, x)
        ptrs = {f: v[1].data_ptr() for f, v in m._packs.items()}
        raw2, sigma2 = m(zs, zt, x), m.density(zs, x)
    assert set(ptrs) == {FOLD, "f32_w16"} and ptrs == {f: v[1].data_ptr() for f, v in m._packs.items()}
    assert torch.equal(raw, raw2) and torch.equal(sigma, sigma2) and torch.equal(raw[:, 3], sigma)


# ---------------------------------------------------------------- opt-out


def test_fold_opt_out(dev, monkeypatch):
    """With the fold disabled the model runs today's kernel: its output is ops.radiance_field(...,
    precision="f32_w16") bit for bit; CODENERF_FOLD=0 makes that the default."""
    from codenerf import ops, synthetic
    from codenerf.models import CodeNeRFModel
    from codenerf.nerf import forward_pass
    p = synthetic.codenerf_params(0)
    torch.manual_seed(9)
    r, s = 37, 8
    rd, pts = torch.randn(r, 3).to(dev), torch.randn(r, s, 3).to(dev)
    zs, zt = synthetic.latent_codes(3, 1).to(dev), synthetic.latent_codes(4, 1).to(dev)
    off = fold_model(dev, p, fold=False)
    assert off.inference_format() == "f32_w16"
    with torch.no_grad():
        got = forward_pass(off, embedders(dev), rd, pts, (zs.expand(r, -1), zt.expand(r, -1)))
        params = [t.detach() for t in off.param_list()]
        want = ops.radiance_field(ops.mlp_pack(params, "f32_w16"), ops.code_bias(params, zs, zt), rd, s, r, FX, FD,
                                  pts=pts, precision="f32_w16")
        on = forward_pass(fold_model(dev, p), embedders(dev), rd, pts, (zs.expand(r, -1), zt.expand(r, -1)))
    assert torch.equal(got, want)
    assert torch.equal(on[..., 3], want[..., 3]) and not torch.equal(on, want)
    monkeypatch.setenv("CODENERF_FOLD", "0")
    assert CodeNeRFModel(256, 1, 256, 256, 10, 4).fold is False
    monkeypatch.delenv("CODENERF_FOLD")
    assert CodeNeRFModel(256, 1, 256, 256, 10, 4).fold is True


# ---------------------------------------------------------------- ABI


def test_fold_abi_refusals(dev):
    """The old entry points refuse the folded format and the new ones every other, before any other check
    (all pointers NULL here: nothing could launch)."""
    from codenerf import _lib
    lib = _lib.load()
    fold = _lib.CN_FMT_F32_W16_FOLD
    assert _lib.FORMATS[FOLD] == fold == 6
    assert lib.cn_mlp_packed_floats(fold) == 28 * 8192 + 1024
    U, I = _lib.CN_EUNSUPPORTED, _lib.CN_EINVAL
    fwd = [None, None, 1, None, 1, None, None]                          # code_bias .. stream
    rf = [None, None, 1, None, None, None, None, 1, 1, 1, None, None, None, None]
    assert lib.cn_mlp_forward(None, fold, *fwd) == U
    assert lib.cn_radiance_field(None, fold, *rf) == U
    for name, fmt in _lib.FORMATS.items():
        if fmt == fold:
            continue
        want = I if name.endswith("_t") else U                          # a transposed pack is no forward format
        assert lib.cn_mlp_forward_fold(None, fmt, None, *fwd) == want, name
        assert lib.cn_radiance_field_fold(None, fmt, None, None, *rf[1:]) == want, name
    assert lib.cn_mlp_forward_fold(None, 99, None, *fwd) == I
    # the folded format with missing arguments: CN_EINVAL, still no launch
    assert lib.cn_mlp_forward_fold(None, fold, None, *fwd) == I
    assert lib.cn_radiance_field_fold(None, fold, None, None, *rf[1:]) == I
    assert lib.cn_fold_bias(None, None, 1, None, None) == I
