"""The folded kernel's per-ray view-direction rows (cn_view_rows, cn_radiance_field_fold_rows; the
``view_rows`` keyword of ops.radiance_field).

Under Q1 a sample's view direction is that of ray k mod Rc of its chunk, so layer_dir1's view-direction
term is per-ray work: the table holds, per ray, c_v1 + W_dir1[:, 256:] enc(d) as the folded kernel's
accumulators hold it after the view-direction chunk, and the table variant starts from it.  The contract is
bit identity: forced on and forced off return the same raw for finite directions, whichever samples share a
wave.  The table variant streams 27 weight chunks per tile through the 4-slot ring with a counter that runs
on across a workgroup's tiles; the ring test walks it through all four phases and past its fold."""
import pytest
import torch

import buffers as B
import exact_cases as E
from test_gpu_field_exact import FD, FX, code_bias, geo_inputs, ident, on_dev, packed, same
from test_gpu_grad import dev  # noqa: F401

pytestmark = pytest.mark.gpu

FOLD = "f32_w16_fold"
U = 2.0 ** -24


def hash_model(dev, n_codes=1):
    """Hash-initialised weights, their folded pack, code terms of ``n_codes`` rows and the fold bias."""
    from codenerf import ops, synthetic
    params = [t.to(dev) for t in synthetic.codenerf_params(0).values()]
    cb = ops.code_bias(params, synthetic.latent_codes(5, n_codes).to(dev), synthetic.latent_codes(6, n_codes).to(dev))
    return params, ops.mlp_pack(params, FOLD), cb, ops.fold_bias(params, cb)


def random_rays(dev, r, s, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(rd=torch.randn(r, 3, generator=g).to(dev), ro=torch.randn(r, 3, generator=g).to(dev),
                z=(0.8 + torch.rand(r, s, generator=g)).to(dev), pts=torch.randn(r, s, 3, generator=g).to(dev))


def field(pk, cb, fb, d, s, chunk, mode="rayz", **kw):
    from codenerf import ops
    geo = dict(pts=d["pts"]) if mode == "pts" else dict(ro=d["ro"], z=d["z"])
    return ops.radiance_field(pk, cb, d["rd"], s, chunk, FX, FD, precision=FOLD, fold_bias=fb, **geo, **kw)


# ---------------------------------------------------------------- forced on against forced off

# (rays, samples, chunk_rows): a last chunk of 5 rays and a wrap inside a wave; Rc no multiple of 16 and M
# no multiple of the 128-sample tile; Rc < 16: several wraps per wave
RAGGED = ((37, 64, 16), (50, 3, 50), (19, 5, 7))


@pytest.mark.parametrize("mode", ["rayz", "pts"])
@pytest.mark.parametrize("r,s,chunk", RAGGED)
def test_forced_on_equals_forced_off(dev, r, s, chunk, mode):
    """The whole raw output, one code row, hash-initialised weights, random geometry: every bit."""
    params, pk, cb, fb = hash_model(dev)
    d = random_rays(dev, r, s, 1000 * r + s)
    on = field(pk, cb, fb, d, s, chunk, mode, view_rows=True)
    off = field(pk, cb, fb, d, s, chunk, mode, view_rows=False)
    assert bool(torch.isfinite(off).all()) and bool(off[..., :3].any())
    assert torch.equal(on, off)


def test_direction_bits_do_not_depend_on_the_wave(dev):
    """One point per wave beyond fast_sincosf's range sends that wave to the up-front sincosf path; the
    finite directions of its other samples keep their encoding's bits, so the table path (whose rows never
    see a point) still equals the in-kernel path, NaN-free rows and all."""
    params, pk, cb, fb = hash_model(dev)
    r, s, chunk = 37, 8, 10
    d = random_rays(dev, r, s, 7)
    d["pts"][::5, 3] = 40.0            # 40 x 2^9 > 2^14: out of fast_sincosf's range, finite
    on = field(pk, cb, fb, d, s, chunk, "pts", view_rows=True)
    off = field(pk, cb, fb, d, s, chunk, "pts", view_rows=False)
    assert bool(torch.isfinite(off).all())
    assert torch.equal(on, off)


def test_non_finite_directions_agree_in_nan(dev):
    """A zero or infinite direction normalises to NaN: both paths agree in which outputs are NaN (the ReLU, a
    signed-integer max on the bits, turns a NaN with the sign bit set into 0, so there may be none), sigma
    has no view direction and keeps its bits, and so does every sample whose Q1 direction is finite (the
    samples of a non-finite direction may differ in bits: a NaN's sign decides what the ReLU leaves)."""
    params, pk, cb, fb = hash_model(dev)
    r, s, chunk = 37, 8, 10
    d = random_rays(dev, r, s, 8)
    d["rd"][3] = 0.0
    d["rd"][20, 1] = float("inf")
    on = field(pk, cb, fb, d, s, chunk, "pts", view_rows=True)
    off = field(pk, cb, fb, d, s, chunk, "pts", view_rows=False)
    assert torch.equal(torch.isnan(on), torch.isnan(off))
    assert bool(torch.isfinite(off[..., 3]).all())
    assert torch.equal(on[..., 3], off[..., 3])
    # Q1: sample row k = r' S + s of a chunk of Rc rays takes the direction of the chunk's ray k mod Rc
    ray = torch.arange(r).repeat_interleave(s)
    base = ray // chunk * chunk
    rcnt = torch.clamp(r - base, max=chunk)
    dray = base + ((ray - base) * s + torch.arange(s).repeat(r)) % rcnt
    finite = ~((dray == 3) | (dray == 20)).to(dev)
    assert 0 < int((~finite).sum()) < r * s
    assert torch.equal(on.reshape(-1, 4)[finite], off.reshape(-1, 4)[finite])


# ---------------------------------------------------------------- integer-exact

ONE_CODE_GEOMETRY = [E.geometry_case(i % E.N_GEO_MODELS, mode, r, s, chunk, "one")
                     for i, (r, s, chunk) in enumerate(E.GEOMETRY_SHAPES) for mode in ("pts", "rayz")]


def run_exact(dev, case):
    from codenerf import ops
    d, ref = on_dev(dev, case), E.reference(case)
    cb = code_bias(dev, case)
    fb = ops.fold_bias(d["params"], cb)
    raw = ops.radiance_field(packed(dev, case, FOLD), cb, d["rd"], case["s"], case["chunk"], FX, FD, precision=FOLD,
                             fold_bias=fb, view_rows=True, **geo_inputs(case, d))
    same(raw.reshape(-1, 4), ref["raw"], "raw")


@pytest.mark.parametrize("case", ONE_CODE_GEOMETRY, ids=ident)
def test_exact_geometry(dev, case):
    """The integer-exact geometry shapes of tests/exact_cases.py with one code row, from points and from
    rays, through the table: the float64 reference bit for bit."""
    E.check_exact(case, backward=False)
    run_exact(dev, case)


def test_ring_counter_walks_every_phase(dev):
    """More than 4 x (CU count) tiles: every workgroup walks the 27-chunk stream through all four ring phases,
    some take a fifth tile and fold the mod-108 counter; chunks of 600 rays and a shorter last one (R = 2100 on
    256 CUs: 1050 tiles, a last chunk of 300 rays)."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    s = 64
    r = (4 * cus * 128) // s + 52            # 4 x CUs + 26 tiles
    assert r * s > 4 * 128 * cus
    case = E.geometry_case(1, "rayz", r, s, 600, "one")
    E.check_exact(case, backward=False)
    run_exact(dev, case)


# ---------------------------------------------------------------- the table itself


def table_float64(params, fb, rd):
    """-> (c_v1 + W_dir1[:, 256:] enc(d) in float64, sum of |terms|, sum of |w|) for the fp32-normalised
    directions d (view_dir's op order) and the fp32 arguments d f; PositionalEmbedder's column order."""
    w = params[12].detach().cpu().double()[:, 256:]                      # layer_dir1.weight (256, 283)
    rd = rd.cpu()
    n = torch.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2])
    vd = rd / n[:, None]                                                  # fp32, IEEE: the kernel's bits
    cols = [vd.double()]
    for f in FD:
        arg = (vd * f).double()                                           # f a power of two: exact
        cols += [torch.sin(arg), torch.cos(arg)]
    enc = torch.cat(cols, dim=1)                                          # (R, 27)
    c = fb[0].cpu().double()
    val = c[None, :] + enc @ w.T
    mag = c.abs()[None, :] + enc.abs() @ w.abs().T
    return val, mag, w.abs().sum(dim=1)[None, :]


def test_table_against_float64(dev):
    """ops.view_rows against float64: |error| <= (27 + 3) u (|c_v1| + sum |w e|) + 2 u sum |w|, u = 2^-24 --
    the summation error of a 28-term fp32 chain with one rounding per term, and fast_sincosf's documented
    1.5 ulp on each encoding value.  The worst ratio to the bound is printed (VIEW_ROWS_TABLE)."""
    from codenerf import ops
    params, pk, cb, fb = hash_model(dev)
    rd = random_rays(dev, 203, 1, 3)["rd"]
    got = ops.view_rows(pk, fb, rd, FD)
    assert got.shape == (203, 256)
    val, mag, wsum = table_float64(params, fb, rd)
    bound = (27 + 3) * U * mag + 2 * U * wsum
    ratio = ((got.cpu().double() - val).abs() / bound).max().item()
    print(f"VIEW_ROWS_TABLE worst |error| / bound = {ratio:.4f}")
    assert ratio <= 1.0, ratio


# ---------------------------------------------------------------- dispatch


def test_dispatch(dev, monkeypatch):
    """None takes the table exactly where it pays: rays, one code row, no code_index, S at the crossover or
    above.  Per-ray codes, a code_index, points and S below the crossover compute in the kernel -- seen by
    counting the table builds -- and every choice returns the forced-off call's bits."""
    from codenerf import ops
    built = []
    real = ops._view_rows_table
    monkeypatch.setattr(ops, "_view_rows_table", lambda *a, **k: built.append(1) or real(*a, **k))
    s_hi, s_lo = ops.VIEW_ROWS_MIN_SAMPLES, ops.VIEW_ROWS_MIN_SAMPLES - 1
    assert s_lo >= 1
    r, chunk = 21, 8
    params, pk, cb, fb = hash_model(dev)
    _, _, cbr, fbr = hash_model(dev, r)
    ci = torch.zeros(r, dtype=torch.int64, device=dev)
    for s, mode, c, f, kw, want in ((s_hi, "rayz", cb, fb, {}, 1), (s_lo, "rayz", cb, fb, {}, 0),
                                    (s_hi, "pts", cb, fb, {}, 0), (s_hi, "rayz", cbr, fbr, {}, 0),
                                    (s_hi, "rayz", cb, fb, dict(code_index=ci), 0)):
        d = random_rays(dev, r, s, 11 + s)
        del built[:]
        auto = field(pk, c, f, d, s, chunk, mode, **kw)
        assert len(built) == want, (s, mode, kw, built)
        assert torch.equal(auto, field(pk, c, f, d, s, chunk, mode, view_rows=False, **kw))
    d = random_rays(dev, r, s_hi, 5)
    for c, f, kw in ((cbr, fbr, {}), (cb, fb, dict(code_index=ci))):
        with pytest.raises(ValueError):
            field(pk, c, f, d, s_hi, chunk, view_rows=True, **kw)
    with pytest.raises(AssertionError):
        ops.radiance_field(ops.mlp_pack(params, "f32_w16"), cb, d["rd"], s_hi, chunk, FX, FD, ro=d["ro"], z=d["z"],
                           precision="f32_w16", view_rows=True)


# ---------------------------------------------------------------- buffers


def test_poison_fills(dev):
    """Both fills of tests/buffers.py at one ragged size: ops.view_rows and the table path of
    ops.radiance_field return the same bits under zero and NaN fills (no row is read before it is written),
    no guard is touched (nothing is stored past n_rays rows), and the same holds for the C entries on a
    table the test owns."""
    from codenerf import _lib, ops
    params, pk, cb, fb = hash_model(dev)
    r, s, chunk = 37, 5, 16
    d = random_rays(dev, r, s, 21)
    lib = _lib.load()
    logs, own = {}, {}
    for fill in B.FILLS:
        with B.contracts(fill) as arena:
            ops.view_rows(pk, fb, d["rd"], FD)
            ops.radiance_field(pk, cb, d["rd"], s, chunk, FX, FD, ro=d["ro"], z=d["z"], precision=FOLD,
                               fold_bias=fb, view_rows=True)
            assert lib.cn_view_rows_bytes(r) == r * 1024
            rows = arena.empty((r, 256), torch.float32, dev)
            raw = arena.empty((r, s, 4), torch.float32, dev)
            _lib.check(lib.cn_view_rows(_lib.ptr(pk), _lib.CN_FMT_F32_W16_FOLD, _lib.ptr(fb), _lib.ptr(d["rd"]), r,
                                        _lib.host_floats(FD), _lib.ptr(rows), _lib.stream_of(rows)), "cn_view_rows")
            _lib.check(lib.cn_radiance_field_fold_rows(
                _lib.ptr(pk), _lib.CN_FMT_F32_W16_FOLD, _lib.ptr(cb), _lib.ptr(fb), _lib.ptr(rows), None, 1, None,
                _lib.ptr(d["ro"]), _lib.ptr(d["rd"]), _lib.ptr(d["z"]), r, s, chunk, _lib.host_floats(FX),
                _lib.host_floats(FD), _lib.ptr(raw), _lib.stream_of(raw)), "cn_radiance_field_fold_rows")
            assert arena.n_allocations >= 4
            logs[fill], own[fill] = arena.returns, (rows.clone(), raw.clone())
    assert [name for name, _, _ in logs["zero"]] == ["view_rows", "radiance_field"]
    B.compare_fills(logs["zero"], logs["poison"])
    for a, b in zip(own["zero"], own["poison"]):
        assert not bool(torch.isnan(b).any())
        assert torch.equal(B.tensor_bytes(a), B.tensor_bytes(b))
    assert torch.equal(own["zero"][0], logs["zero"][0][1][0][1])
    assert torch.equal(own["zero"][1], logs["zero"][1][1][0][1])
