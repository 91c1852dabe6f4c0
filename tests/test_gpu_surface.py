"""Iso-surface ray casting on the device: the three kernels against the numpy rule of tests/surface_cases.py, bit
for bit, on hand-made arrays between guard rows; render_surface end to end against the same rule driven by the
device's own density kernel; the activated level, the occupancy forms, streams and capture, and the refusals."""
import math

import numpy as np
import pytest
import torch

import buffers as B
import occupancy_cases as OC
import streams as ST
import surface_cases as S
from test_gpu_parity import dev, embedders, load, models  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
FX = [2.0 ** k for k in range(10)]
LEVEL = F(0.25)
GUARD = 8                                 # guard rows before and after every output of the kernel tests
CANARY = {torch.float32: 12345.0, torch.int32: 77}
MODULES = B.PATCHED_MODULES + ("codenerf.nerf.surface",)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and \
        np.array_equal(got.view(np.uint8), want.view(np.uint8))


def same(a, b):
    """Bitwise equal torch values, NaN wherever the other has NaN."""
    if not a.is_floating_point():
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


class Guarded:
    """Output buffers between GUARD canary rows; ``check()`` asserts no guard row was touched."""

    def __init__(self, dev):
        self.dev, self.whole = dev, []

    def new(self, shape, dtype=torch.float32, value=None):
        rows = shape[0] + 2 * GUARD
        whole = torch.full((rows,) + tuple(shape[1:]), CANARY[dtype], dtype=dtype, device=self.dev)
        self.whole.append(whole)
        view = whole[GUARD:GUARD + shape[0]]
        if value is not None:
            view.copy_(value)
        return view

    def check(self):
        torch.cuda.synchronize()
        for w in self.whole:
            n = w.shape[0] - 2 * GUARD
            assert bool((w[:GUARD] == CANARY[w.dtype]).all()) and bool((w[GUARD + n:] == CANARY[w.dtype]).all()), \
                ("a guard row was written", tuple(w.shape), w.dtype)


def firsts(r):
    """Class offsets that make R-ray cases cover every class of surface_cases.CLASSES between them."""
    return [0] if r >= len(S.CLASSES) else list(range(0, len(S.CLASSES), r))


def strided(a, stride, dev):
    """``a`` on the device as the surface entries read it: contiguous, or column 3 of (.., 4) rows of junk."""
    if stride == 1:
        return T(a, dev)
    rows = np.full(a.shape + (4,), np.nan, dtype=F)
    rows[..., 0] = 1.0e9
    rows[..., 3] = a
    return T(rows, dev)[..., 3]


# ---------------------------------------------------------------- 1. the kernels against the rule


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("s", [2, 63, 64, 65, 200])
@pytest.mark.parametrize("r", [1, 5, 257])
def test_bracket_bit_exact(dev, r, s, stride):
    from codenerf import ops
    seen, hits = set(), set()
    for first in firsts(r):
        sigma, z, kinds, want = S.class_case(r, s, LEVEL, seed=1000 * r + s, first=first)
        seen |= set(kinds)
        b_want, h_want = S.bracket(sigma, z, LEVEL)
        assert [h for h, _ in want] == h_want.tolist()
        hits |= set(h_want.tolist())
        g = Guarded(dev)
        bracket, hit = g.new((r, 4)), g.new((r,), torch.int32)
        out = ops.surface_bracket(strided(sigma, stride, dev), T(z, dev), float(LEVEL), bracket=bracket, hit=hit)
        assert out[0] is bracket and out[1] is hit
        g.check()
        assert bits_equal(hit.cpu().numpy(), h_want), (first, hit.cpu().numpy(), h_want)
        assert bits_equal(bracket.cpu().numpy(), b_want), (first, kinds)
    assert seen == set(S.CLASSES) and hits == {0, 1, 2}


def test_bracket_fresh_outputs_and_the_s_limit(dev):
    """Without buffers the op allocates its own; S = 1024 is the last size taken."""
    from codenerf import ops
    sigma, z, _, _ = S.class_case(13, 1024, LEVEL, seed=7)
    b_want, h_want = S.bracket(sigma, z, LEVEL)
    with B.contracts("poison") as arena:
        bracket, hit = ops.surface_bracket(T(sigma, dev), T(z, dev), float(LEVEL))
    assert arena.n_allocations == 2
    assert bits_equal(bracket.cpu().numpy(), b_want) and bits_equal(hit.cpu().numpy(), h_want)
    with pytest.raises(AssertionError):
        ops.surface_bracket(torch.zeros(2, 1025, device=dev), torch.zeros(2, 1025, device=dev), 0.5)
    with pytest.raises(AssertionError):
        ops.surface_bracket(torch.zeros(2, 8, device=dev), torch.zeros(2, 8, device=dev), float("nan"))


PROBES = (0.55, 0.25, -0.15, np.nan, -1.0e4, np.inf, -np.inf)      # above, a tie, below, NaN, the marker, +-inf


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("r", [1, 5, 257])
def test_step_bit_exact(dev, r, stride):
    """The first call; two updates whose probes move either end, tie, are NaN, the marker or infinite; a finishing
    update; and a finishing first call (refine = 0), whose low ends are known and unknown."""
    from codenerf import ops
    seen = {"up": 0, "down": 0, "nan": 0, "still": 0, "known": 0, "unknown": 0, "flat": 0}
    for first in firsts(r):
        sigma, z, kinds, _ = S.class_case(r, 65, LEVEL, seed=r, first=first)
        b0, hit = S.bracket(sigma, z, LEVEL)
        ro, rd = S.rays(r, seed=first)
        d_ro, d_rd, d_hit = T(ro, dev), T(rd, dev), T(hit, dev)
        rng = np.random.default_rng(first)
        probes = [np.array([PROBES[(k + shift + first) % len(PROBES)] for k in range(r)], dtype=F)
                  for shift in (0, 3)]
        probes.append((LEVEL + F(0.4) * rng.standard_normal(r)).astype(F))

        g = Guarded(dev)
        bracket, t, pts = g.new((r, 4), value=T(b0, dev)), g.new((r,)), g.new((r, 3))
        out = ops.surface_step(d_ro, d_rd, d_hit, bracket, float(LEVEL), t=t, pts=pts)
        assert out[0] is t and out[1] is pts
        b_want, t_want, p_want = S.step(ro, rd, hit, b0, LEVEL)
        assert bits_equal(bracket.cpu().numpy(), b_want) and bits_equal(t.cpu().numpy(), t_want)
        assert bits_equal(pts.cpu().numpy(), p_want)
        for i, probe in enumerate(probes):
            finish = i == len(probes) - 1
            live = hit == 1
            seen["up"] += int((live & S.reached(probe, LEVEL)).sum())
            seen["down"] += int((live & ~S.reached(probe, LEVEL) & ~np.isnan(probe)).sum())
            seen["nan"] += int((live & np.isnan(probe)).sum())
            seen["still"] += int((~live).sum())
            ops.surface_step(d_ro, d_rd, d_hit, bracket, float(LEVEL), t=t, probe=strided(probe, stride, dev),
                             finish=finish, pts=pts)
            b_next, t_want, p_want = S.step(ro, rd, hit, b_want, LEVEL, t=t_want, probe=probe, finish=finish)
            assert np.array_equal(b_next[~live], b_want[~live], equal_nan=True)     # hit 0 and 2: left alone
            b_want = b_next
            assert bits_equal(bracket.cpu().numpy(), b_want), (first, i)
            assert bits_equal(t.cpu().numpy(), t_want), (first, i)
            assert bits_equal(pts.cpu().numpy(), p_want), (first, i)
        g.check()

        # refine = 0: the finishing call straight from the search bracket, into buffers the op allocates
        bracket = T(b0, dev)
        t, pts = ops.surface_step(d_ro, d_rd, d_hit, bracket, float(LEVEL), finish=True)
        b_want, t_want, p_want = S.step(ro, rd, hit, b0, LEVEL, finish=True)
        assert bits_equal(bracket.cpu().numpy(), b0) and bits_equal(t.cpu().numpy(), t_want)
        assert bits_equal(pts.cpu().numpy(), p_want)
        live = hit == 1
        seen["known"] += int((live & S.known(b0[:, 2])).sum())
        seen["unknown"] += int((live & ~S.known(b0[:, 2])).sum())
        seen["flat"] += int((b0[:, 2] == b0[:, 3]).sum())
    assert all(seen.values()), seen


@pytest.mark.parametrize("r", [1, 5, 257])
def test_shade(dev, r):
    """All three hit values under a background other than white: depth, the points and the missed rows' colour
    bit for bit; a hit row's colour within 1e-6 of sigmoid(raw) 1.002 - 0.001 in float64 (volume_render's own
    tolerance; sigmoid_hw is documented to within 2e-7)."""
    from codenerf import ops
    bg = (0.1, 0.7, 0.25)
    for first in range(3 if r < 3 else 1):
        rng = np.random.default_rng(r + first)
        hit = ((np.arange(r) + first) % 3).astype(np.int32)
        raw = (4.0 * rng.standard_normal((r, 4))).astype(F)
        raw[::7, 0], raw[::5, 1] = 40.0, -40.0                       # saturated channels
        t = (rng.random(r) + 0.5).astype(F)
        pts0 = rng.standard_normal((r, 3)).astype(F)
        rgb_want, depth_want, pts_want = S.shade(raw, hit, t, pts0, bg)
        g = Guarded(dev)
        pts, rgb, depth = g.new((r, 3), value=T(pts0, dev)), g.new((r, 3)), g.new((r,))
        out = ops.surface_shade(T(raw, dev), T(hit, dev), T(t, dev), pts, bg, rgb=rgb, depth=depth)
        assert out[0] is rgb and out[1] is depth
        g.check()
        assert bits_equal(depth.cpu().numpy(), depth_want)
        got_pts = pts.cpu().numpy()
        assert np.array_equal(np.isnan(got_pts), np.isnan(pts_want)) and \
            bits_equal(np.nan_to_num(got_pts), np.nan_to_num(pts_want))
        got = rgb.cpu().numpy()
        miss = hit == 0
        assert bits_equal(got[miss], np.tile(np.array(bg, dtype=F), (int(miss.sum()), 1)))
        if (~miss).any():
            err = float(np.abs(got[~miss].astype(np.float64) - rgb_want[~miss]).max())
            print(f"shade r={r}: max |rgb - exact| = {err:.3e}")
            assert err <= 1e-6
    # the (R, 1, 4) rows a points-form field call returns are taken as they are
    rgb2, _ = ops.surface_shade(T(raw, dev).view(r, 1, 4), T(hit, dev), T(t, dev), T(pts0, dev), bg)
    assert torch.equal(rgb2, rgb)


# ---------------------------------------------------------------- 2. end to end against the rule

R, NS, REFINE = 1024, 64, 6


@pytest.fixture(scope="module")
def scene(dev):
    """The 32 x 32 rays of the render_small.npz camera, the coarse synthetic model, a 64-depth sampler linear in
    depth (spacing_mode "lindisp": quirk Q2's name for it) that PERTURBS (the surface must not), one code and two codes with a per-ray index."""
    from codenerf import synthetic
    from codenerf.models.model import CodeRows
    from codenerf.nerf import PointSampler, RaySampler
    g = load("render_small.npz", dev)
    k = torch.tensor([[28.0, 0, 16.0, 0], [0, 28.0, 16.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    rs = RaySampler(32, 32, k, sample_size=1024, device=dev, datatype=torch.float32)
    ro, rd = (t.reshape(-1, 3).contiguous() for t in rs.get_bundle(g["pose"]))
    assert ro.shape == (R, 3)
    m, = models(dev, (0,))
    sc = dict(ro=ro, rd=rd, m=m, emb=embedders(dev), zs=g["z_s"], zt=g["z_t"],
              ps=PointSampler(NS, 8, 0.8, 1.8, "lindisp", True, torch.float32, dev))
    zs2, zt2 = synthetic.latent_codes(21, 2).to(dev), synthetic.latent_codes(22, 2).to(dev)
    index = (torch.arange(R, device=dev) % 2).to(torch.int64)
    z_s, z_t = zs2[index], zt2[index]
    z_s._cn_code_rows = z_t._cn_code_rows = CodeRows(zs2, zt2, index)
    sc["two"] = (z_s, z_t, zs2, index)
    return sc


def codes_of(sc, codes):
    if codes == "one":
        return sc["zs"].expand(R, -1), sc["zt"].expand(R, -1)
    return sc["two"][0], sc["two"][1]


def surface(sc, level, codes="one", ro=None, rd=None, **kw):
    from codenerf.nerf import render_surface
    zs, zt = codes_of(sc, codes)
    with torch.no_grad():
        return render_surface(sc["ro"] if ro is None else ro, sc["rd"] if rd is None else rd, zs, zt, sc["ps"],
                              sc["emb"], sc["m"], level, **kw)


def search_sigma(sc, codes):
    """The device's own sigma_raw at the unperturbed search depths -> (z (R, S), sigma (R, S), sigma_at)."""
    from codenerf import ops
    from codenerf.models.model import density_code_bias
    ps, m = sc["ps"], sc["m"]
    with torch.no_grad():
        _, z = ops.sample_uniform(sc["ro"], sc["rd"], ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
        if codes == "one":
            cb, index = density_code_bias(m, sc["zs"]), None
        else:
            cb, index = density_code_bias(m, sc["two"][2]), sc["two"][3]

        def sigma_at(pts):
            return ops.density_field(m.packed(), cb, FX, pts=T(pts, z.device), code_index=index).cpu().numpy()

        sigma = ops.density_field(m.packed(), cb, FX, ro=sc["ro"], rd=sc["rd"], z=z, code_index=index)
    return z, sigma, sigma_at


@pytest.fixture(scope="module")
def reference(dev, scene):
    """Per code layout: the search densities, their median as the level, the render and the rule's result."""
    out = {}
    for codes in ("one", "two"):
        z, sigma, sigma_at = search_sigma(scene, codes)
        level = float(sigma.flatten().median())
        got = surface(scene, level, codes, activated=False, refine=REFINE)
        torch.cuda.synchronize()
        want = S.render_surface(scene["ro"].cpu().numpy(), scene["rd"].cpu().numpy(), z.cpu().numpy(), level, REFINE,
                                sigma_at)
        out[codes] = dict(z=z, sigma=sigma, level=level, got=got, want=want)
    return out


@pytest.mark.parametrize("codes", ["one", "two"])
def test_render_surface_is_the_rule(dev, scene, reference, codes):
    from codenerf import nerf
    sc, ref = scene, reference[codes]
    got, want, level = ref["got"], ref["want"], F(ref["level"])
    assert sorted(got) == sorted(["rgb", "depth", "hit", "point", "sigma", "bracket", "z_search", "normal"])
    # the search depths are the sampler's, unperturbed, and the ray form's densities are the points form's
    assert torch.equal(got["z_search"], ref["z"])
    pts_search = S.ray_points(sc["ro"].cpu().numpy(), sc["rd"].cpu().numpy(), ref["z"].cpu().numpy())
    assert bits_equal(search_sigma(sc, codes)[2](pts_search), ref["sigma"].cpu().numpy())
    hit = got["hit"].cpu().numpy()
    counts = {h: int((hit == h).sum()) for h in (0, 1, 2)}
    print(f"render_surface [{codes}]: level {float(level):.6f}, hit counts {counts}")
    assert counts[1] > 0 and (counts[0] > 0 or counts[2] > 0), counts            # crossings and rays without one
    assert bits_equal(hit, want["hit"])
    assert bits_equal(got["bracket"].cpu().numpy(), want["bracket"][:, :2])
    assert bits_equal(got["depth"].cpu().numpy(), want["depth"])
    point = got["point"].cpu().numpy()
    assert np.array_equal(np.isnan(point), np.isnan(want["point"])) and \
        bits_equal(np.nan_to_num(point), np.nan_to_num(want["point"]))
    assert np.array_equal(np.isinf(want["depth"]), hit == 0) and np.array_equal(np.isnan(point).all(axis=1), hit == 0)

    # the bracket's ends hold the densities the rule stored for them
    zs_rows = sc["zs"] if codes == "one" else sc["two"][0]
    ro, rd = sc["ro"].cpu().numpy(), sc["rd"].cpu().numpy()
    live = hit == 1
    b = want["bracket"]
    for col, s_col in ((0, 2), (1, 3)):
        ends = T((ro + rd * b[:, col:col + 1]).astype(F), dev)
        dens = nerf.density(sc["m"], sc["emb"], ends, zs_rows).cpu().numpy()
        rows = live & (S.known(b[:, 2]) if col == 0 else True)
        assert rows.any() and bits_equal(dens[rows], b[rows, s_col]), col
    lo_known = live & S.known(b[:, 2])
    assert np.all(b[lo_known, 2] < level) and np.all(b[live, 3] >= level)
    assert np.all(b[live, 0] <= want["t"][live]) and np.all(want["t"][live] <= b[live, 1])

    # sigma, normal and colour at the point
    some = torch.from_numpy(hit != 0).to(dev)
    assert bool(some.any())
    pts = got["point"][some]
    rows_zs = zs_rows if codes == "one" else zs_rows[some]
    assert torch.equal(got["sigma"][some], nerf.density(sc["m"], sc["emb"], pts, rows_zs))
    assert same(got["normal"][some], nerf.normals(sc["m"], sc["emb"], pts, rows_zs))
    assert bool((got["sigma"][~some] == 0).all()) and bool((got["normal"][~some] == 0).all())
    zs, zt = codes_of(sc, codes)
    with torch.no_grad():
        finite = torch.nan_to_num(got["point"])
        raw = nerf._field(sc["m"], sc["emb"], sc["rd"], zs, zt, chunk_rows=R, pts=finite.view(R, 1, 3))[:, 0, :3]
        # the colour call takes the codes as the density calls do (the distinct rows and the per-ray index):
        # shading the tagged field call's rows gives the render's colours bit for bit
        from codenerf import ops
        rows = torch.cat((raw, torch.zeros(R, 1, device=dev)), dim=1)
        again, _ = ops.surface_shade(rows, got["hit"], got["depth"], finite.clone())
    assert torch.equal(again[some], got["rgb"][some])
    exact = torch.sigmoid(raw.double()) * 1.002 - 0.001
    err = float((got["rgb"].double() - exact)[some].abs().max())
    print(f"render_surface [{codes}]: max |rgb - exact| on hit rows = {err:.3e}")
    assert err <= 1e-6
    assert bool((got["rgb"][~some] == 1.0).all())


def test_refine_zero_and_given_depths(dev, scene, reference):
    """refine = 0 goes straight to the finishing step; ``z`` replaces the sampler's depths."""
    sc, ref = scene, reference["one"]
    _, _, sigma_at = search_sigma(sc, "one")
    ro, rd = sc["ro"].cpu().numpy(), sc["rd"].cpu().numpy()
    z = ref["z"][:, ::3].contiguous()                             # 22 depths
    for refine in (0, 1):
        got = surface(sc, ref["level"], activated=False, refine=refine, z=z, normals=False)
        want = S.render_surface(ro, rd, z.cpu().numpy(), ref["level"], refine, sigma_at)
        assert "normal" not in got and torch.equal(got["z_search"], z)
        assert bits_equal(got["hit"].cpu().numpy(), want["hit"])
        assert bits_equal(got["depth"].cpu().numpy(), want["depth"])
        assert bits_equal(got["bracket"].cpu().numpy(), want["bracket"][:, :2])


def test_a_level_half_the_rays_never_reach(dev, scene, reference):
    """The median of the rays' largest search densities: about half the rays miss without any grid (the level of the
    end-to-end test above is reached by every ray), held against the rule."""
    sc, ref = scene, reference["one"]
    _, _, sigma_at = search_sigma(sc, "one")
    level = float(ref["sigma"].max(dim=1).values.median())
    got = surface(sc, level, activated=False, refine=2)
    want = S.render_surface(sc["ro"].cpu().numpy(), sc["rd"].cpu().numpy(), ref["z"].cpu().numpy(), level, 2, sigma_at)
    hit = got["hit"].cpu().numpy()
    counts = {h: int((hit == h).sum()) for h in (0, 1, 2)}
    print(f"render_surface at the rows' median maximum: level {level:.6f}, hit counts {counts}")
    assert counts[0] > 0 and counts[1] > 0, counts
    assert bits_equal(hit, want["hit"]) and bits_equal(got["depth"].cpu().numpy(), want["depth"])
    assert bits_equal(got["bracket"].cpu().numpy(), want["bracket"][:, :2])
    miss = got["hit"] == 0
    assert bool(torch.isinf(got["depth"][miss]).all()) and bool(torch.isnan(got["point"][miss]).all())
    assert bool((got["rgb"][miss] == 1.0).all()) and bool((got["sigma"][miss] == 0).all())
    assert bool((got["normal"][miss] == 0).all())
    assert bool(torch.isfinite(got["point"][~miss]).all())


# ---------------------------------------------------------------- 3. the activated level


def test_activated_level_is_the_same_crossing(dev, scene, reference):
    sc, ref = scene, reference["one"]
    x = ref["level"] - 1.0
    level = x if x > 20.0 else math.log1p(math.exp(x))            # softplus(level_raw - 1) in float64
    got = surface(sc, level, activated=True, refine=REFINE)
    assert torch.equal(got["hit"], ref["got"]["hit"])
    differ = ~((got["depth"] == ref["got"]["depth"]))
    # a search sample within one fp32 step of the level may fall on the other side of a converted level
    near = ((ref["sigma"] - ref["level"]).abs() <= float(np.spacing(F(abs(ref["level"]))))).any(dim=1)
    print(f"activated level: {int(differ.sum())} rays differ in depth, {int(near.sum())} have a sample within one "
          f"fp32 step of the level")
    assert not bool((differ & ~near).any())
    assert int(differ.sum()) <= R // 100


# ---------------------------------------------------------------- 4. occupancy


def sphere_bits(dev, kind="sphere"):
    bits = OC.grid_bits(kind, 32, bound=1.0, radius=0.45)
    return torch.from_numpy(np.ascontiguousarray(bits.view(np.int32))).to(dev)


def assert_same_result(out, ref, what):
    assert sorted(out) == sorted(ref), what
    for key in ref:
        assert same(out[key], ref[key]), (what, key)


def test_full_grid_is_the_plain_call(dev, scene, reference):
    from codenerf.nerf import OccupancyGrid
    sc, ref = scene, reference["one"]
    full = OccupancyGrid.full(32, 8.0, dev)                       # a cube that holds every sample
    for sync_free in (False, True):
        out = surface(sc, ref["level"], activated=False, refine=REFINE, occupancy=full, sync_free=sync_free)
        assert_same_result(out, ref["got"], sync_free)


def test_sphere_grid_misses_and_forms(dev, scene, reference):
    from codenerf.nerf import OccupancyGrid
    sc, ref = scene, reference["one"]
    grid = OccupancyGrid(sphere_bits(dev), 32, 1.0)
    ro = sc["ro"].clone()
    ro[::2, 0] += 3.0                                             # every other ray passes the sphere by
    bg = (0.2, 0.4, 0.6)
    level = float(ref["sigma"].min()) - 1.0                       # below every density: any kept sample is reached
    out = surface(sc, level, activated=False, refine=3, ro=ro, occupancy=grid, background=bg)
    past = torch.zeros(R, dtype=torch.bool, device=dev)
    past[::2] = True
    assert bool((out["hit"][past] == 0).all()) and bool((out["hit"][~past] != 0).any())
    miss = out["hit"] == 0
    assert bool(torch.isinf(out["depth"][miss]).all()) and bool((out["depth"][miss] > 0).all())
    assert bool(torch.isnan(out["point"][miss]).all())
    assert torch.equal(out["rgb"][miss], torch.tensor(bg, device=dev).expand(int(miss.sum()), 3))
    assert bool(torch.isfinite(out["depth"][~miss]).all()) and bool(torch.isfinite(out["point"][~miss]).all())
    free = surface(sc, level, activated=False, refine=3, ro=ro, occupancy=grid, background=bg, sync_free=True)
    assert_same_result(free, out, "sync_free")
    span = surface(sc, level, activated=False, refine=3, ro=ro, occupancy=grid, background=bg, span_probes=64)
    assert span["ray_span"].shape == (R, 2) and span["ray_hit"].dtype == torch.bool
    assert not bool(span["ray_hit"][past].any()) and bool(span["ray_hit"][~past].any())
    assert bool((span["hit"][past] == 0).all()) and bool((span["hit"][~past] != 0).any())
    assert_same_result(surface(sc, level, activated=False, refine=3, ro=ro, occupancy=grid, background=bg,
                               span_probes=64, sync_free=True), span, "span, sync_free")


# ---------------------------------------------------------------- 5. streams and capture


def test_side_stream(dev, scene, reference):
    """Every ops call of the render lands on the current stream: its log under a side stream (the default stream
    held busy) equals the default-stream log, bit for bit."""
    sc, ref = scene, reference["one"]

    def run():
        surface(sc, ref["level"], activated=False, refine=2)

    run()
    with B.contracts("poison", modules=MODULES, log_returns_of=None), ST.plain() as base:
        run()
    with B.contracts("poison", modules=MODULES, log_returns_of=None), ST.side_stream(wall_ms=base.wall_ms) as side:
        run()
    names = [r[0] for r in base.returns]
    assert "surface_bracket" in names and names.count("surface_step") == 3 and "surface_shade" in names
    assert side.slack_ms and min(side.slack_ms) > 0
    ST.compare_logs(base.returns, side.returns, "the side-stream run")


def test_capture_and_replay_on_new_rays_and_bits(dev, scene, reference):
    """The occupancy + sync_free form captured in a graph; replayed after the rays and the grid's bits were
    overwritten in place it equals the eager, synchronising call on those inputs."""
    from codenerf.nerf import OccupancyGrid
    sc, ref = scene, reference["one"]
    level = float(ref["sigma"].min()) - 1.0
    ro, rd = sc["ro"].clone(), sc["rd"].clone()
    bits = sphere_bits(dev)
    grid = OccupancyGrid(bits, 32, 1.0)
    assert grid.bits.data_ptr() == bits.data_ptr()
    kw = dict(activated=False, refine=2)
    surface(sc, level, ro=ro, rd=rd, occupancy=grid, sync_free=True, **kw)         # the packs are cached from here on
    graph, out = ST.capture(lambda: surface(sc, level, ro=ro, rd=rd, occupancy=grid, sync_free=True, **kw))
    ro0, rd0 = ro.clone(), rd.clone()
    shift = torch.tensor([0.1, 0.05, 0.0], device=dev)
    seen = []
    for name, new_ro, new_rd, kind in (("as captured", ro0, rd0, "sphere"), ("away", ro0, -rd0, "sphere"),
                                       ("moved", ro0 + shift, rd0, "half"), ("moved back", ro0 - shift, rd0, "full")):
        ro.copy_(new_ro)
        rd.copy_(new_rd)
        bits.copy_(sphere_bits(dev, kind))
        for t in out.values():
            B.poison_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = surface(sc, level, ro=ro.clone(), rd=rd.clone(), occupancy=OccupancyGrid(bits.clone(), 32, 1.0), **kw)
        assert_same_result(out, eager, name)
        seen.append(int((eager["hit"] != 0).sum()))
    assert seen[0] > 0 and seen[1] == 0 and seen[3] > seen[0], seen


# ---------------------------------------------------------------- 6. refusals


def test_refusals(dev, scene, reference):
    from codenerf.nerf import OccupancyGrid, render_surface
    sc, ref = scene, reference["one"]
    zs, zt = codes_of(sc, "one")
    args = (sc["ro"], sc["rd"], zs, zt, sc["ps"], sc["emb"], sc["m"])
    level = ref["level"]
    with pytest.raises(ValueError, match="inference"):
        grad = sc["zs"].clone().requires_grad_(True)
        render_surface(sc["ro"], sc["rd"], grad.expand(R, -1), zt, sc["ps"], sc["emb"], sc["m"], level, activated=False)
    with torch.no_grad():
        for precision in ("f16", "bf16x3"):
            other, = models(dev, (0,), precision=precision)
            with pytest.raises(NotImplementedError):
                render_surface(*args[:6], other, level, activated=False)
        for bad in (0.0, -0.5):
            with pytest.raises(ValueError, match="level"):
                render_surface(*args, bad, activated=True)
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="level"):
                render_surface(*args, bad, activated=False)
        for bad in (-1, 25, 6.0, True):
            with pytest.raises(ValueError, match="refine"):
                render_surface(*args, level, activated=False, refine=bad)
        for bad in (torch.zeros(R, device=dev), torch.zeros(R - 1, NS, device=dev), torch.zeros(R, 1, device=dev),
                    torch.zeros(R, 1025, device=dev)):
            with pytest.raises(ValueError, match="z must be"):
                render_surface(*args, level, activated=False, z=bad)
        with pytest.raises(ValueError, match="occupancy"):
            render_surface(*args, level, activated=False, span_probes=64)
        with pytest.raises(ValueError, match="span_probes"):
            render_surface(*args, level, activated=False, span_probes=100,
                           occupancy=OccupancyGrid(sphere_bits(dev), 32, 1.0))
        with pytest.raises(ValueError):
            render_surface(sc["ro"].cpu(), sc["rd"].cpu(), zs.cpu(), zt.cpu(), sc["ps"], sc["emb"], sc["m"], level,
                           activated=False)
