"""The iso-surface ray casting rule of tests/surface_cases.py on analytic fields: no GPU."""
import numpy as np
import pytest

import surface_cases as S

F = np.float32


def cubic_field(k=2.0):
    """sigma(p) = k (p_z + 0.2)^3: monotone along rays of direction +z, root of ``level`` known in closed form."""
    def sigma_at(pts):
        return (F(k) * (pts[..., 2] + F(0.2)) ** 3).astype(F)
    return sigma_at


def z_rays(r):
    ro = np.zeros((r, 3), dtype=F)
    ro[:, 0] = np.linspace(-0.5, 0.5, r)
    ro[:, 2] = -1.0
    rd = np.zeros((r, 3), dtype=F)
    rd[:, 2] = 1.0
    return ro, rd


def depths(r, s, near=0.25, far=2.25):
    return np.tile(np.linspace(near, far, s, dtype=F), (r, 1))


@pytest.mark.parametrize("s", [8, 64])
def test_monotone_ramp_converges_to_the_root(s):
    ro, rd = z_rays(7)
    z = depths(7, s)
    level = 0.3
    root = 1.0 - 0.2 + (level / 2.0) ** (1.0 / 3.0)          # p_z = -1 + t
    spacing = float(z[0, 1] - z[0, 0])
    errs = []
    for refine in (0, 1, 3, 6, 12, 24):
        out = S.render_surface(ro, rd, z, level, refine, cubic_field())
        assert np.all(out["hit"] == 1)
        err = float(np.abs(out["depth"].astype(np.float64) - root).max())
        # the root lies in the bracket, the interpolated depth too: the error is at most the bracket's width
        assert err <= spacing / 2 ** refine + 1e-6, (refine, err)
        errs.append(err)
    assert errs[-1] <= 1e-6 and errs[3] < errs[0] / 50
    # the point is the ray at that depth
    assert np.array_equal(out["point"], (ro + rd * out["depth"][:, None]).astype(F))


def test_bracket_never_widens_and_holds_the_depth():
    rng = np.random.default_rng(3)
    ro, rd = S.rays(40, seed=1)
    z = np.sort(rng.random((40, 16)).astype(F) * F(2.0) + F(0.3), axis=1)

    def sigma_at(pts):                       # a bumpy field: several crossings per ray
        return (np.sin(F(9.0) * pts[..., 2]) + F(0.5) * pts[..., 0]).astype(F)

    trace = []
    out = S.render_surface(ro, rd, z, 0.1, 10, sigma_at, trace=trace)
    assert set(out["hit"].tolist()) >= {1} and len(trace) == 11
    for (b0, _), (b1, _) in zip(trace, trace[1:]):
        assert np.all(b1[:, 0] >= b0[:, 0]) and np.all(b1[:, 1] <= b0[:, 1])
    for b, t in trace:
        assert np.all(b[:, 0] <= t) and np.all(t <= b[:, 1])
    live = out["hit"] == 1
    b = out["bracket"]
    assert np.all(b[live, 2] < F(0.1)) and np.all(b[live, 3] >= F(0.1))
    still = out["hit"] != 1                  # hit 0 and 2: the bracket is one depth and never moves
    assert np.array_equal(trace[0][0][still], trace[-1][0][still])
    assert np.all(b[still, 0] == b[still, 1])


def test_refine_zero_is_the_search_samples_interpolation():
    ro, rd = z_rays(5)
    z = depths(5, 8)
    sigma_at = cubic_field()
    out = S.render_surface(ro, rd, z, 0.3, 0, sigma_at)
    sig = sigma_at(S.ray_points(ro, rd, z))
    j = (sig >= F(0.3)).argmax(axis=1)
    rows = np.arange(5)
    s_lo, s_hi, t_lo, t_hi = sig[rows, j - 1], sig[rows, j], z[rows, j - 1], z[rows, j]
    w = ((F(0.3) - s_lo) / (s_hi - s_lo)).astype(F)
    assert np.array_equal(out["depth"], (t_lo + w * (t_hi - t_lo)).astype(F))
    assert np.array_equal(out["bracket"], np.stack([t_lo, t_hi, s_lo, s_hi], axis=1))


def test_classes_give_the_stated_brackets():
    for s in (2, 3, 63, 64, 65, 200):
        sigma, z, kinds, want = S.class_case(len(S.CLASSES), s, seed=s)
        assert sorted(kinds) == sorted(S.CLASSES)
        b, hit = S.bracket(sigma, z, 0.25)
        for r, (h, j) in enumerate(want):
            lo, hi = (s - 1, s - 1) if h == 0 else (max(j - 1, 0), j)
            assert hit[r] == h, (s, kinds[r])
            got, exp = b[r], np.array([z[r, lo], z[r, hi], sigma[r, lo], sigma[r, hi]], dtype=F)
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (s, kinds[r])


def one(t_lo, t_hi, s_lo, s_hi, hit=1, level=0.25, **kw):
    ro, rd = np.zeros((1, 3), dtype=F), np.ones((1, 3), dtype=F)
    b, t, pts = S.step(ro, rd, np.array([hit], dtype=np.int32), np.array([[t_lo, t_hi, s_lo, s_hi]], dtype=F),
                       level, **kw)
    assert np.array_equal(pts[0], np.full(3, t[0], dtype=F), equal_nan=True)
    return b[0], t[0]


def test_step_cases():
    # the midpoint, and the plain interpolation
    assert one(1.0, 2.0, 0.0, 1.0)[1] == F(1.5)
    assert one(1.0, 2.0, 0.0, 1.0, finish=True)[1] == F(1.25)
    # a tie at the high end interpolates to it; a tie cannot be the low end (it would have been reached)
    assert one(1.0, 2.0, 0.0, 0.25, finish=True)[1] == F(2.0)
    # an unknown low end (marker, NaN, -inf): the high end's depth
    for s_lo in (S.EMPTY, S.NAN, -S.INF):
        assert one(1.0, 2.0, s_lo, 1.0, finish=True)[1] == F(2.0)
    # a flat or falling bracket: the high end's depth
    assert one(1.0, 2.0, 0.5, 0.5, finish=True)[1] == F(2.0)
    assert one(1.0, 2.0, 0.5, 0.4, finish=True)[1] == F(2.0)
    # an infinite high end: the quotient is 0, the low end's depth
    assert one(1.0, 2.0, 0.0, S.INF, finish=True)[1] == F(1.0)
    # hit 0 and 2 have one depth, whatever the densities (+inf - +inf is NaN: the quotient becomes 0)
    for s in (0.1, 3.0, S.INF, S.NAN, S.EMPTY):
        for hit in (0, 2):
            for finish in (False, True):
                assert one(1.5, 1.5, s, s, hit=hit, finish=finish)[1] == F(1.5)
    # the update: a probe at or above the level replaces the high end, one below it or NaN the low end
    t = np.array([1.5], dtype=F)
    for probe, want in ((0.25, [1.0, 1.5, 0.0, 0.25]), (0.9, [1.0, 1.5, 0.0, 0.9]), (0.2, [1.5, 2.0, 0.2, 1.0]),
                        (np.nan, [1.5, 2.0, np.nan, 1.0]), (-1.0e4, [1.5, 2.0, -1.0e4, 1.0])):
        b, t_new = one(1.0, 2.0, 0.0, 1.0, t=t, probe=np.array([probe], dtype=F))
        assert np.array_equal(b, np.array(want, dtype=F), equal_nan=True), probe
        assert t_new == F(0.5) * (b[0] + b[1])
    # hit 0 and 2 ignore the probe
    for hit in (0, 2):
        b, t_new = one(1.5, 1.5, 0.0, 0.0, hit=hit, t=t, probe=np.array([9.0], dtype=F))
        assert np.array_equal(b, np.array([1.5, 1.5, 0.0, 0.0], dtype=F)) and t_new == F(1.5)


def test_shade_rule():
    raw = np.array([[0.0, 1.0, -1.0, 5.0]] * 3, dtype=F)
    pts = np.arange(9, dtype=F).reshape(3, 3)
    rgb, depth, out = S.shade(raw, np.array([0, 1, 2]), np.array([1.0, 2.0, 3.0], dtype=F), pts, (0.1, 0.2, 0.3))
    assert np.array_equal(rgb[0], np.array([0.1, 0.2, 0.3], dtype=F).astype(np.float64))
    assert abs(rgb[1, 0] - 0.5) < 1e-12 and np.array_equal(rgb[1], rgb[2])
    assert depth.tolist() == [np.inf, 2.0, 3.0]
    assert np.isnan(out[0]).all() and np.array_equal(out[1:], pts[1:])
