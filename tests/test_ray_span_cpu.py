"""The per-ray depth-span rule (include/codenerf.h, "Per-ray depth spans") as tests/ray_span_cases.py states it
in numpy: its invariants, its edge cases, and what it buys in a ray integral.  No device."""
import numpy as np
import pytest

import occupancy_cases as C
import ray_span_cases as S

F = np.float32


def taus(kind, n_rays, nc, seed=0):
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros((n_rays, nc), dtype=F)
    if kind == "max":
        return np.full((n_rays, nc), S.TAU_MAX, dtype=F)
    return np.random.default_rng(seed).random((n_rays, nc)).astype(F)


@pytest.mark.parametrize("tau", ["none", "zero", "max", "random"])
@pytest.mark.parametrize("nc", [2, 3, 16, 65, 200])
@pytest.mark.parametrize("kind", ["sphere", "half", "full", "empty"])
def test_rows_are_ordered_and_inside_the_span(kind, nc, tau):
    """Rows are non-decreasing, also with tau all 0 and all the largest float below 1; z in [t_lo, t_hi], a
    subset of [near, far]; the last depth is t_hi itself."""
    near, far, p = 0.5, 2.1, 128
    ro, rd = S.camera_rays(67, seed=3)
    z, span, pr = S.sample_span(ro, rd, S.Grid.of(kind), near, far, p, nc, taus(tau, 67, nc))
    assert z.dtype == F and z.shape == (67, nc) and span.dtype == F and pr.dtype == np.int32
    assert np.all(np.diff(z, axis=1) >= 0)
    assert np.all(z >= span[:, :1]) and np.all(z <= span[:, 1:])
    assert np.all(span[:, 0] >= F(near)) and np.all(span[:, 1] <= F(far)) and np.all(span[:, 1] > span[:, 0])
    assert np.array_equal(z[:, -1], span[:, 1])
    if tau in ("none", "zero"):
        assert np.array_equal(z[:, 0], span[:, 0])
    hit = pr[:, 0] >= 0
    assert np.all((pr[:, 0] <= pr[:, 1]) & (pr[:, 1] < p)) and np.all(pr[~hit] == -1)
    if kind == "sphere":
        assert hit.any() and (~hit).any()             # the case has both


def test_full_grid_keeps_the_whole_range():
    """Rays that stay inside the cube of a full grid: every probe is occupied."""
    rng = np.random.default_rng(1)
    ro = rng.uniform(-0.3, 0.3, (9, 3)).astype(F)
    rd = rng.standard_normal((9, 3))
    rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(F)
    near, far, p = 0.0, 0.6, 64
    z, span, pr = S.sample_span(ro, rd, S.Grid.of("full"), near, far, p, 8)
    assert np.all(pr == np.array([0, p - 1])) and np.all(span == np.array([near, far], dtype=F))
    assert np.array_equal(z[:, 0], np.full(9, near, dtype=F)) and np.array_equal(z[:, -1], np.full(9, far, dtype=F))


def test_misses_keep_the_whole_range():
    """The empty grid, NaN directions and rays outside the cube: first = last = -1 and (near, far)."""
    near, far, p, nc = 0.5, 2.1, 64, 5
    ro, rd = S.camera_rays(7, seed=5)
    want = S.span_depths(np.tile(np.array([[near, far]], dtype=F), (7, 1)), nc)
    cases = {"empty": (ro, rd, "empty")}
    nan_rd = rd.copy()
    nan_rd[:, 1] = np.nan
    cases["nan"] = (ro, nan_rd, "full")
    cases["outside"] = (ro + F(5.0), np.abs(rd), "full")
    for name, (o, d, kind) in cases.items():
        z, span, pr = S.sample_span(o, d, S.Grid.of(kind), near, far, p, nc)
        assert np.all(pr == -1), name
        assert np.all(span == np.array([near, far], dtype=F)), name
        assert np.array_equal(z, want), name
    # one NaN ray among hits is a miss of its own
    mixed = rd.copy()
    mixed[2, 0] = np.nan
    _, _, pr = S.sample_span(ro, mixed, S.Grid.of("full"), near, far, p, nc)
    assert np.all(pr[2] == -1) and np.all(np.delete(pr, 2, axis=0)[:, 0] >= 0)


def test_probes_on_cell_faces():
    """occupancy_cases.face_rays, near 0, far 63/16, P = 64: the probes are exactly j / 16, on the cell faces
    and the cube's faces; a face belongs to the cell above it and the cube's far face to nobody."""
    ro, rd, near, far, p = S.face_case()
    assert np.array_equal(S.probe_depths(near, far, p), (np.arange(64) / 16.0).astype(F))
    _, span, pr = S.sample_span(ro, rd, S.Grid.of("full"), near, far, p, 4)
    assert pr[0].tolist() == [0, 31] and pr[1].tolist() == [1, 32]
    assert np.all(pr[0::2] == np.array([0, 31])) and np.all(pr[1::2] == np.array([1, 32]))
    assert span[0].tolist() == [0.0, 2.0] and span[1].tolist() == [0.0, 33.0 / 16.0]
    _, span, pr = S.sample_span(ro, rd, S.Grid.of("half"), near, far, p, 4)
    assert pr[0].tolist() == [0, 15] and pr[1].tolist() == [17, 32]
    assert span[0].tolist() == [0.0, 1.0] and span[1].tolist() == [1.0, 33.0 / 16.0]


@pytest.mark.parametrize("n_objects", [1, 3, 8])
def test_terminating_depth_is_unoccupied(n_objects):
    """For every ray with last < P - 1 the last depth's point -- formed from z's bits as cn_occupancy_cull forms
    it -- is unoccupied for every object, so the last real sample's interval ends at t_hi."""
    _, _, _, grids, ro_k, rd_k = S.scene_case(n_objects, 67, seed=11)
    near, far, p, nc = 0.4, 3.0, 128, 9
    t_rand = taus("random", 67, nc, seed=2)
    z, span, pr = S.sample_span(ro_k, rd_k, grids, near, far, p, nc, t_rand)
    ends_free = (pr[:, 0] >= 0) & (pr[:, 1] < p - 1)
    assert ends_free.sum() >= 10
    for k, grid in enumerate(grids):
        occ = C.lookup(C.ray_points(ro_k[k], rd_k[k], z[:, -1:]), grid.bits, grid.g, grid.bound)[:, 0]
        assert not occ[ends_free].any(), k


def test_two_objects_give_the_union():
    _, _, _, grids, ro_k, rd_k = S.scene_case(3, 67, seed=7)
    near, far, p = 0.4, 3.0, 128
    pick = [0, 1]                                     # a sphere and a half grid, posed apart
    both = S.probe_mask(ro_k[pick], rd_k[pick], [grids[k] for k in pick], near, far, p)
    singles = [S.probe_mask(ro_k[k], rd_k[k], grids[k], near, far, p) for k in pick]
    assert np.array_equal(both, singles[0] | singles[1])
    assert (singles[0] & ~singles[1]).any() and (singles[1] & ~singles[0]).any()
    pr, span = S.span_of_mask(both, near, far)
    pr0, _ = S.span_of_mask(singles[0], near, far)
    pr1, _ = S.span_of_mask(singles[1], near, far)
    hit0, hit1 = pr0[:, 0] >= 0, pr1[:, 0] >= 0
    two = hit0 & hit1
    assert two.any()
    assert np.array_equal(pr[two, 0], np.minimum(pr0[two, 0], pr1[two, 0]))
    assert np.array_equal(pr[two, 1], np.maximum(pr0[two, 1], pr1[two, 1]))
    assert np.array_equal(pr[hit0 & ~hit1], pr0[hit0 & ~hit1]) and np.array_equal(pr[~hit0 & hit1], pr1[~hit0 & hit1])
    assert np.all(pr[~hit0 & ~hit1] == -1)


def test_parallel_image_render_passes_span_probes_through(monkeypatch):
    """parallel_image_render hands ``span_probes`` to render_rays beside ``occupancy``; None by default."""
    import types

    import torch
    from codenerf import nerf as N
    seen = []

    def spy(ro, rd, z_s, z_t, point_sampler, embedders, coarse, fine, chunk_rows=None, **kw):
        seen.append(kw)
        return {"rgb_fine": torch.zeros(ro.shape[0], 3)}

    class Rays:
        def get_bundle(self, tform_cam2world):
            return torch.zeros(1, 2, 3, 3), torch.ones(1, 2, 3, 3)

    monkeypatch.setattr(N, "render_rays", spy)
    cfg = types.SimpleNamespace(nerf=types.SimpleNamespace(validation=types.SimpleNamespace(chunksize=4)))
    models = {"nerf_coarse": torch.nn.Identity(), "nerf_fine": torch.nn.Identity()}
    codes = [torch.zeros(1, 4), torch.zeros(1, 4)]
    grid = object()
    for kw, want in ((dict(occupancy=grid, span_probes=128), 128), (dict(occupancy=grid), None), ({}, None)):
        rgb = N.parallel_image_render(cfg, torch.eye(4)[None], codes, models, (Rays(), None), (None, None), "cpu", **kw)
        assert rgb.shape == (6, 3)
        assert seen[-1]["span_probes"] == want and seen[-1]["occupancy"] is kw.get("occupancy")


# ---------------------------------------------------------------- what the spans buy in a ray integral


def acc_f64(occ, z):
    """1 - exp(-sum sigma_i delta_i) in float64: density 6 where occupied, volume_render's intervals (to the next
    depth, 1e10 after the last; the rays are unit length)."""
    z = z.astype(np.float64)
    delta = np.concatenate([np.diff(z, axis=1), np.full((z.shape[0], 1), 1e10)], axis=1)
    return 1.0 - np.exp(-(6.0 * occ * delta).sum(axis=1))


@pytest.fixture(scope="module")
def quadrature():
    """The G = 32 sphere of radius 0.5, a 24 x 24 pinhole camera at distance 1.3, near 0.5, far 2.1, P = 256,
    homogeneous density 6 inside the grid's cells; the truth is a 4096-sample quadrature."""
    grid = S.Grid.of("sphere", 32, radius=0.5)
    ro, rd = S.pinhole_rays(24, 1.3)
    near, far, p = 0.5, 2.1, 256

    def occupied(z):
        return C.lookup(C.ray_points(ro, rd, z), grid.bits, grid.g, grid.bound)

    dense = np.tile(np.linspace(near, far, 4096).astype(F)[None, :], (ro.shape[0], 1))
    dense_occ = occupied(dense)
    pr, span = S.span_of_mask(S.probe_mask(ro, rd, grid, near, far, p), near, far)
    return dict(ro=ro, near=near, far=far, occupied=occupied, dense=dense, dense_occ=dense_occ,
                truth=acc_f64(dense_occ, dense), pr=pr, span=span)


@pytest.mark.parametrize("nc", [16, 32])
def test_span_depths_halve_the_quadrature_error(quadrature, nc):
    """Mean |acc error| over the rays that hit, same Nc, same quadrature: the span depths' is below half the
    plain depths' (the prototype had 0.20 of it at Nc = 16 and 0.18 at 32)."""
    q = quadrature
    hit = q["pr"][:, 0] >= 0
    assert hit.sum() > 200 and (~hit).any()
    plain = np.tile(np.linspace(q["near"], q["far"], nc).astype(F)[None, :], (q["ro"].shape[0], 1))
    spans = S.span_depths(q["span"], nc)
    err_plain = np.abs(acc_f64(q["occupied"](plain), plain) - q["truth"])[hit].mean()
    err_span = np.abs(acc_f64(q["occupied"](spans), spans) - q["truth"])[hit].mean()
    print(f"Nc {nc}: {int(hit.sum())} hit rays, mean |acc error| plain {err_plain:.4g} span {err_span:.4g} "
          f"ratio {err_span / err_plain:.3f}")
    assert err_span < 0.5 * err_plain


def test_spans_hold_the_occupied_samples(quadrature):
    """Fewer than 0.1 % of the occupied dense samples lie outside their ray's span (the rule is not strictly
    conservative: a corner clip shorter than a probe step; the prototype had 0.0012 %), and no terminating
    sample is occupied."""
    q = quadrature
    outside = q["dense_occ"] & ((q["dense"] < q["span"][:, :1]) | (q["dense"] > q["span"][:, 1:]))
    n_occ = int(q["dense_occ"].sum())
    print(f"{int(outside.sum())} of {n_occ} occupied dense samples outside their span")
    assert n_occ > 100000 and outside.sum() < 1e-3 * n_occ
    assert not q["occupied"](q["span"][:, 1:])[:, 0].any()
