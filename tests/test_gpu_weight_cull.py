"""Weight-bounded colour culling on the device: cn_weight_cull / cn_scatter_rgb against the numpy model
(tests/weight_cull_cases.py), and render_rays / parallel_image_render with ``rgb_tolerance=``.

Every comparison is exact unless it says otherwise: the ops-level weights are multiples of 2^-30 (any
order of the tail's double additions is exact), the render tests first assert that no tail of the
device's own weights lies within 1e-9 relative of eps_tail, and a kept sample goes through the same
field arithmetic wherever it sits in the launch (test_gpu_occupancy.test_field_over_compact_list).
"""
import numpy as np
import pytest
import torch

import occupancy_cases as OC
import weight_cull_cases as WC
from test_gpu_occupancy import FD, FX, T, _image_rays, _same, dev_bits, empty_row
from test_gpu_parity import dev, embedders, load, models  # noqa: F401

pytestmark = pytest.mark.gpu

SCAN_PART = 4096     # rays per partition of the cull's offset scan (kScanPart, occupancy.hip)
TOL = 1e-3
SAMPLERS = [(64, 64), (32, 128)]
CHUNK = 400


# ---------------------------------------------------------------- cull


def _check_cull(dev, w, ro, rd, z, chunk_rows, code_index, eps_weight=WC.EPS_WEIGHT, eps_tail=WC.EPS_TAIL):
    """ops.weight_cull against the model, every output exact -> (model dict, the op's outputs)."""
    from codenerf import ops
    want = WC.cull(w, ro, rd, z, chunk_rows, code_index, eps_weight, eps_tail)
    tw, tro, trd, tz = T(w, dev), T(ro, dev), T(rd, dev), T(z, dev)
    ci = None if code_index is None else T(code_index, dev)
    got = ops.weight_cull(tw, tro, trd, tz, chunk_rows, float(eps_weight), eps_tail, code_index=ci)
    count, sidx, pts, vdir, code, state = got
    assert isinstance(count, int) and count == want["count"]
    assert sidx.dtype == torch.int32 and code.dtype == torch.int64
    assert sidx.shape == (count,) and pts.shape == (count, 3) and vdir.shape == (count, 3) and code.shape == (count,)
    assert torch.equal(sidx, T(want["sample_index"], dev))
    all_pts = ops.ray_points(tro, trd, tz).reshape(-1, 3)
    assert torch.equal(pts.view(torch.int32), all_pts[sidx.long()].view(torch.int32))
    assert torch.equal(pts.view(torch.int32), T(want["pts"], dev).view(torch.int32))
    assert torch.equal(vdir.view(torch.int32), T(want["vdir"], dev).view(torch.int32))
    assert torch.equal(code, T(want["code_out"], dev))
    return want, got


@pytest.mark.parametrize("r,s", [(1, 1), (37, 64), (50, 3), (3, 65), (9, 192), (5, 512), (4100, 2)])
def test_weight_cull_matches_model(dev, r, s):
    """Dyadic weight rows with the special rows (all zero, all kept, NaN, ties at both thresholds) where
    the shape has room; one chunk, a ragged last chunk, per-ray chunks; with and without code_index.
    (3, 65): one sample in the second word; (4100, 2): across the scan's 4096-ray partition."""
    from codenerf import ops
    w = WC.dyadic_weights(r, s, seed=r + s)
    ro, rd, z = OC.random_rays(r, s, seed=r * s)
    index = np.random.default_rng(r).integers(0, 3, size=r)
    keep = WC.keep_mask(w, WC.EPS_WEIGHT, WC.EPS_TAIL)
    if r >= 5:
        assert not keep[0].any() and np.isnan(w[2]).any() and keep[3, 0] and keep[3, -1] and not keep[4].any()
        assert keep[1].all() or s > 128
    if r > 8:
        assert 0 < keep[5:].sum() < keep[5:].size
    if r > SCAN_PART:
        assert keep[:SCAN_PART].any() and keep[SCAN_PART:].any()
    for chunk_rows in sorted({r, 16, 1}):          # one chunk; a ragged last chunk (r > 16, r % 16 != 0); per-ray
        assert chunk_rows != 16 or r < 16 or r % 16
        for code_index in (None, index):
            want, got = _check_cull(dev, w, ro, rd, z, chunk_rows, code_index)
    # the state it leaves is cn_occupancy_expand's: kept rows bit-equal, the others the empty row
    count, sidx, _, _, _, state = got
    compact = torch.randn(count, 4, generator=torch.Generator().manual_seed(r)).to(dev)
    compact[::3, 3] = float("nan")
    raw = ops.occupancy_expand(compact if count else None, state)
    expect = empty_row(dev).repeat(r * s, 1)
    expect[sidx.long()] = compact
    assert torch.equal(raw.view(-1, 4).view(torch.int32), expect.view(torch.int32))
    tkeep = T(want["keep"], dev)
    assert torch.equal(raw[~tkeep], empty_row(dev).repeat(int((~tkeep).sum()), 1))


def test_weight_cull_zero_thresholds(dev):
    """eps 0 / 0 keeps exactly the samples of weight > 0 that have no NaN at or after them."""
    w = WC.dyadic_weights(37, 64, seed=5)
    ro, rd, z = OC.random_rays(37, 64, seed=5)
    want, _ = _check_cull(dev, w, ro, rd, z, 16, None, eps_weight=np.float32(0), eps_tail=0.0)
    expect = w > 0
    expect[2, :33] = False                      # the NaN of row 2 sits at sample 32
    assert np.array_equal(want["keep"], expect)


def test_weight_cull_without_code_output_and_refusals(dev):
    from codenerf import ops
    w = WC.dyadic_weights(20, 7, seed=1)
    ro, rd, z = OC.random_rays(20, 7, seed=1)
    args = (T(w, dev), T(ro, dev), T(rd, dev), T(z, dev), 20)
    out = ops.weight_cull(*args, float(WC.EPS_WEIGHT), WC.EPS_TAIL, want_code=False)
    assert out[4] is None and out[0] == int(WC.keep_mask(w, WC.EPS_WEIGHT, WC.EPS_TAIL).sum()) > 0
    for ew, et in ((-1.0, 0.0), (0.0, -1.0), (float("nan"), 0.0), (0.0, float("nan"))):
        with pytest.raises(ValueError):
            ops.weight_cull(*args, ew, et)
    with pytest.raises(AssertionError):
        ops.weight_cull(T(w[:, :-1], dev), *args[1:], 0.0, 0.0)


# ---------------------------------------------------------------- scatter

SENTINEL = 0x7FC0BEEF      # a NaN with a payload, as int32


@pytest.mark.parametrize("n_slots,n_rows", [(1, 1), (7, 3), (300, 300), (1000, 257), (64 * 130, 4097)])
def test_scatter_rgb(dev, n_slots, n_rows):
    """Only components 0..2 of the indexed rows change, to the compact rows' bits."""
    from codenerf import ops
    g = torch.Generator().manual_seed(n_slots)
    idx = torch.randperm(n_slots, generator=g)[:n_rows].sort().values.to(torch.int32)
    compact = torch.randn(n_rows, 4, generator=g)
    compact[::5, 1] = float("nan")
    compact[1::7, 0] = -0.0
    raw = torch.full((n_slots, 4), SENTINEL, dtype=torch.int32).view(torch.float32).to(dev)
    expect = raw.view(torch.int32).clone()
    expect[idx.long().to(dev), :3] = compact.to(dev).view(torch.int32)[:, :3]
    out = ops.scatter_rgb(compact.to(dev), idx.to(dev), raw)
    assert out is raw
    assert torch.equal(raw.view(torch.int32), expect)
    assert int((raw.view(torch.int32)[:, 3] != SENTINEL).sum()) == 0
    assert int((raw.view(torch.int32)[:, :3] != SENTINEL).any(dim=1).sum()) == n_rows


def test_scatter_rgb_shapes_and_nothing_kept(dev):
    from codenerf import ops
    raw = torch.full((5, 8, 4), SENTINEL, dtype=torch.int32).view(torch.float32).to(dev)
    before = raw.view(torch.int32).clone()
    none = torch.empty(0, dtype=torch.int32, device=dev)
    assert ops.scatter_rgb(torch.empty(0, 4, device=dev), none, raw) is raw      # no row kept: no launch
    assert ops.scatter_rgb(None, none, raw) is raw
    assert torch.equal(raw.view(torch.int32), before)
    idx = torch.tensor([0, 9, 39], dtype=torch.int32, device=dev)                # an (R, S, 4) destination
    rows = torch.arange(12.0, device=dev).view(3, 4)
    ops.scatter_rgb(rows, idx, raw)
    assert torch.equal(raw.view(-1, 4)[idx.long(), :3], rows[:, :3])
    before.view(-1, 4)[idx.long(), :3] = rows.view(torch.int32)[:, :3]
    assert torch.equal(raw.view(torch.int32), before)
    with pytest.raises(AssertionError):
        ops.scatter_rgb(rows[:2], idx, raw)                                      # wrong row count
    with pytest.raises(AssertionError):
        ops.scatter_rgb(rows, idx, raw[..., :3])                                 # not (.., 4) rows


# ---------------------------------------------------------------- render


@pytest.fixture(scope="module")
def scene(dev):
    """32 x 32 rays of the render_small.npz pose; the synthetic coarse model (seed 0), the fine model
    (seed 1: every weight > 0) and a private copy of it with fc_out.bias[0] -- sigma_raw's bias -- raised
    by 60, so that the transmittance dies inside the volume."""
    g = load("render_small.npz", dev)
    rs, ro, rd = _image_rays(dev, g, 32, 32)
    n = ro.shape[0]
    mc, mf = models(dev)
    dense, = models(dev, (1,))
    with torch.no_grad():
        dense.fc_out.bias[0] += 60.0
    return dict(g=g, rs=rs, ro=ro, rd=rd, n=n, mc=mc, mf=mf, dense=dense, zs=g["z_s"].expand(n, -1),
                zt=g["z_t"].expand(n, -1))


def _render(sc, dev, ps, fine, **kw):
    from codenerf.nerf import render_rays
    with torch.no_grad():
        return render_rays(sc["ro"], sc["rd"], sc["zs"], sc["zt"], ps, embedders(dev), sc["mc"], fine,
                           chunk_rows=CHUNK, **kw)


def _sampler(dev, nc, nf):
    from codenerf.nerf import PointSampler
    return PointSampler(nc, nf, 0.8, 1.8, "lindepth", False, torch.float32, dev)


@pytest.mark.parametrize("coarse_rgb", [True, False])
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("nc,nf", SAMPLERS)
def test_render_zero_tolerance_bitwise(dev, scene, nc, nf, fold, coarse_rgb):
    """rgb_tolerance=0.0 culls only weights of 0, of which the seed-1 fine model has none: every entry
    is the plain call's, bit for bit -- the density kernel's sigma and the scattered colours included."""
    sc, ps = scene, _sampler(dev, nc, nf)
    before = sc["mc"].fold, sc["mf"].fold
    try:
        sc["mc"].fold = sc["mf"].fold = fold
        ref = _render(sc, dev, ps, sc["mf"], coarse_rgb=coarse_rgb)
        out = _render(sc, dev, ps, sc["mf"], coarse_rgb=coarse_rgb, rgb_tolerance=0.0)
    finally:
        sc["mc"].fold, sc["mf"].fold = before
    assert sorted(out) == sorted(ref) and ("rgb_coarse" in out) == coarse_rgb
    for k in ref:
        assert torch.equal(out[k], ref[k]), k


def _compose(sc, dev, z_f, grid_bits=None, bound=1.0):
    """What the two-phase fine pass must give, from the UNCULLED field: the full field rows (under a grid:
    torch.where with the empty row), the device's own fine weights from them, the model's mask on
    those weights, zero colours where it culls, and the existing volume_render.
    -> (rgb, weights numpy, keep numpy, (eps_weight, eps_tail))."""
    from codenerf import ops
    from codenerf.models.model import _field_op
    ro, rd = sc["ro"], sc["rd"]
    raw = _field_op(sc["dense"], sc["g"]["z_s"], sc["g"]["z_t"], rd, CHUNK, FX, FD, ro=ro, z=z_f)
    if grid_bits is not None:
        in_grid = OC.lookup(OC.ray_points(ro.cpu().numpy(), rd.cpu().numpy(), z_f.cpu().numpy()), grid_bits, 32, bound)
        raw = torch.where(T(in_grid, dev)[..., None], raw, empty_row(dev))
    w = ops.volume_render(raw, z_f, rd)[3].cpu().numpy()
    eps = WC.thresholds(TOL, z_f.shape[1])
    keep = WC.keep_mask(w, *eps)
    raw_c = raw.clone()
    raw_c[..., :3] = torch.where(T(keep, dev)[..., None], raw[..., :3], torch.zeros((), device=dev))
    return ops.volume_render(raw_c, z_f, rd)[0], w, keep, eps


def _check_against_plain(out, plain, rgb_expect, w, keep, s):
    assert sorted(out) == sorted(plain)
    for k in plain:
        if k != "rgb_fine":
            assert _same(out[k], plain[k], equal_nan=k.startswith(("disp", "depth"))), k
    assert torch.equal(out["rgb_fine"], rgb_expect)
    dropped = WC.dropped_weight(w, keep)
    assert dropped.max() <= TOL
    err = (out["rgb_fine"].double() - plain["rgb_fine"].double()).abs().max(dim=-1).values.cpu().numpy()
    bound = 0.501 * dropped + 2 * s * 2.0 ** -24
    print(f"max dropped {dropped.max():.3e}  max |d rgb| {err.max():.3e}  min slack {(bound - err).min():.3e}")
    assert (err <= bound).all()
    return dropped, err


@pytest.mark.parametrize("coarse_rgb", [True, False])
@pytest.mark.parametrize("nc,nf", SAMPLERS)
def test_render_tolerance_composed(dev, scene, nc, nf, coarse_rgb):
    """tol = 1e-3 on the dense fine model: everything but rgb_fine is the plain render's bits, rgb_fine is
    the composition from the unculled field, and per ray it is within 0.501 x dropped + 2 S 2^-24 of
    the plain render's, dropped <= tol."""
    sc, ps = scene, _sampler(dev, nc, nf)
    plain = _render(sc, dev, ps, sc["dense"], coarse_rgb=coarse_rgb)
    events = {}
    out = _render(sc, dev, ps, sc["dense"], coarse_rgb=coarse_rgb, rgb_tolerance=TOL, events=events)
    assert len(events["field"]) == 2                # the two-phase fine call is one timed field call
    with torch.no_grad():
        rgb_expect, w, keep, (_, eps_tail) = _compose(sc, dev, out["z_fine"])
    # preconditions: the scene does cull, part of every ray, and no tail is near the threshold
    kept = keep.mean()
    print(f"kept {kept:.4f}")
    assert 0.1 < kept < 0.8
    assert WC.band_count(w, eps_tail) == 0
    per_ray = keep.sum(axis=-1)
    assert per_ray.min() > 0 and per_ray.max() < nc + nf
    dropped, err = _check_against_plain(out, plain, rgb_expect, w, keep, nc + nf)
    assert dropped.max() > 0.25 * TOL and err.max() > 0          # the culling shows in the colours


@pytest.mark.parametrize("nc,nf", SAMPLERS)
def test_render_tolerance_with_grid(dev, scene, nc, nf):
    """With a sphere grid as well: against the grid-culled plain render, composed in the same way from
    the grid-culled rows (whose empty rows have weight 0 and fall out by w > 0)."""
    from codenerf.nerf import OccupancyGrid
    sc, ps = scene, _sampler(dev, nc, nf)
    bits = OC.grid_bits("sphere", 32, bound=1.0, radius=0.45)
    grid = OccupancyGrid(dev_bits(bits, dev), 32, 1.0)
    plain = _render(sc, dev, ps, sc["dense"], coarse_rgb=False, occupancy=grid)
    out = _render(sc, dev, ps, sc["dense"], coarse_rgb=False, occupancy=grid, rgb_tolerance=TOL)
    with torch.no_grad():
        rgb_expect, w, keep, (_, eps_tail) = _compose(sc, dev, out["z_fine"], grid_bits=bits)
        in_grid = OC.lookup(OC.ray_points(sc["ro"].cpu().numpy(), sc["rd"].cpu().numpy(),
                                          out["z_fine"].cpu().numpy()), bits, 32, 1.0)
    print(f"kept {keep.mean():.4f} of all, {keep.sum() / in_grid.sum():.4f} of the grid's")
    assert WC.band_count(w, eps_tail) == 0
    assert not (keep & ~in_grid).any() and 0 < keep.sum() < in_grid.sum()        # both cull
    assert (w[~in_grid] == 0).all()
    _check_against_plain(out, plain, rgb_expect, w, keep, nc + nf)


def test_parallel_image_render_tolerance(dev, scene):
    from types import SimpleNamespace as NS
    from codenerf.nerf import parallel_image_render
    sc, ps = scene, _sampler(dev, 32, 128)
    cfg = NS(is_distributed=False, gpus=1, nerf=NS(validation=NS(chunksize=CHUNK)))
    mdls = {"nerf_coarse": sc["mc"], "nerf_fine": sc["dense"]}
    args = (cfg, sc["g"]["pose"], [sc["g"]["z_s"], sc["g"]["z_t"]], mdls, (sc["rs"], ps), embedders(dev), dev)
    for coarse_rgb in (True, False):
        img = parallel_image_render(*args, coarse_rgb=coarse_rgb, rgb_tolerance=TOL)
        ref = _render(sc, dev, ps, sc["dense"], coarse_rgb=coarse_rgb, rgb_tolerance=TOL)
        assert torch.equal(img, ref["rgb_fine"])
    plain = parallel_image_render(*args)
    assert plain.shape == img.shape and not torch.equal(plain, img)      # the tolerance did cull
    assert (plain - img).abs().max().item() <= 0.501 * TOL + 2 * 160 * 2.0 ** -24


def test_render_tolerance_refusals(dev, scene):
    from codenerf.nerf import render_rays
    sc = scene
    n = 64
    ps = _sampler(dev, 8, 8)
    mc, mf = models(dev)
    for m in (mc, mf):
        m.requires_grad_(False)
    zs = sc["g"]["z_s"].clone().requires_grad_(True)
    args = (sc["ro"][:n], sc["rd"][:n], zs.expand(n, -1), sc["g"]["z_t"].expand(n, -1), ps, embedders(dev), mc, mf)
    with pytest.raises(ValueError, match="rgb_tolerance"):          # a code that requires grad, grad mode on
        render_rays(*args, chunk_rows=50, rgb_tolerance=TOL)
    mc.requires_grad_(True)
    with pytest.raises(ValueError, match="rgb_tolerance"):          # trainable parameters, grad mode on
        render_rays(sc["ro"][:n], sc["rd"][:n], sc["zs"][:n], sc["zt"][:n], ps, embedders(dev), mc, mf, chunk_rows=50,
                    rgb_tolerance=TOL)
    with torch.no_grad():
        for bad in (-1e-3, float("nan"), -0.5):
            with pytest.raises(ValueError, match="rgb_tolerance"):
                render_rays(*args, chunk_rows=50, rgb_tolerance=bad)
        with pytest.raises(ValueError, match="rgb_tolerance"):
            render_rays(*args, chunk_rows=50, coarse_only=True, rgb_tolerance=TOL)
        out = render_rays(*args, chunk_rows=50, rgb_tolerance=TOL)       # the same inputs with grad mode off render
        ref = render_rays(*args, chunk_rows=50)
    assert sorted(out) == sorted(ref)
    assert (out["rgb_fine"] - ref["rgb_fine"]).abs().max().item() <= 0.501 * TOL + 2 * 16 * 2.0 ** -24
    for k in ("depth_fine", "acc_fine", "weights_coarse", "rgb_coarse", "z_fine"):
        assert torch.equal(out[k], ref[k]), k
