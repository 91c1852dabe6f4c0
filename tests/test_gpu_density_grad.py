"""The density-gradient kernel (cn_density_gradient) and what is built on it: ops.density_gradient,
nerf.density_gradient / nerf.normals, extract_mesh's vertex normals and colours, render_rays' normal map.

The kernel runs the density kernel's forward and the tail of the fused backward with the same
instructions in the same order, so its sigma is compared with ``torch.equal`` against ops.density_field
and its gradient value for value (``==``, NaNs in the same places) against the composed path --
ops.radiance_field_masks, then ops.field_backward_x3(precision="f32") on d_raw = (0, 0, 0, 1) -- which
adds only exact zeros to the same chain.  Independent of both it is held against the float64 statement
of tests/density_grad_cases.py.
"""
import pytest
import torch

import buffers
import density_grad_cases as C
from conftest import margin
from exact_cases import persistent_rows, probe_model
from test_gpu_parity import dev, embedders, models  # noqa: F401

pytestmark = pytest.mark.gpu

FX = [2.0 ** k for k in range(10)]
FD = [2.0 ** k for k in range(4)]


class Field:
    """A parameter set on the device with its two packs and code terms (shared, read-only)."""

    def __init__(self, dev, state, z_s):
        from codenerf import ops
        self.params = [v.to(dev) for v in state.values()]
        self.packed = ops.mlp_pack(self.params, "f32_w16")
        self.packed_t = ops.mlp_pack(self.params, "f32_w16_t")
        self.z_s = z_s.to(dev)
        self.cb = ops.code_bias(self.params, self.z_s, torch.zeros_like(self.z_s))

    def row(self, k):
        return self.cb[k:k + 1].contiguous()


@pytest.fixture(scope="module")
def field(dev):
    """The coarse synthetic model with three code rows."""
    from codenerf import synthetic
    return Field(dev, synthetic.codenerf_params(0), synthetic.latent_codes(3, 3))


def composed(f, cb, pts):
    """The composed path on points (R, S, 3) with one code row -> (d_pts (R, S, 3), sigma_raw (R, S))."""
    from codenerf import ops
    r, s = pts.shape[:2]
    rd = torch.zeros(r, 3, device=pts.device)
    rd[:, 2] = 1.0
    raw, masks = ops.radiance_field_masks(f.packed, cb, rd, s, r, FX, FD, pts=pts, precision="f32")
    d_raw = torch.zeros(r, s, 4, device=pts.device)
    d_raw[..., 3] = 1.0
    out = ops.field_backward_x3(f.packed_t, masks, d_raw, r, s, r, 1, FX, FD, rd, pts=pts, want_pts=True,
                                precision="f32")
    return out["d_pts"], raw[..., 3]


def same_values(a, b):
    """Elementwise equal as values, NaNs in the same places."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def same_bits(a, b):
    """torch.equal on the bits of two float32 tensors: a NaN included, and -0 apart from +0."""
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _points(m, seed, scale=1.0):
    return torch.randn(m, 3, generator=torch.Generator().manual_seed(seed)) * scale


def _rays(dev, r, s, seed):
    g = torch.Generator().manual_seed(seed)
    ro = torch.randn(r, 3, generator=g) * 0.3
    rd = torch.randn(r, 3, generator=g)
    z = torch.sort(0.8 + torch.rand(r, s, generator=g), dim=-1).values
    return ro.to(dev), rd.to(dev), z.to(dev)


# ---------------------------------------------------------------- a, b: the bits of both halves


def _check_points(f, pts):
    """Columns 0..2 against the composed path, column 3 against the density kernel, on (M, 3) points."""
    from codenerf import ops
    cb = f.row(0)
    out = ops.density_gradient(f.packed, f.packed_t, cb, FX, pts=pts)
    assert out.shape == (pts.shape[0], 4)
    assert same_bits(out[:, 3], ops.density_field(f.packed, cb, FX, pts=pts))
    d_pts, sigma = composed(f, cb, pts.view(-1, 1, 3))
    assert same_bits(out[:, 3], sigma.view(-1))
    assert same_values(out[:, :3], d_pts.view(-1, 3))
    return out


@pytest.mark.parametrize("m", [1, 127, 128, 129])
def test_gradient_and_sigma_bits_small(dev, field, m):
    """One (partly clamped) tile, a full one, and one row into a second workgroup."""
    out = _check_points(field, _points(m, m).to(dev))
    assert bool(torch.isfinite(out).all()) and bool((out[:, :3] != 0).any())


def test_gradient_and_sigma_bits_two_tiles_per_workgroup(dev, field):
    """m = 128 (CUs + 1) + 5: some workgroup runs two tiles -- the ring across a tile boundary, the
    prefetch of the next tile's chunks and A fragments, the trailing drain -- and the last tile is ragged."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    m = 128 * (cu + 1) + 5
    assert m < persistent_rows(cu), "smaller than the every-workgroup-twice size: one workgroup wraps"
    _check_points(field, _points(m, 17).to(dev))


@pytest.mark.parametrize("r,s", [(50, 3), (7, 16)])
def test_gradient_and_sigma_bits_ray_mode(dev, field, r, s):
    """Ray mode: the point is ro + rd z as the field forms it, the gradient is with respect to that point."""
    from codenerf import ops
    ro, rd, z = _rays(dev, r, s, 100 * r + s)
    cb = field.row(0)
    out = ops.density_gradient(field.packed, field.packed_t, cb, FX, ro=ro, rd=rd, z=z)
    assert out.shape == (r, s, 4)
    assert torch.equal(out[..., 3], ops.density_field(field.packed, cb, FX, ro=ro, rd=rd, z=z))
    pts = ro[:, None, :] + rd[:, None, :] * z[..., None]            # each operation rounded: mul_add_rn
    d_pts, sigma = composed(field, cb, pts)
    assert torch.equal(out[..., 3], sigma)
    assert same_values(out[..., :3], d_pts)
    assert torch.equal(out, ops.density_gradient(field.packed, field.packed_t, cb, FX, pts=pts))


def test_gradient_and_sigma_bits_beyond_fast_sincos(dev, field):
    """Every point beyond the fast sin / cos bound (|x| 2^9 > 2^14): the up-front sincosf path in every wave."""
    pts = _points(300, 23)
    pts = (pts.sign() + (pts == 0).float()) * (40.0 + pts.abs())      # every |coordinate| >= 40 > 32
    assert bool((pts.abs().amax(dim=-1) * 512.0 > 16384.0).all())
    _check_points(field, pts.to(dev))


def test_gradient_and_sigma_bits_one_wave_beyond_fast_sincos(dev, field):
    """One tile in which exactly one wave (rows 48..63) holds such a point: its waves take different paths."""
    pts = _points(128, 29) * 0.5
    pts[53] = torch.tensor([45.0, -38.0, 41.0])
    far = (pts.abs().amax(dim=-1) * 512.0 > 16384.0).view(8, 16).any(dim=-1)
    assert far.tolist() == [False, False, False, True, False, False, False, False]
    _check_points(field, pts.to(dev))


def test_integer_probe_model(dev):
    """A geometry probe model of tests/exact_cases.py (integer weights on the raw-input columns only, so
    every product and sum is exact) at integer points: the gradient is the float64 chain bit for bit."""
    from codenerf import ops
    state = probe_model(1, geometry=True)
    g = torch.Generator().manual_seed(2)
    z_s = torch.randint(-2, 3, (1, 256), generator=g).float()
    f = Field(dev, state, z_s)
    pts = torch.randint(-2, 3, (133, 3), generator=g).float()
    out = _check_points(f, pts.to(dev))
    grad, sigma = C.sigma_chain(state, z_s, pts)
    assert torch.equal(out[:, :3].cpu().double(), grad) and torch.equal(out[:, 3].cpu().double(), sigma)


# ---------------------------------------------------------------- c: code rows


@pytest.mark.parametrize("mode", ["pts", "rays"])
@pytest.mark.parametrize("layout", ["per_ray", "index"])
def test_code_rows_inside_a_wave(dev, field, layout, mode):
    """Code rows that change inside a wave (per-ray rows, or a code_index): every sample has, bit for bit,
    the single-code call's result for its own code."""
    from codenerf import ops
    r, s = 45, 3
    ro, rd, z = _rays(dev, r, s, 5)
    geo = dict(ro=ro, rd=rd, z=z) if mode == "rays" else dict(pts=ro[:, None, :] + rd[:, None, :] * z[..., None])
    index = torch.randint(0, 3, (r,), generator=torch.Generator().manual_seed(r)).to(dev)
    assert len(set(index[:5].tolist())) > 1, "the first wave (16 samples = 5 rays) mixes codes"
    single = torch.stack([ops.density_gradient(field.packed, field.packed_t, field.row(k), FX, **geo)
                          for k in range(3)])
    want = single[index, torch.arange(r, device=dev)]
    if layout == "index":
        got = ops.density_gradient(field.packed, field.packed_t, field.cb, FX, code_index=index, **geo)
    else:
        got = ops.density_gradient(field.packed, field.packed_t, field.cb[index].contiguous(), FX, **geo)
    assert got.shape == (r, s, 4) and torch.equal(got, want)
    assert not torch.equal(single[0], single[1])


# ---------------------------------------------------------------- d: accuracy

# The composed path's error against the float64 statement on an MI355X (profiles/densitygrad/parity.json,
# 1000 standard-normal points, one code row): max |d - d64| / max |d64| over the three gradient columns.
COMPOSED_ERR = {"hash": 2.780426175418111e-07, "trained": 2.5829496413549316e-07}


def _rel_err(got, want):
    return float((got.cpu().double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("weights", ["hash", "trained"])
def test_accuracy_against_float64(dev, weights):
    """Against tests/density_grad_cases.py's float64 statement on the hash-initialised and the
    trained-magnitude ("t4") synthetic weights, 1000 points.  The bound is twice the composed path's own
    error against the same float64 values, measured on an MI355X (COMPOSED_ERR; the project's 2x-measured
    rule).  Measured there: hash weights, composed path 2.78e-7 and this kernel 2.78e-7 (bound 5.56e-7);
    trained-magnitude weights, 2.58e-7 and 2.58e-7 (bound 5.17e-7) -- the kernel's values equal the
    composed path's, so the two errors are the same numbers.  sigma_raw: 2.6e-7 and 4.5e-6 absolute
    (profiles/densitygrad/parity.json)."""
    from codenerf import ops, synthetic
    if weights == "hash":
        state, z_s = synthetic.codenerf_params(0), synthetic.latent_codes(3, 1)
    else:
        state, z_s = synthetic.trained_params(0), synthetic.trained_codes(3, 1)
    f = Field(dev, state, z_s)
    pts = _points(1000, 41)
    want, sigma = C.sigma_autograd(state, z_s, pts)
    out = ops.density_gradient(f.packed, f.packed_t, f.row(0), FX, pts=pts.to(dev))
    d_pts, _ = composed(f, f.row(0), pts.to(dev).view(-1, 1, 3))
    print("COMPOSED", weights, _rel_err(d_pts.view(-1, 3), want))
    margin("test_accuracy_against_float64", f"gradient, {weights}", _rel_err(out[:, :3], want),
           2.0 * COMPOSED_ERR[weights], composed=COMPOSED_ERR[weights])
    margin("test_accuracy_against_float64", f"sigma_raw, {weights}",
           float((out[:, 3].cpu().double() - sigma).abs().max()), 1e-4)      # the project's raw-output bound


def test_nonfinite_points(dev, field):
    """NaN where the float64 statement is NaN, finite values elsewhere."""
    from codenerf import ops, synthetic
    inf, nan = float("inf"), float("nan")
    pts = _points(40, 43)
    pts[3] = torch.tensor([inf, 0.1, 0.2])
    pts[17, 1] = nan
    pts[18, 2] = -inf
    pts[39] = nan
    want, sigma = C.sigma_autograd(synthetic.codenerf_params(0), field.z_s[:1].cpu(), pts)
    out = _check_points(field, pts.to(dev)).cpu()                   # the composed path's NaNs too
    bad = torch.isnan(want).any(dim=-1)
    assert bad.nonzero().view(-1).tolist() == [3, 17, 18, 39] and bool(torch.isnan(sigma[bad]).all())
    # element by element: only the non-finite coordinate's own derivative (g x cos(inf)) is NaN; the other
    # two are finite on both sides -- torch's ReLU backward lets a gradient through a NaN pre-activation,
    # the kernel's mask bit (pre > 0) closes and gives 0 -- and their values are not compared
    assert torch.equal(torch.isnan(out[:, :3]), torch.isnan(want))
    assert torch.equal(torch.isnan(out[:, 3]), torch.isnan(sigma))
    assert bool(torch.isfinite(out[~torch.isnan(torch.cat((want, sigma[:, None]), dim=-1))]).all())
    assert bool(torch.isnan(out[39]).all())


# ---------------------------------------------------------------- e: buffers


@pytest.mark.parametrize("mode", ["pts", "rays"])
def test_buffers(dev, field, mode):
    """The output is written in full from stale memory, nothing is stored past its end or past any
    input's, and the inputs are unmodified."""
    from codenerf import ops
    r, s = 37, 5                              # 185 samples: a ragged second tile
    ro, rd, z = _rays(dev, r, s, 9)
    src = dict(ro=ro, rd=rd, z=z) if mode == "rays" else dict(pts=ro[:, None, :] + rd[:, None, :] * z[..., None])
    index = torch.randint(0, 3, (r,), generator=torch.Generator().manual_seed(1)).to(dev)
    want = ops.density_gradient(field.packed, field.packed_t, field.cb, FX, code_index=index, **src)
    results = {}
    for fill in buffers.FILLS:
        with buffers.contracts(fill) as arena:
            guarded = {}
            for name, t in dict(src, packed=field.packed, packed_t=field.packed_t, cb=field.cb, index=index).items():
                guarded[name] = arena.empty(t.shape, t.dtype, dev).copy_(t)
            before = arena.n_allocations
            geo = {k: guarded[k] for k in src}
            out = ops.density_gradient(guarded["packed"], guarded["packed_t"], guarded["cb"], FX,
                                       code_index=guarded["index"], **geo)
            assert arena.n_allocations == before + 1, "the output went through the guarded allocator"
            results[fill] = out
            for name, t in dict(src, packed=field.packed, packed_t=field.packed_t, cb=field.cb, index=index).items():
                assert torch.equal(guarded[name], t), f"{name} was modified"
        assert not bool(torch.isnan(out).any()), "a row of the output was left as it was"
        assert torch.equal(out, want)
    assert torch.equal(results["zero"], results["poison"])


# ---------------------------------------------------------------- f: the public layer


@pytest.fixture(scope="module")
def scene(dev):
    from codenerf import synthetic
    ms = models(dev, (0, 1))
    return ms, embedders(dev), synthetic.latent_codes(5, 1).to(dev), synthetic.latent_codes(6, 1).to(dev)


def test_nerf_density_gradient_and_normals(dev, scene):
    from codenerf import nerf, ops
    from codenerf.models.model import density_code_bias
    (m, _), emb, z_s, _ = scene
    cb = density_code_bias(m, z_s)
    for shape in ((130, 3), (9, 4, 3)):
        pts = torch.randn(*shape, generator=torch.Generator().manual_seed(len(shape))).to(dev)
        grad, sigma = nerf.density_gradient(m, emb, pts, z_s)
        assert grad.shape == shape and sigma.shape == shape[:-1]
        rows = ops.density_gradient(m.packed(), m.packed("f32_w16_t"), cb, FX, pts=pts.reshape(-1, 3))
        assert torch.equal(grad.reshape(-1, 3), rows[:, :3]) and torch.equal(sigma.reshape(-1), rows[:, 3])
        assert torch.equal(sigma, nerf.density(m, emb, pts, z_s))
        ga, sa = nerf.density_gradient(m, emb, pts, z_s, activated=True)
        assert torch.equal(sa, torch.nn.functional.softplus(sigma - 1.0))
        assert torch.equal(ga, grad * torch.sigmoid(sigma - 1.0)[..., None])
        n = nerf.normals(m, emb, pts, z_s)
        assert n.shape == shape and torch.equal(n, nerf._normals_from_gradient(grad))
        assert float((torch.linalg.vector_norm(n.double(), dim=-1) - 1).abs().max()) <= 1e-6
        assert bool(((n * grad).sum(-1) < 0).all()), "normals point towards lower density"
    # one code row per first-dimension row
    zs3 = torch.cat([z_s, z_s * 0.5, -z_s])
    pts = torch.randn(3, 7, 3, generator=torch.Generator().manual_seed(8)).to(dev)
    grad, sigma = nerf.density_gradient(m, emb, pts, zs3)
    for k in range(3):
        gk, sk = nerf.density_gradient(m, emb, pts[k], zs3[k:k + 1])
        assert torch.equal(grad[k], gk) and torch.equal(sigma[k], sk)
    # empty input: empty outputs, no launch
    for shape in ((0, 3), (0, 5, 3)):
        grad, sigma = nerf.density_gradient(m, emb, torch.empty(*shape, device=dev), z_s)
        assert grad.shape == shape and sigma.shape == shape[:-1]
        assert nerf.normals(m, emb, torch.empty(*shape, device=dev), z_s).shape == shape
    assert ops.density_gradient(m.packed(), m.packed("f32_w16_t"), cb, FX, pts=torch.empty(0, 3, device=dev)).shape \
        == (0, 4)


def test_extract_mesh_normals_and_colors(dev, scene):
    from codenerf import nerf
    (m, _), emb, z_s, z_t = scene
    nodes = nerf.density_grid(m, emb, z_s, 17, 1.0, activated=False)
    level = float(nodes.median())
    plain = nerf.extract_mesh(m, emb, z_s, 17, 1.0, level, activated=False)
    assert plain.n_vertices > 0 and plain.normals is None and plain.colors is None
    mesh = nerf.extract_mesh(m, emb, z_s, 17, 1.0, level, activated=False, normals=True, colors=True, z_t=z_t)
    assert torch.equal(mesh.vertices, plain.vertices) and torch.equal(mesh.faces, plain.faces)
    assert torch.equal(mesh.normals, nerf.normals(m, emb, mesh.vertices, z_s))
    length = torch.linalg.vector_norm(mesh.normals.double(), dim=-1)
    assert bool((((length - 1).abs() <= 1e-6) | (length == 0)).all())
    assert mesh.colors.shape == mesh.vertices.shape
    assert bool(((mesh.colors >= 0) & (mesh.colors <= 1)).all())
    v = mesh.n_vertices
    usable = torch.isfinite(mesh.normals).all(-1, keepdim=True) & (mesh.normals != 0).any(-1, keepdim=True)
    rd = torch.where(usable, -mesh.normals, torch.tensor([0.0, 0.0, -1.0], device=dev).expand(v, 3)).contiguous()
    with torch.no_grad():
        raw = nerf.forward_pass(m, emb, rd, mesh.vertices.view(v, 1, 3), (z_s, z_t))
    assert torch.equal(mesh.colors, torch.sigmoid(raw[:, 0, :3]))
    only_normals = nerf.extract_mesh(m, emb, z_s, 17, 1.0, level, activated=False, normals=True)
    assert torch.equal(only_normals.normals, mesh.normals) and only_normals.colors is None


# ---------------------------------------------------------------- g: the render's normal map


@pytest.mark.parametrize("option", ["plain", "occupancy", "rgb_tolerance"])
def test_render_normal_map(dev, scene, option):
    from codenerf import nerf, ops
    from codenerf.models.model import density_code_bias
    (mc, mf), emb, z_s, z_t = scene
    r = 37
    g = torch.Generator().manual_seed(12)
    ro = (torch.randn(r, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 1.3])).to(dev)
    rd = (torch.randn(r, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0])).to(dev)
    ps = nerf.PointSampler(8, 8, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    zs, zt = z_s.expand(r, -1), z_t.expand(r, -1)
    kw = {"plain": {}, "occupancy": dict(occupancy=nerf.OccupancyGrid.full(32, 0.45, dev)),
          "rgb_tolerance": dict(rgb_tolerance=1e-3)}[option]
    with torch.no_grad():
        base = nerf.render_rays(ro, rd, zs, zt, ps, emb, mc, mf, chunk_rows=16, **kw)
        out = nerf.render_rays(ro, rd, zs, zt, ps, emb, mc, mf, chunk_rows=16, normals=True, **kw)
    assert sorted(out) == sorted(list(base) + ["normal_fine"])
    for key, t in base.items():       # bit for bit (a ray with no weight at all has a NaN disparity in both)
        assert same_bits(out[key], t), key
    # the composition, recomputed: the fine weights from the render's own raw rows, the normals from the op
    z_f = out["z_fine"]
    with torch.no_grad():
        if option == "occupancy":
            raw = nerf._culled_field(mf, emb, rd, zs, zt, 16, ro, z_f, kw["occupancy"], density_only=True)
            assert bool((ops.volume_render(raw, z_f, rd)[3] == 0).any()), "the grid culls some fine samples"
        else:
            raw = nerf._density_field_raw(mf, emb, rd, zs, zt, 16, ro=ro, z=z_f)
        w = ops.volume_render(raw, z_f, rd)[3]
        rows = ops.density_gradient(mf.packed(), mf.packed("f32_w16_t"), density_code_bias(mf, z_s), FX,
                                    ro=ro, rd=rd, z=z_f)
    n = nerf._normals_from_gradient(rows[..., :3])
    want = torch.where(w[..., None] == 0, torch.zeros_like(n), w[..., None] * n).sum(dim=-2)
    assert out["normal_fine"].shape == (r, 3) and torch.equal(out["normal_fine"], want)
    assert bool(torch.isfinite(want).all())
    assert bool((torch.linalg.vector_norm(want, dim=-1) <= out["acc_fine"] + 1e-5).all())


def test_render_normal_map_refusals(dev, scene):
    from codenerf import nerf
    (mc, mf), emb, z_s, z_t = scene
    r = 5
    ro, rd, _ = _rays(dev, r, 1, 3)
    ps = nerf.PointSampler(8, 8, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    zs, zt = z_s.expand(r, -1), z_t.expand(r, -1)
    with torch.no_grad():
        with pytest.raises(ValueError):
            nerf.render_rays(ro, rd, zs, zt, ps, emb, mc, mf, coarse_only=True, normals=True)
        with pytest.raises(ValueError):
            nerf.render_rays(ro, rd, zs, zt, ps, emb, mc, None, normals=True)
    with torch.enable_grad():
        with pytest.raises(ValueError):
            nerf.render_rays(ro.clone().requires_grad_(True), rd, zs, zt, ps, emb, mc, mf, normals=True)


# ---------------------------------------------------------------- h: graph capture


def test_graph_capture(dev, field):
    """One cn_density_gradient call captured in a graph and replayed twice gives the eager bits."""
    from codenerf import _lib
    lib = _lib.load()
    pts = _points(300, 31).to(dev)
    cb = field.row(0)
    fx = _lib.host_floats(FX)
    out = torch.full((300, 4), float("nan"), device=dev)

    def call():
        rc = lib.cn_density_gradient(_lib.ptr(field.packed), _lib.ptr(field.packed_t), _lib.CN_FMT_F32_W16,
                                     _lib.CN_FMT_F32_W16_T, _lib.ptr(cb), None, 1, _lib.ptr(pts), None, None, None,
                                     300, 1, fx, _lib.ptr(out), _lib.stream_of(out))
        assert rc == _lib.CN_OK, rc

    call()
    torch.cuda.synchronize()
    eager = out.clone()
    assert bool(torch.isfinite(eager).all())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
