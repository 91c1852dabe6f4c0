"""The density-only field kernel (cn_density_field) and what is built on it: sigma queries
(ops.density_field, CodeNeRFModel.density, nerf.density, nerf.density_grid) and the render whose
coarse pass computes densities only (render_rays / parallel_image_render with coarse_rgb=False).

The kernel runs the full field kernel's first ten weight chunks with the same instructions in the
same order, so wherever both exist the comparison is ``torch.equal`` against sigma_raw of the full
field (raw[..., 3]); independent of that kernel it is held to the project's raw-output bound
(1e-4 absolute) against the CPU oracle and the reference's fixture.
"""
import pytest
import torch

from conftest import margin
from test_gpu_parity import dev, embedders, load, maxdiff, models  # noqa: F401

pytestmark = pytest.mark.gpu

TOL_RAW = 1e-4       # raw MLP output, absolute (test_gpu_parity.py)
TOL_RENDER = 1e-4    # rendered rgb, absolute (test_gpu_parity.py)
FX = [2.0 ** k for k in range(10)]
FD = [2.0 ** k for k in range(4)]


@pytest.fixture(scope="module")
def field(dev):
    """The coarse synthetic model with its fp32 pack and parameter list (shared, read-only)."""
    m, = models(dev, (0,))
    return m, m.packed(), [p.detach() for p in m.param_list()]


def _codes(dev, layout, r, seed=3):
    """-> (z_s rows, z_t rows, code_index or None) on the device for a code layout over r rays."""
    from codenerf import synthetic
    n = {"one": 1, "per_ray": r, "index": 3}[layout]
    zs, zt = synthetic.latent_codes(seed, n).to(dev), synthetic.latent_codes(seed + 1, n).to(dev)
    index = None
    if layout == "index":      # codes varying inside a wave: the kernel's non-uniform branch
        index = torch.randint(0, 3, (r,), generator=torch.Generator().manual_seed(r)).to(dev)
    return zs, zt, index


def _geometry(dev, r, s, seed):
    g = torch.Generator().manual_seed(seed)
    rd = torch.randn(r, 3, generator=g)
    pts = torch.randn(r, s, 3, generator=g)
    ro = torch.randn(r, 3, generator=g) * 0.3
    z = torch.sort(0.8 + torch.rand(r, s, generator=g), dim=-1).values
    return rd.to(dev), pts.to(dev), ro.to(dev), z.to(dev)


def _both(field, cb, rd, s, index, **geo):
    """(density kernel's sigma, the full field's raw[..., 3]) on the same inputs and code terms."""
    from codenerf import ops
    _, packed, _ = field
    full = ops.radiance_field(packed, cb, rd, s, rd.shape[0], FX, FD, code_index=index, precision="f32_w16", **geo)
    dgeo = dict(geo, rd=rd) if "ro" in geo else geo
    sig = ops.density_field(packed, cb, FX, code_index=index, **dgeo)
    return sig, full[..., 3]


# ---------------------------------------------------------------- 1. bitwise against the full field


@pytest.mark.parametrize("layout", ["one", "per_ray", "index"])
@pytest.mark.parametrize("mode", ["pts", "rayz"])
@pytest.mark.parametrize("r,s", [(1, 1), (50, 8), (37, 64), (300, 3)])
def test_density_bitwise_vs_full_field(dev, field, r, s, mode, layout):
    from codenerf import ops
    rd, pts, ro, z = _geometry(dev, r, s, r * s)
    zs, zt, index = _codes(dev, layout, r)
    cb = ops.code_bias(field[2], zs, zt)
    geo = dict(pts=pts) if mode == "pts" else dict(ro=ro, z=z)
    sig, ref = _both(field, cb, rd, s, index, **geo)
    assert sig.shape == (r, s)
    assert torch.equal(sig, ref)


# ---------------------------------------------------------------- 2. several tiles per workgroup


def test_density_many_tiles_per_workgroup(dev, field):
    """m = 128 CU 5 + 77: every workgroup walks 5 (some 6) tiles, so the running ring counter passes
    its full period of two tiles more than once, and the last tile is ragged."""
    from codenerf import ops
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    m = 128 * cu * 5 + 77
    g = torch.Generator().manual_seed(5)
    pts = torch.randn(m, 1, 3, generator=g).to(dev)
    rd = torch.randn(m, 3, generator=g).to(dev)
    zs, zt, _ = _codes(dev, "one", m)
    cb = ops.code_bias(field[2], zs, zt)
    sig, ref = _both(field, cb, rd, 1, None, pts=pts)
    assert torch.equal(sig, ref)
    # codes that change from tile to tile and inside waves, over the same walk
    zs3, zt3, _ = _codes(dev, "index", m)
    index = (torch.arange(m, device=dev) // 100) % 3
    sig, ref = _both(field, ops.code_bias(field[2], zs3, zt3), rd, 1, index, pts=pts)
    assert torch.equal(sig, ref)


# ---------------------------------------------------------------- 3. large arguments


def _large_arg_case(case, r, s, seed):
    """test_gpu_parity's constructions: "far" puts (almost) every lane past fast_sincosf's argument
    bound (|x| 2^9 > 2^14), "mixed" one sample of one wave."""
    g = torch.Generator().manual_seed(seed)
    rd = torch.randn(r, 3, generator=g)
    pts = torch.randn(r, s, 3, generator=g)
    if case == "far":
        pts = pts * 40.0
    else:
        pts[37, 5] = torch.tensor([45.0, -38.0, 41.0])
    return rd, pts


@pytest.mark.parametrize("mode", ["pts", "rayz"])
@pytest.mark.parametrize("case", ["far", "mixed"])
def test_density_large_arguments(dev, field, case, mode):
    """The per-wave sincosf branch ("far") and a tile whose waves take different branches ("mixed")."""
    from codenerf import ops
    r, s = 300, 64
    rd, pts = _large_arg_case(case, r, s, 11)
    rd, pts = rd.to(dev), pts.to(dev)
    geo = dict(pts=pts)
    if mode == "rayz":       # pts = ro + rd z formed in the kernel: far rays from far origins
        z = torch.sort(0.8 + torch.rand(r, s, generator=torch.Generator().manual_seed(3)), dim=-1).values
        geo = dict(ro=pts[:, 0, :].clone(), z=z.to(dev))
    zs, zt, _ = _codes(dev, "per_ray", r)
    sig, ref = _both(field, ops.code_bias(field[2], zs, zt), rd, s, None, **geo)
    assert torch.equal(sig, ref)


# ---------------------------------------------------------------- 4. independent of the full kernel


@pytest.fixture(scope="module")
def oracle_50x8():
    """The CPU oracle's raw output at (50, 8) with per-ray codes (inputs on the CPU)."""
    from codenerf import synthetic
    from oracle import codenerf_oracle as O
    r, s = 50, 8
    torch.manual_seed(r * s)
    rd, pts = torch.randn(r, 3), torch.randn(r, s, 3)
    zs, zt = synthetic.latent_codes(3, r), synthetic.latent_codes(4, r)
    ref = O.forward_pass(synthetic.codenerf_params(0), O.EmbedCfg(), rd, pts, zs, zt)
    return pts, zs, ref


def test_density_vs_oracle(dev, field, oracle_50x8):
    from codenerf.nerf import density
    pts, zs, ref = oracle_50x8
    sig = density(field[0], embedders(dev), pts.to(dev), zs.to(dev))
    assert sig.shape == (50, 8)
    margin("density_vs_oracle[f32]", "sigma_raw", maxdiff(sig, ref[..., 3]), TOL_RAW)


# ---------------------------------------------------------------- 5. reference fixture


def test_model_density_golden(dev, field):
    """CodeNeRFModel.density on the reference's encoded rows: (M, 90) and their (M, 63) slice."""
    g = load("mlp.npz", dev)
    m = field[0]
    with torch.no_grad():
        s90 = m.density(g["z_s"], g["x"])
        s63 = m.density(g["z_s"], g["x"][:, :63].contiguous())
    assert s90.shape == (g["x"].shape[0],)
    margin("model_density_golden[f32]", "sigma_raw (M,90)", maxdiff(s90, g["raw"][:, 3]), TOL_RAW)
    margin("model_density_golden[f32]", "sigma_raw (M,63)", maxdiff(s63, g["raw"][:, 3]), TOL_RAW)
    assert torch.equal(s90, s63)
    with torch.no_grad():
        assert torch.equal(s90, m(g["z_s"], g["z_t"], g["x"])[:, 3])      # and the full kernel's bits


# ---------------------------------------------------------------- 6. texture independence


def test_density_ignores_texture_code(dev, field):
    from codenerf import ops, synthetic
    r, s = 37, 16
    _, pts, _, _ = _geometry(dev, r, s, 6)
    zs = synthetic.latent_codes(3, r).to(dev)
    outs = [ops.density_field(field[1], ops.code_bias(field[2], zs, synthetic.latent_codes(seed, r).to(dev)), FX,
                              pts=pts) for seed in (4, 9)]
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------- 7. output forms


def test_density_output_forms(dev, field):
    from codenerf import ops
    r, s = 50, 8
    _, pts, _, _ = _geometry(dev, r, s, 7)
    zs, zt, _ = _codes(dev, "one", r)
    cb = ops.code_bias(field[2], zs, zt)
    sig = ops.density_field(field[1], cb, FX, pts=pts)
    raw = ops.density_field(field[1], cb, FX, pts=pts, want_sigma=False, want_raw=True)
    sig2, raw2 = ops.density_field(field[1], cb, FX, pts=pts, want_raw=True)
    assert sig.shape == (r, s) and raw.shape == (r, s, 4)
    assert torch.equal(sig, sig2) and torch.equal(raw, raw2)
    assert bool((raw[..., :3] == 0).all()) and torch.equal(raw[..., 3], sig)
    flat = ops.density_field(field[1], cb, FX, pts=pts.reshape(-1, 3))        # the (M, 3) form
    assert flat.shape == (r * s,) and torch.equal(flat, sig.reshape(-1))


# ---------------------------------------------------------------- 8. render


def _image_rays(dev, g, h, w):
    from codenerf.nerf import RaySampler
    rs = RaySampler(h, w, g["intrinsics"].cpu(), sample_size=min(4096, h * w), device=dev, datatype=torch.float32)
    ro, rd = rs.get_bundle(g["pose"])
    return rs, ro.reshape(-1, 3), rd.reshape(-1, 3)


RENDER_KEYS = ("weights_coarse", "acc_coarse", "depth_coarse", "z_fine", "rgb_fine", "depth_fine", "acc_fine")


@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("chunk_rows", [256, 100, 50])
@pytest.mark.parametrize("nc,nf", [(8, 8), (32, 128)])
def test_render_density_coarse_bitwise(dev, nc, nf, chunk_rows, perturb):
    """render_rays(coarse_rgb=False) against the default call on the render_small.npz view (its 192
    rays).  chunk_rows 256 (one chunk) and 100 (not dividing) are the bitwise cases; 50 is the
    fixture's own chunking, where rgb_fine is also held to its golden value."""
    from codenerf.nerf import PointSampler, render_rays
    g = load("render_small.npz", dev)
    _, ro, rd = _image_rays(dev, g, 12, 16)
    n = ro.shape[0]
    ps = PointSampler(nc, nf, 0.8, 1.8, "lindepth", perturb, torch.float32, dev)
    mc, mf = models(dev)
    kw = {}
    if perturb:
        gen = torch.Generator().manual_seed(nc)
        kw = dict(t_rand=g["p_t_rand"] if nc == 8 else torch.rand(n, nc, generator=gen).to(dev),
                  u=g["p_u"] if nf == 8 else torch.rand(n, nf, generator=gen).to(dev))
    zs, zt = g["z_s"].expand(n, -1), g["z_t"].expand(n, -1)
    with torch.no_grad():
        ref = render_rays(ro, rd, zs, zt, ps, embedders(dev), mc, mf, chunk_rows=chunk_rows, **kw)
        out = render_rays(ro, rd, zs, zt, ps, embedders(dev), mc, mf, chunk_rows=chunk_rows, coarse_rgb=False, **kw)
    assert "rgb_coarse" not in out and "rgb_coarse" in ref
    for k in RENDER_KEYS:
        assert torch.equal(out[k], ref[k]), k
    if chunk_rows == 50:
        gold = "p_rgb_fine" if perturb else f"nc{nc}_n1_rgb"
        if not perturb or (nc, nf) == (8, 8):
            margin(f"render_density_coarse[nc{nc}{'_p' if perturb else ''}]", "rgb_f",
                   maxdiff(out["rgb_fine"], g[gold]), TOL_RENDER)


# ---------------------------------------------------------------- 9. parallel_image_render


def _render_cfg(dev, g):
    from types import SimpleNamespace as NS
    from codenerf.nerf import PointSampler, RaySampler
    rs = RaySampler(12, 16, g["intrinsics"].cpu(), sample_size=64, device=dev, datatype=torch.float32)
    ps = PointSampler(8, 8, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    mc, mf = models(dev)
    cfg = NS(is_distributed=False, gpus=1, nerf=NS(validation=NS(chunksize=50)))
    return cfg, {"nerf_coarse": mc, "nerf_fine": mf}, (rs, ps)


def test_parallel_image_render_density_coarse(dev):
    from codenerf.nerf import parallel_image_render
    g = load("render_small.npz", dev)
    cfg, mdls, samplers = _render_cfg(dev, g)
    args = (cfg, g["pose"], [g["z_s"], g["z_t"]], mdls, samplers, embedders(dev), dev)
    ref = parallel_image_render(*args)
    out = parallel_image_render(*args, coarse_rgb=False)
    assert torch.equal(out, ref)
    margin("parallel_image_render_density_coarse[f32]", "rgb_f", maxdiff(out, g["nc8_n1_rgb"]), TOL_RENDER)


# ---------------------------------------------------------------- 10. density_grid


def test_density_grid(dev, field):
    from codenerf import synthetic
    from codenerf.nerf import density, density_grid
    from oracle import codenerf_oracle as O
    m, emb, d, bound = field[0], embedders(dev), 9, 1.0
    zs = synthetic.latent_codes(5, 1)
    raw = density_grid(m, emb, zs.to(dev), d, bound, activated=False)
    assert raw.shape == (d, d, d)
    lin = torch.linspace(-bound, bound, d)
    pts = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), dim=-1)        # [ix, iy, iz]
    assert torch.equal(raw, density(m, emb, pts.to(dev), zs.to(dev)))
    assert torch.equal(raw, density_grid(m, emb, zs.to(dev), d, bound, activated=False, max_points=200))
    act = density_grid(m, emb, zs.to(dev), d, bound)
    assert torch.equal(act, density_grid(m, emb, zs.to(dev), d, bound, max_points=200))
    # the oracle's sigma at the same points (its view direction and texture code do not reach sigma)
    flat = pts.reshape(-1, 1, 3)
    n = flat.shape[0]
    ref = O.forward_pass(synthetic.codenerf_params(0), O.EmbedCfg(), torch.ones(n, 3), flat, zs.expand(n, -1),
                         synthetic.latent_codes(6, 1).expand(n, -1))[..., 3].reshape(d, d, d)
    margin("density_grid[f32]", "sigma_raw", maxdiff(raw, ref), TOL_RAW)
    margin("density_grid[f32]", "softplus(sigma_raw - 1)", maxdiff(act, torch.nn.functional.softplus(ref - 1.0)),
           TOL_RAW)


# ---------------------------------------------------------------- torch.ops


def test_torch_op_density_field(dev, field):
    import codenerf.torch_ops  # noqa: F401
    from codenerf import synthetic
    from codenerf.nerf import density
    _, pts, _, _ = _geometry(dev, 37, 5, 8)
    zs = synthetic.latent_codes(5, 1).to(dev)
    got = torch.ops.codenerf.density_field(zs, pts, field[2])
    assert torch.equal(got, density(field[0], embedders(dev), pts, zs))


# ---------------------------------------------------------------- 11. errors and edges


def test_density_empty_batch_launches_nothing(dev, field, monkeypatch):
    from codenerf import ops
    from codenerf.nerf import density
    zs, zt, _ = _codes(dev, "one", 1)
    cb = ops.code_bias(field[2], zs, zt)
    lib = ops._lib_ready()

    class NoLaunch:
        def __getattr__(self, name):
            if name == "cn_density_field":
                raise AssertionError("an empty batch must not reach the kernel")
            return getattr(lib, name)

    monkeypatch.setattr(ops, "_lib_ready", lambda: NoLaunch())
    sig, raw = ops.density_field(field[1], cb, FX, pts=torch.empty(0, 4, 3, device=dev), want_raw=True)
    assert sig.shape == (0, 4) and raw.shape == (0, 4, 4)
    assert ops.density_field(field[1], cb, FX, x=torch.empty(0, 63, device=dev)).shape == (0,)
    assert density(field[0], embedders(dev), torch.empty(0, 3, device=dev), zs).shape == (0,)


def test_density_render_errors(dev):
    from codenerf.nerf import PointSampler, parallel_image_render, render_rays
    g = load("render_small.npz", dev)
    _, ro, rd = _image_rays(dev, g, 12, 16)
    n = ro.shape[0]
    ps = PointSampler(8, 8, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    mc, mf = models(dev)
    for m in (mc, mf):
        m.requires_grad_(False)
    zs = g["z_s"].clone().requires_grad_(True)
    with pytest.raises(ValueError):          # a code that requires grad, grad mode on
        render_rays(ro, rd, zs.expand(n, -1), g["z_t"].expand(n, -1), ps, embedders(dev), mc, mf, chunk_rows=50,
                    coarse_rgb=False)
    with torch.no_grad():                    # the same inputs with grad mode off render
        out = render_rays(ro, rd, zs.expand(n, -1), g["z_t"].expand(n, -1), ps, embedders(dev), mc, mf,
                          chunk_rows=50, coarse_rgb=False)
    assert "rgb_fine" in out and "rgb_coarse" not in out
    cfg, mdls, samplers = _render_cfg(dev, g)
    with pytest.raises(ValueError):
        parallel_image_render(cfg, g["pose"], [g["z_s"], g["z_t"]], mdls, samplers, embedders(dev), dev,
                              key="rgb_coarse", coarse_rgb=False)


@pytest.mark.parametrize("precision", ["bf16x3", "f32_v1", "bf16x3_w16"])
def test_density_other_precisions_refuse(dev, precision):
    """No silent fall-back to another arithmetic: a model that does not run the fp32 16x16x4 kernel
    raises from every density entry point."""
    from codenerf import synthetic
    from codenerf.nerf import PointSampler, density, density_grid, render_rays
    m, mf = models(dev, precision=precision)
    zs = synthetic.latent_codes(5, 1).to(dev)
    emb = embedders(dev)
    with pytest.raises(NotImplementedError, match="f32"):
        density(m, emb, torch.zeros(4, 3, device=dev), zs)
    with pytest.raises(NotImplementedError, match="f32"):
        density_grid(m, emb, zs, 3, 1.0)
    with pytest.raises(NotImplementedError, match="f32"):
        m.density(zs.expand(4, -1), torch.zeros(4, 63, device=dev))
    ps = PointSampler(8, 8, 0.8, 1.8, "lindepth", False, torch.float32, dev)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="f32"):
        render_rays(torch.zeros(4, 3, device=dev), torch.ones(4, 3, device=dev), zs.expand(4, -1), zs.expand(4, -1),
                    ps, emb, m, mf, chunk_rows=4, coarse_rgb=False)
