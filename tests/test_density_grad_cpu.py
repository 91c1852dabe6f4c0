"""The density gradient's float64 statement and the host-side rules built on it (no device): the two
statements of tests/density_grad_cases.py agree, the normals rule and the activated scaling of
codenerf.nerf follow their definitions, Mesh validates and writes its vertex attributes, and
"normal_fine" composes as stated."""
import math

import numpy as np
import pytest
import torch

import density_grad_cases as C


@pytest.fixture(scope="module")
def statement():
    """Both statements on the hash-initialised and the trained-magnitude synthetic weights, 200 points, one
    code row and one per point (computed once, read-only)."""
    from codenerf import synthetic
    out = {}
    g = torch.Generator().manual_seed(7)
    pts = torch.randn(200, 3, generator=g)
    for name, params, codes in (("hash", synthetic.codenerf_params(0), synthetic.latent_codes(3, 200)),
                                ("trained", synthetic.trained_params(0), synthetic.trained_codes(3, 200))):
        for layout, zs in (("one", codes[:1]), ("per_point", codes)):
            out[name, layout] = (C.sigma_autograd(params, zs, pts), C.sigma_chain(params, zs, pts))
    return out


@pytest.mark.parametrize("layout", ["one", "per_point"])
@pytest.mark.parametrize("weights", ["hash", "trained"])
def test_autograd_and_chain_agree(statement, weights, layout):
    (ga, sa), (gc, sc) = statement[weights, layout]
    assert ga.shape == (200, 3) and sa.shape == (200,)
    assert float(ga.abs().max()) > 0
    scale = float(ga.abs().max())
    assert float((ga - gc).abs().max()) <= 1e-12 * scale
    assert float((sa - sc).abs().max()) <= 1e-12 * float(sa.abs().max())


def test_statement_is_nan_at_nonfinite_points():
    from codenerf import synthetic
    pts = torch.tensor([[0.1, 0.2, 0.3], [float("inf"), 0.0, 0.0], [0.0, float("nan"), 0.0]])
    g, s = C.sigma_autograd(synthetic.codenerf_params(0), synthetic.latent_codes(3, 1), pts)
    assert bool(torch.isfinite(g[0]).all()) and bool(torch.isnan(g[1:]).any(dim=-1).all())
    assert bool(torch.isnan(s[1:]).all())


# ---------------------------------------------------------------- normals, activation


def test_normals_rule():
    from codenerf.nerf import _normals_from_gradient
    inf, nan = float("inf"), float("nan")
    g = torch.tensor([[3.0, 0.0, -4.0], [0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [nan, 1.0, 2.0], [1.0, inf, 0.0],
                      [-inf, -inf, 1.0], [0.0, -2.0, 0.0], [1e-30, 0.0, 0.0], [1e-3, 2e-3, -2e-3]])
    n = _normals_from_gradient(g)
    assert n.dtype == torch.float32 and n.shape == g.shape
    assert torch.equal(n[0], torch.tensor([-0.6, 0.0, 0.8]))          # towards lower density: -g / |g|
    for zero in (1, 2):
        assert bool((n[zero] == 0).all()), "a zero gradient has the zero normal, not NaN"
    for bad in (3, 4, 5):
        assert bool(torch.isnan(n[bad]).all()), "a non-finite gradient has a NaN normal in every component"
    assert torch.equal(n[6], torch.tensor([0.0, 1.0, 0.0]))
    assert torch.equal(n[7], torch.tensor([-1.0, 0.0, 0.0]))
    want = C.normals_rule(g.numpy())
    assert np.array_equal(np.isnan(want), torch.isnan(n).numpy())
    ok = ~np.isnan(want)
    assert np.abs(n.numpy()[ok] - want[ok]).max() <= 2 ** -22      # two fp32 roundings of values <= 1
    lengths = torch.linalg.vector_norm(n[[0, 6, 7, 8]].double(), dim=-1)
    assert float((lengths - 1).abs().max()) <= 1e-6


def test_activated_scaling_matches_autograd():
    """(grad, sigma_raw) -> (d softplus(sigma_raw - 1) / d p, softplus(sigma_raw - 1)): against autograd of
    torch's softplus (threshold 20) through a sigma_raw that is linear in p."""
    from codenerf.nerf import _activate_gradient
    sig = torch.tensor([-30.0, -3.0, 0.0, 1.0, 2.5, 20.5, 21.5, 60.0])
    g = torch.tensor([[1.0, -2.0, 0.5]]).expand(sig.shape[0], 3).contiguous()
    ga, sa = _activate_gradient(g, sig)
    p = torch.zeros(sig.shape[0], 3, dtype=torch.float64, requires_grad=True)
    raw = sig.double() + (p * g.double()).sum(-1)                   # d raw / d p = g at p = 0
    act = torch.nn.functional.softplus(raw - 1.0)
    want, = torch.autograd.grad(act.sum(), p)
    assert torch.equal(sa, torch.nn.functional.softplus(sig - 1.0))
    assert float((sa.double() - act.detach()).abs().max()) <= 1e-6 * float(act.detach().max())
    # torch's softplus is the identity above its threshold (derivative 1 there); sigmoid(20) = 1 - 2e-9
    assert float((ga.double() - want).abs().max()) <= 4e-7 * float(g.abs().max())
    assert bool((ga[0].abs() < 1e-12).all()) and torch.equal(ga[-1], g[-1])


# ---------------------------------------------------------------- "normal_fine"


def test_normal_composition_rule():
    from codenerf.nerf import _composite_normals
    g = torch.Generator().manual_seed(1)
    w = torch.rand(6, 5, generator=g)
    n = torch.randn(6, 5, 3, generator=g)
    n = n / torch.linalg.vector_norm(n, dim=-1, keepdim=True)
    w[0, 2] = 0.0
    n[0, 2] = float("nan")                       # culled sample with a NaN normal: contributes 0
    w[1] = 0.0
    n[1, 3] = float("inf")                       # a ray with no weight at all: exactly zero
    n[2, 1] = 0.0                                # a zero normal under a positive weight
    w[3, 0] = -0.0
    n[3, 0] = float("nan")                       # -0 is a zero weight too
    out = _composite_normals(w, n)
    assert out.shape == (6, 3) and bool(torch.isfinite(out).all())
    assert bool((out[1] == 0).all())
    want = C.composite_rule(w.numpy(), n.numpy())
    assert np.abs(out.numpy() - want).max() <= 5 * 2 ** -24
    acc = w.sum(-1)
    assert bool((torch.linalg.vector_norm(out, dim=-1) <= acc + 1e-6).all()), "|sum w n| <= sum w for unit n"
    n[4, 4] = float("nan")                       # NaN under a positive weight is not hidden
    assert bool(torch.isnan(_composite_normals(w, n)[4]).all())


# ---------------------------------------------------------------- Mesh


def _tetra():
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.1, 0.25, 1.0 / 3.0]])
    f = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=torch.int32)
    nrm = torch.tensor([[0.0, 0.0, -1.0], [0.6, 0.0, 0.8], [0.0, 1.0, 0.0], [1.0 / 3.0, -2.0 / 3.0, 2.0 / 3.0]])
    col = torch.tensor([[0.0, 0.5, 1.0], [0.25, 0.1, 0.999], [1.0, 1.0, 1.0], [0.002, 0.498, 0.502]])
    return v, f, nrm, col


def test_mesh_validates_attributes():
    from codenerf.nerf import Mesh
    v, f, nrm, col = _tetra()
    m = Mesh(v, f, normals=nrm, colors=col)
    assert m.normals is nrm and m.colors is col
    plain = Mesh(v, f)
    assert plain.normals is None and plain.colors is None
    with pytest.raises(TypeError):
        Mesh(v, f, nrm)                                   # keyword only
    for name in ("normals", "colors"):
        for bad in (nrm[:3], nrm.double(), nrm.reshape(-1), nrm[:, :2], nrm.to(torch.int32)):
            with pytest.raises(ValueError):
                Mesh(v, f, **{name: bad})
    for bad in (col + 0.01, col - 0.01, torch.full_like(col, float("nan"))):
        with pytest.raises(ValueError):
            Mesh(v, f, colors=bad)
    Mesh(v[:0], f[:0], normals=nrm[:0], colors=col[:0])   # empty meshes are meshes


@pytest.mark.parametrize("with_normals,with_colors", [(True, False), (False, True), (True, True)])
def test_mesh_files_carry_attributes(tmp_path, with_normals, with_colors):
    from codenerf.nerf import Mesh
    v, f, nrm, col = _tetra()
    m = Mesh(v, f, normals=nrm if with_normals else None, colors=col if with_colors else None)
    ply, obj = str(tmp_path / "m.ply"), str(tmp_path / "m.obj")
    m.save_ply(ply)
    m.save_obj(obj)
    names, verts, faces = C.read_ply(ply)
    assert names == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + \
        (["red", "green", "blue"] if with_colors else [])
    assert np.array_equal(np.stack([verts[k] for k in "xyz"], -1), v.numpy())
    assert np.array_equal(faces, f.numpy())
    if with_normals:
        assert np.array_equal(np.stack([verts[k] for k in ("nx", "ny", "nz")], -1), nrm.numpy())
    if with_colors:
        got = np.stack([verts[k] for k in ("red", "green", "blue")], -1)
        assert got.dtype == np.uint8
        want = [[min(255, max(0, int(math.floor(float(c) * 255.0 + 0.5)))) for c in row] for row in col.double()]
        # round(c * 255): no channel here sits on a .5 tie, so half-up and half-even agree
        assert got.tolist() == want and got[0].tolist() == [0, 128, 255] and got[3].tolist() == [1, 127, 128]
    vs, vns, fs = C.read_obj(obj)
    assert len(vs) == 4 and all(len(r) == (6 if with_colors else 3) for r in vs)
    assert np.array_equal(np.array(vs, dtype=np.float64)[:, :3].astype(np.float32), v.numpy())   # %.9g round-trips
    if with_colors:
        assert np.array_equal(np.array(vs, dtype=np.float64)[:, 3:].astype(np.float32), col.numpy())
    if with_normals:
        assert np.array_equal(np.array(vns, dtype=np.float64).astype(np.float32), nrm.numpy())
        assert fs == [["%d//%d" % (a + 1, a + 1) for a in row] for row in f.tolist()]
    else:
        assert vns == [] and fs == [[str(a + 1) for a in row] for row in f.tolist()]


def test_mesh_files_without_attributes_are_unchanged(tmp_path):
    """With neither attribute both writers produce the bytes they always did (stated here in full)."""
    from codenerf.nerf import Mesh
    v, f, _, _ = _tetra()
    ply, obj = str(tmp_path / "m.ply"), str(tmp_path / "m.obj")
    Mesh(v, f).save_ply(ply)
    Mesh(v, f).save_obj(obj)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\n"
              "property float z\nelement face 4\nproperty list uchar int vertex_indices\nend_header\n")
    rows = b"".join(b"\x03" + np.asarray(r, dtype="<i4").tobytes() for r in f.tolist())
    assert open(ply, "rb").read() == header.encode("ascii") + v.numpy().astype("<f4").tobytes() + rows
    text = "".join("v %.9g %.9g %.9g\n" % tuple(float(x) for x in r) for r in v.numpy()) + \
        "".join("f %d %d %d\n" % (a + 1, b + 1, c + 1) for a, b, c in f.tolist())
    assert open(obj).read() == text


def test_extract_mesh_colors_need_a_texture_code():
    from codenerf.nerf import extract_mesh
    with pytest.raises(ValueError):
        extract_mesh(None, None, torch.zeros(1, 256), 9, 1.0, 0.5, colors=True)
