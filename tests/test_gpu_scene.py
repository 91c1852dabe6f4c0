"""Scene rendering on the device: cn_object_rays and cn_volume_render_compose against the rule of
include/codenerf.h (tests/scene_cases.py) and against cn_volume_render's own bits, and render_scene end
to end."""
import itertools

import numpy as np
import pytest
import torch

import buffers as B
import occupancy_cases as OC
import scene_cases as SC
from conftest import margin
from test_gpu_parity import dev, embedders, load, models  # noqa: F401

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def dev_bits(bits, dev):
    return T(np.asarray(bits).view(np.int32), dev)


def _same(a, b):
    """Bitwise equal values, NaN in the same places (disp is NaN where acc is 0)."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _pose_pairs(rows):
    return [(p[:9].reshape(3, 3).tolist(), p[9:].tolist()) for p in rows]


# ---------------------------------------------------------------- 1. object rays


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("r", [1, 5, 67])
def test_object_rays_bit_exact(dev, r, k):
    from codenerf import ops
    ro, rd = SC.pose_rays(r, seed=10 * r + k)
    poses = SC.poses(k)
    want_ro, want_rd = SC.object_rays(ro, rd, poses)
    got_ro, got_rd = ops.object_rays(T(ro, dev), T(rd, dev), _pose_pairs(poses))
    assert got_ro.shape == (k, r, 3) and got_rd.shape == (k, r, 3)
    assert np.array_equal(got_ro.cpu().numpy().view(np.uint32), want_ro.view(np.uint32))
    assert np.array_equal(got_rd.cpu().numpy().view(np.uint32), want_rd.view(np.uint32))


# ---------------------------------------------------------------- 2. one object is cn_volume_render


@pytest.mark.parametrize("r", [1, 3, 4, 67])
@pytest.mark.parametrize("s", [1, 2, 17, 64, 65, 128, 192, 512])
def test_one_object_is_volume_render(dev, r, s):
    """S = 64 with R % 4 == 0 is the existing kernel's grouped launch, 64 / 128 its FULL instances."""
    from codenerf import ops
    g = torch.Generator().manual_seed(1000 * s + r)
    raw = (torch.randn(r, s, 4, generator=g) * 2).to(dev)
    z = torch.sort(1 + torch.rand(r, s, generator=g), -1).values.to(dev)
    rd = torch.randn(r, 3, generator=g).to(dev)
    ref = ops.volume_render(raw, z, rd)
    got = ops.volume_render_compose([raw], z, rd)
    for name, a, b in zip(("rgb", "disp", "acc", "weights", "depth"), got, ref):
        if name == "disp":
            assert _same(a, b), name
        else:
            assert torch.equal(a, b), name
    assert got[5].shape == (1, r) and torch.equal(got[5][0], got[2])


# ---------------------------------------------------------------- 3. exclusive activity


@pytest.mark.parametrize("s", [17, 64, 192])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_exclusive_activity(dev, k, s):
    from codenerf import ops
    r = 37
    raws, z, rd, selected, owner = SC.exclusive_case(k, r, s, seed=31 * k + s)
    zd, rdd = T(z, dev), T(rd, dev)
    ref = ops.volume_render(T(selected, dev), zd, rdd)
    got = ops.volume_render_compose([T(raws[j], dev) for j in range(k)], zd, rdd)
    for name, a, b in zip(("rgb", "disp", "acc", "weights", "depth"), got, ref):
        assert _same(a, b), name
    # the all-empty ray
    assert not got[0][-1].any() and got[2][-1] == 0 and got[4][-1] == 0 and torch.isnan(got[1][-1])
    assert not got[5][:, -1].any()
    assert (got[2][:-1] > 0).all()
    # an object's mask is the sum of its own samples' weights: an fp32 sum of <= S terms, each partial sum
    # <= acc <= 1, against the float64 sum of the same fp32 weights
    w = got[3].double().cpu().numpy()
    for j in range(k):
        own = (w * (owner == j)).sum(axis=1)
        assert np.abs(got[5][j].double().cpu().numpy() - own).max() <= s * 2.0 ** -24
    # the order of the objects only permutes acc_objects' rows
    perms = list(itertools.permutations(range(k))) if k <= 3 else \
        [tuple(reversed(range(k))), (3, 0, 7, 1, 6, 2, 5, 4), (1, 2, 3, 4, 5, 6, 7, 0)]
    for perm in perms:
        alt = ops.volume_render_compose([T(raws[j], dev) for j in perm], zd, rdd)
        for name, a, b in zip(("rgb", "disp", "acc", "weights", "depth"), alt, got):
            assert _same(a, b), (perm, name)
        assert torch.equal(alt[5], got[5][list(perm)]), perm


# ---------------------------------------------------------------- 4. overlap


@pytest.mark.parametrize("s", [64, 192, 512])
@pytest.mark.parametrize("k", [2, 8])
def test_overlap_against_the_rule(dev, k, s):
    """Against the float64 rule.  The bound is the project's own for cn_volume_render against the oracle,
    5e-6 max(1, S / 256) (test_volume_render_sizes); the colour mix adds (K + 2) 1.2e-7 on the rgb
    channels (K products and sums and a division, each within 2^-24 relative of a colour <= 1.001)."""
    from codenerf import ops
    r = 129
    raws, z, rd = SC.overlap_case(k, r, s, seed=7 * k + s)
    want = SC.compose(raws, z, rd)
    got = ops.volume_render_compose([T(raws[j], dev) for j in range(k)], T(z, dev), T(rd, dev))
    got = dict(zip(("rgb", "disp", "acc", "weights", "depth", "acc_objects"), got))
    base = 5e-6 * max(1.0, s / 256)
    test = f"scene_overlap[k={k},s={s}]"
    _, _, _, active = SC.mix(raws)
    assert 0.05 < (active.sum(axis=0) > 1).mean() and (active.sum(axis=0) == 0).any()   # the cases do overlap
    for key in ("rgb", "acc", "depth", "weights", "acc_objects", "disp"):
        a, b = got[key].double().cpu().numpy(), want[key]
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin), key
        if key == "disp":        # 1 / (depth / acc): as test_gpu_parity, compared where the ray is not transparent
            fin = fin & (want["acc"] > 1e-6)
        err = np.abs(a[fin] - b[fin]).max() if fin.any() else 0.0
        margin(test, key, err, base + ((k + 2) * 1.2e-7 if key == "rgb" else 0.0), k=k, s=s)


# ---------------------------------------------------------------- 5. buffers


@pytest.mark.parametrize("want_acc_objects", [True, False])
@pytest.mark.parametrize("want_weights", [True, False])
def test_buffers(dev, want_weights, want_acc_objects):
    """Both entries under the poison-fill and guard harness at ragged sizes: every output is fully written
    (no NaN survives the poison), nothing is stored past an end, no result depends on the fill."""
    from codenerf import ops
    r, s, k = 67, 65, 3
    raws, z, rd = SC.overlap_case(k, r, s, seed=3)
    raws[:, :, 0] = (1.0, -1.0, 0.5, 2.0)         # no ray is empty: no NaN disp to expect
    ro, _ = SC.pose_rays(r, seed=4)
    args = ([T(raws[j], dev) for j in range(k)], T(z, dev), T(rd, dev))
    rod, poses = T(ro, dev), _pose_pairs(SC.poses(k))
    logs = {}
    for fill in B.FILLS:
        with B.contracts(fill) as arena:
            out = ops.volume_render_compose(*args, want_weights=want_weights, want_acc_objects=want_acc_objects)
            rays = ops.object_rays(rod, args[2], poses)
        assert arena.n_allocations == 4 + want_weights + want_acc_objects + 2
        assert (out[3] is None) == (not want_weights) and (out[5] is None) == (not want_acc_objects)
        for t in [t for t in out if t is not None] + list(rays):
            assert not bool(torch.isnan(t).any())
        logs[fill] = arena.returns
    assert [name for name, _, _ in logs["zero"]] == ["volume_render_compose", "object_rays"]
    B.compare_fills(logs["zero"], logs["poison"])
    # the optional outputs do not change the others
    full = ops.volume_render_compose(*args)
    for i in (0, 1, 2, 4):
        assert torch.equal(out[i], full[i])


# ---------------------------------------------------------------- 6. render_scene


FLIP_T = [0.1, -0.05, 0.2]
T_A, T_B, CUBE = [0.08, -0.31, -0.34], [0.32, 0.0, 0.46], 0.35      # disjoint cubes: 0.8 apart on z, 0.7 wide
SHARED = ("rgb_coarse", "disp_coarse", "acc_coarse", "weights_coarse", "depth_coarse", "z_coarse", "rgb_fine",
          "disp_fine", "acc_fine", "depth_fine", "z_fine")


@pytest.fixture(scope="module")
def scene(dev):
    """32 x 32 rays of the render_small.npz camera, the synthetic models, a 16 + 16 unperturbed sampler,
    G = 32 grids, and the renders several cases share."""
    from codenerf import ops, synthetic
    from codenerf.nerf import OccupancyGrid, PointSampler, RaySampler, SceneObject, render_rays, render_scene
    g = load("render_small.npz", dev)
    k = torch.tensor([[28.0, 0, 16.0, 0], [0, 28.0, 16.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    rs = RaySampler(32, 32, k, sample_size=1024, device=dev, datatype=torch.float32)
    ro, rd = (t.reshape(-1, 3) for t in rs.get_bundle(g["pose"]))
    mc, mf = models(dev)
    sc = dict(ro=ro, rd=rd, n=ro.shape[0], mc=mc, mf=mf, zs=g["z_s"], zt=g["z_t"], emb=embedders(dev),
              zs2=synthetic.latent_codes(11, 1).to(dev), zt2=synthetic.latent_codes(12, 1).to(dev),
              ps=PointSampler(16, 16, 0.8, 1.8, "lindepth", False, torch.float32, dev),
              sphere=OccupancyGrid(dev_bits(OC.grid_bits("sphere", 32, bound=1.0, radius=0.45), dev), 32, 1.0),
              empty=OccupancyGrid(dev_bits(OC.grid_bits("empty", 32), dev), 32, 1.0),
              cube=OccupancyGrid.full(32, CUBE, dev))

    def scene_render(objects, **kw):
        with torch.no_grad():
            return render_scene(ro, rd, objects, sc["ps"], sc["emb"], mc, mf, **kw)

    def plain_render(ro_, rd_, grid, **kw):
        with torch.no_grad():
            n = ro_.shape[0]
            return render_rays(ro_, rd_, sc["zs"].expand(n, -1), sc["zt"].expand(n, -1), sc["ps"], sc["emb"], mc, mf,
                               chunk_rows=None, occupancy=grid, **kw)

    sc["scene_render"], sc["plain_render"] = scene_render, plain_render
    sc["one"] = scene_render([SceneObject(sc["zs"], sc["zt"], sc["sphere"])])
    return sc


def test_scene_of_one_identity_object_is_render_rays(scene):
    """(a)"""
    sc = scene
    ref = sc["plain_render"](sc["ro"], sc["rd"], sc["sphere"])
    out = sc["one"]
    assert sorted(out) == sorted(SHARED + ("acc_objects_coarse", "acc_objects_fine")) and sorted(ref) == sorted(SHARED)
    for key in SHARED:
        assert _same(out[key], ref[key]), key
    assert out["acc_objects_fine"].shape == (1, sc["n"]) and torch.equal(out["acc_objects_fine"][0], out["acc_fine"])
    assert torch.equal(out["acc_objects_coarse"][0], out["acc_coarse"])
    assert 0.05 < float((out["acc_fine"] > 0).float().mean()) < 0.95         # the sphere is in view, and not all of it


def test_an_object_with_an_empty_grid_changes_nothing(scene):
    """(b)"""
    from codenerf.nerf import SceneObject
    sc = scene
    ghost = SceneObject(sc["zs2"], sc["zt2"], sc["empty"], rotation=SC.rotation([1, 2, 3], 0.5).tolist(),
                        translation=[0.1, 0.0, -0.1])
    out = sc["scene_render"]([SceneObject(sc["zs"], sc["zt"], sc["sphere"]), ghost])
    for key in SHARED:
        assert _same(out[key], sc["one"][key]), key
    for key in ("acc_objects_coarse", "acc_objects_fine"):
        assert torch.equal(out[key][0], sc["one"][key][0]) and not out[key][1].any(), key


def test_a_posed_object_is_render_rays_on_its_rays(scene):
    """(c) A half turn about z and a translation: the squares of rd's components are unchanged, so |rd| has
    the world ray's bits and the render of the object-frame rays is the scene's."""
    from codenerf import ops
    from codenerf.nerf import SceneObject
    sc = scene
    # the object sits where the camera looks: its frame's origin at t, the camera's rays turned into it
    out = sc["scene_render"]([SceneObject(sc["zs"], sc["zt"], sc["sphere"], rotation=SC.FLIP.tolist(),
                                          translation=FLIP_T)])
    ro_k, rd_k = ops.object_rays(sc["ro"], sc["rd"], [(SC.FLIP.tolist(), FLIP_T)])
    assert torch.equal(rd_k[0] * rd_k[0], sc["rd"] * sc["rd"])
    ref = sc["plain_render"](ro_k[0], rd_k[0], sc["sphere"])
    for key in SHARED:
        assert _same(out[key], ref[key]), key
    assert torch.equal(out["acc_objects_fine"][0], out["acc_fine"])
    assert float((out["acc_fine"] > 0).float().mean()) > 0.05 and not _same(out["rgb_fine"], sc["one"]["rgb_fine"])


def test_two_disjoint_objects(scene):
    """(d)"""
    from codenerf import ops
    from codenerf.nerf import SceneObject
    sc = scene
    a = SceneObject(sc["zs"], sc["zt"], sc["cube"], translation=T_A)
    b = SceneObject(sc["zs2"], sc["zt2"], sc["cube"], translation=T_B)
    assert max(abs(p - q) for p, q in zip(T_A, T_B)) > 2 * CUBE
    ab, ba, only_a = sc["scene_render"]([a, b]), sc["scene_render"]([b, a]), sc["scene_render"]([a])
    # swapped: identical bits, the masks' rows swapped
    for key in SHARED:
        assert _same(ab[key], ba[key]), key
    for key in ("acc_objects_coarse", "acc_objects_fine"):
        assert torch.equal(ab[key], ba[key][[1, 0]]), key
    # which rays have a coarse or fine sample in which cube: the grid lookup on the object-frame points
    ro_k, rd_k = (t.cpu().numpy() for t in ops.object_rays(sc["ro"], sc["rd"], [(a.rotation, T_A), (b.rotation, T_B)]))
    bits = OC.grid_bits("full", 32)
    hit = []
    for j in range(2):
        inside = [OC.lookup(OC.ray_points(ro_k[j], rd_k[j], ab[zkey].cpu().numpy()), bits, 32, CUBE).any(axis=1)
                  for zkey in ("z_coarse", "z_fine")]
        hit.append(inside[0] | inside[1])
    in_a, in_b = hit
    for kind in (in_a & ~in_b, in_b & ~in_a, in_a & in_b, ~in_a & ~in_b):
        assert kind.mean() >= 0.05, [float(x.mean()) for x in (in_a & ~in_b, in_b & ~in_a, in_a & in_b, ~in_a & ~in_b)]
    free = T(~in_b, sc["ro"].device)          # no sample in B's cube: the A-only render, bit for bit
    for key in SHARED:
        assert _same(ab[key][free], only_a[key][free]), key
    for key in ("acc_objects_coarse", "acc_objects_fine"):
        assert torch.equal(ab[key][0][free], only_a[key][0][free]) and not ab[key][1][free].any(), key
    # and B is seen on rays that do reach it
    assert (ab["acc_objects_fine"][1][T(in_b, free.device)] > 0).any()
    assert not _same(ab["rgb_fine"], only_a["rgb_fine"])


def test_two_overlapping_objects(scene):
    """(e) Two copies in the same place with different codes."""
    from codenerf.nerf import SceneObject
    sc = scene
    out = sc["scene_render"]([SceneObject(sc["zs"], sc["zt"], sc["sphere"]),
                              SceneObject(sc["zs2"], sc["zt2"], sc["sphere"])])
    # every entry of a pass is finite where that pass's acc > 0 (disp is NaN where it is 0: a ray the coarse
    # samples miss can still be hit by the fine ones)
    for key in SHARED + ("acc_objects_coarse", "acc_objects_fine"):
        seen = out["acc_coarse" if key.endswith("coarse") else "acc_fine"] > 0
        assert 0.05 < float(seen.float().mean())
        v = out[key][..., seen] if key.startswith("acc_objects") else out[key][seen]
        assert bool(torch.isfinite(v).all()), key
    s = out["z_fine"].shape[1]
    assert s == 32
    err = (out["acc_objects_fine"].double().sum(dim=0) - out["acc_fine"].double()).abs().max().item()
    margin("scene_overlapping_copies", "sum of acc_objects_fine - acc_fine", err, 16 * s * 2.0 ** -24)
    assert (out["acc_objects_fine"] > 0).all(dim=0).any()          # both objects weigh on some ray
    assert not _same(out["rgb_fine"], sc["one"]["rgb_fine"])


def test_density_only_coarse_pass(scene):
    """(f)"""
    from codenerf.nerf import SceneObject
    sc = scene
    objects = [SceneObject(sc["zs"], sc["zt"], sc["sphere"]),
               SceneObject(sc["zs2"], sc["zt2"], sc["cube"], rotation=SC.FLIP.tolist(), translation=[0.2, 0.1, 0.0])]
    full = sc["scene_render"](objects)
    lean = sc["scene_render"](objects, coarse_rgb=False)
    assert sorted(set(full) - set(lean)) == ["rgb_coarse"]
    for key in lean:
        assert _same(lean[key], full[key]), key
    coarse = sc["scene_render"](objects, coarse_only=True)
    assert sorted(coarse) == sorted(k for k in full if "coarse" in k)
    for key in coarse:
        assert _same(coarse[key], full[key]), key


def test_render_scene_refuses_gradients(scene, dev):
    """(g)"""
    from codenerf.nerf import SceneObject, render_scene
    sc = scene
    mc, mf = models(dev)
    for m in (mc, mf):
        m.requires_grad_(False)
    zs = sc["zs"].clone().requires_grad_(True)
    objects = [SceneObject(zs, sc["zt"], sc["sphere"])]
    n = 64
    args = (sc["ro"][:n], sc["rd"][:n], objects, sc["ps"], sc["emb"], mc, mf)
    with pytest.raises(ValueError):          # a code that requires grad, grad mode on
        render_scene(*args)
    plain = [SceneObject(sc["zs"], sc["zt"], sc["sphere"])]
    mc.requires_grad_(True)
    with pytest.raises(ValueError):          # trainable parameters, grad mode on
        render_scene(sc["ro"][:n], sc["rd"][:n], plain, sc["ps"], sc["emb"], mc, mf)
    with torch.no_grad():                    # the same inputs with grad mode off render
        out = render_scene(*args)
    assert "rgb_fine" in out and out["acc_objects_fine"].shape == (1, n)
