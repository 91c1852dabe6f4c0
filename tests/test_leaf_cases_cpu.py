"""The input sets of tests/leaf_cases.py are usable (CPU only): each reaches the branch it is built for,
the NaN patterns are the stated ones, there are at least the stated numbers of cases, and the oracle's own
fp32 run stays within HALF of each bound against its float64 run, so the bounds the GPU tests hold the
kernels to (tests/test_gpu_leaf_edges.py) are feasible for a correct fp32 implementation."""
import math

import pytest
import torch

import leaf_cases as L

F32, F64 = torch.float32, torch.float64
GRAD_RTOL = 2e-4      # tests/test_gpu_grad.py (not imported: that module is all-GPU)


# ---------------------------------------------------------------- volume render


@pytest.mark.parametrize("r,s", L.VOLUME_SHAPES)
@pytest.mark.parametrize("regime", L.VOLUME_REGIMES)
def test_volume_oracle_fp32_within_half_bound(regime, r, s):
    ref, own = L.volume_forward(regime, r, s, F64), L.volume_forward(regime, r, s, F32)
    for name, a, b in zip(L.VOLUME_TERMS, own, ref):
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b)), name
        fin = torch.isfinite(b)
        err = (a.double()[fin] - b[fin]).abs().max().item() if fin.any() else 0.0
        assert err <= 0.5 * L.volume_bound(s), (name, err)
    if s > 1:
        terms = L.volume_loss_terms(regime)
        for name, a, b in zip(("d raw", "d rd"), L.volume_grads(regime, r, s, terms, F32),
                              L.volume_grads(regime, r, s, terms, F64)):
            assert torch.isfinite(b).all(), name
            assert L.rel_err(a, b) <= 0.5 * GRAD_RTOL, (name, L.rel_err(a, b))


@pytest.mark.parametrize("r,s", L.VOLUME_SHAPES)
def test_volume_regimes_reach_their_branches(r, s):
    case = {k: L.volume_case(k, r, s) for k in L.VOLUME_REGIMES}
    # opaque: the softplus threshold branch (x > 20) on every ray, twice on the even ones
    x = case["opaque"]["raw"][..., 3] - 1
    assert bool((x[:, s // 3] > 20).all()) and bool((x[::2, 0] > 20).all())
    if 1 < s <= 7:
        # widely spaced samples: the transmittance behind the opaque first sample is below 1e-3 on most
        # even rays, so every later weight is a product with a nearly underflowed factor
        w = L.volume_forward("opaque", r, s)[3]
        assert int((w[::2, 0] > 1 - 1e-3).sum()) >= (r + 1) // 4
    # transparent: every third ray has acc == 0 exactly and disp NaN in float64, the others a tiny positive acc
    _, disp, acc, _, _ = L.volume_forward("transparent", r, s)
    zero = torch.zeros(r, dtype=torch.bool)
    zero[::3] = True
    assert torch.equal(acc == 0, zero if s > 1 else torch.ones(r, dtype=torch.bool))
    assert torch.equal(torch.isnan(disp), acc == 0)
    if s > 1:
        assert bool((acc[~zero] > 0).all()) and bool((acc[~zero] < 1e-2).all())
        assert L.volume_zero_acc_rays("transparent", r, s).tolist() == list(range(0, r, 3))
    # ties: odd depths equal their left neighbour, every fourth ray has one depth
    z = case["ties"]["z"]
    assert torch.equal(z[:, 1::2], z[:, 0::2][:, :z[:, 1::2].shape[1]])
    assert bool((z[::4] == z[::4, :1]).all()) and bool((z[:, 1:] >= z[:, :-1]).all())
    # rdscale: |rd| three decades either side of 1
    n = case["rdscale"]["rd"].norm(dim=-1)
    assert bool((n[::2] > 30).all()) and bool((n[1::2] < 3e-2).all())
    # satcol: every colour logit saturates the sigmoid in fp32
    c = case["satcol"]["raw"][..., :3]
    assert bool((c.abs() == 40).all()) and bool((c > 0).any()) and bool((c < 0).any())
    # zero_rd: exactly two rays with rd == 0: acc == 0 and disp NaN there
    rd = case["zero_rd"]["rd"]
    assert (rd.abs().sum(-1) == 0).nonzero().flatten().tolist() == list(L.VOLUME_ZERO_RD_RAYS)
    if s > 1:
        assert L.volume_zero_acc_rays("zero_rd", r, s).tolist() == list(L.VOLUME_ZERO_RD_RAYS)


@pytest.mark.parametrize("s", L.VOLUME_VARIANT_S)
@pytest.mark.parametrize("regime,term", L.VOLUME_SINGLE_UPSTREAM)
def test_volume_single_upstream_cases_have_a_scale(regime, term, s):
    """Every upstream gradient is run alone, each on a regime where its gradients are not identically zero, and
    the fp32 oracle is within half of close()'s bound there."""
    assert {t for _, t in L.VOLUME_SINGLE_UPSTREAM} == set(L.VOLUME_TERMS)
    ref, own = L.volume_grads(regime, 21, s, (term,), F64), L.volume_grads(regime, 21, s, (term,), F32)
    for what, a, b in zip(("d raw", "d rd"), own, ref):
        scale = b.abs().max().item()
        assert scale > 1e-5, (what, scale)
        assert (a.double() - b).abs().max().item() <= 0.5 * (GRAD_RTOL * scale + 1e-7), what
    # d acc vanishes identically (to float64 rounding) where the last interval is opaque
    for other in ("opaque", "ties"):
        assert max(g.abs().max().item() for g in L.volume_grads(other, 21, s, ("acc",), F64)) < 1e-12


def test_volume_shapes_cover_every_instance():
    s_of = sorted({s for _, s in L.VOLUME_SHAPES})
    assert s_of == [1, 2, 7, 64, 65, 128, 129, 300]
    assert (20, 64) in L.VOLUME_SHAPES and (21, 64) in L.VOLUME_SHAPES       # grouped and per-group forward
    assert 21 % 4 != 0 and 21 % 16 != 0 and 21 > 16                          # ragged wave, second workgroup
    assert set(L.VOLUME_VARIANT_S) == {7, 129}


# ---------------------------------------------------------------- loss


def test_loss_cases_reach_their_rounds():
    assert [3 * n for n in L.LOSS_RAYS] == [3, 4095, 4098]                   # 4096 elements per round
    assert [a * b for a, b in L.LOSS_CODES] == [0, 256, 2048, 2304]          # workspace boundary: 2048 / 2049
    assert 2304 % 1024 != 0                                                  # the last partial block is ragged
    c = L.loss_case(1366, 4, (9, 256))
    out, *grads = L.loss_reference(c["rgb_c"], c["rgb_f"], c["target"], c["z_s"], c["z_t"], 300)
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(g).all()) for g in grads)
    # fp32 torch (the reference's arithmetic) is within half of the 1e-5 bound of float64
    lc = torch.nn.functional.mse_loss(c["rgb_c"], c["target"][:, :3])
    assert abs(lc.item() - out[0].item()) <= 0.5e-5 * out[0].item()


# ---------------------------------------------------------------- AdamW


def test_adam_layout_needs_two_launches():
    groups, has_grad = L.adam_layout()
    sizes = [t.numel() for grp in groups for t in grp]
    assert min(sizes) >= 4 and max(sizes) <= 40 and max(sizes) == 40 and min(sizes) == 4
    flags = [h for hh in has_grad for h in hh]
    assert sum(flags) == 12 >= 11 and not any(a and b for a, b in zip(flags, flags[1:]))   # never adjacent
    assert 1 - L.ADAM_BETAS[0] >= 0.5
    _, segs = L.adam_flat_case()
    assert len(segs) == 11 and all(b % 4 == 0 and e % 4 == 0 and b < e for b, e, *_ in segs)
    assert segs[0][0] > 0 and all(a[1] < b[0] for a, b in zip(segs, segs[1:]))            # gaps everywhere
    assert len({s[2] for s in segs}) == 11                                                 # every lr its own


def test_adam_float64_bound():
    """ADAM_F64_BOUND is 4 x torch's own fp32-vs-float64 error on these inputs (measured here)."""
    worst = 0.0
    for wd in (0.0, 0.5):
        e = L.adam_err(L.adam_torch_run(wd, F32), L.adam_torch_run(wd, F64))
        print("adam fp32 vs float64", wd, e)
        worst = max(worst, *e.values())
    assert worst <= L.ADAM_F64_ERR_MEASURED * 1.0001, worst
    assert worst >= L.ADAM_F64_ERR_MEASURED * 0.5, worst
    assert L.ADAM_F64_BOUND == 4 * L.ADAM_F64_ERR_MEASURED


# ---------------------------------------------------------------- rays and pose


def test_ray_selections():
    assert L.RAY_HW == 4608 > 2 * 2048 and L.RAY_B == 3
    assert [None if k is None else L.selection(k).shape[1] for k in L.POSE_SELECTIONS] == [1, 2047, 2049, None, 2049]
    for k in (1, 2047, 2049):
        assert L.repeated_fraction(L.selection(k)) == 0.0
    rep = L.selection("repeat")
    assert L.repeated_fraction(rep) >= 0.10, L.repeated_fraction(rep)
    assert bool((rep[:, 0] == rep[:, 1]).all())
    bad, mask = L.with_bad_indices(L.selection(2049), L.RAY_HW)
    assert bool(((bad == -1) | (bad == L.RAY_HW)).eq(mask).all()) and int(mask.sum()) >= 3 * L.RAY_B
    assert bool((bad == -1).any()) and bool((bad == L.RAY_HW).any())


@pytest.mark.parametrize("kind", L.POSE_SELECTIONS)
def test_pose_backward_reference_is_finite(kind):
    c = L.pose_case(kind)
    dirs = L.ray_dirs()
    for kw in ({"angles": c["angles"]}, {"c2w": c["c2w"]}):
        ang, d_c2w = L.pose_grads(dirs, c["sel"], c["g_ro"], c["g_rd"], F64, **kw)
        assert d_c2w.dtype == F64 and bool(torch.isfinite(d_c2w).all()) and bool((d_c2w[:, 3] == 0).all())
        ang32, d32 = L.pose_grads(dirs, c["sel"], c["g_ro"], c["g_rd"], F32, **kw)
        assert d32.dtype == F32
        # the bound the GPU test uses is max(1e-5, 4 x this); the fp32 oracle itself is far inside it
        assert L.rel_err(d32, d_c2w) <= 0.25 * L.ray_bound(d_c2w, d32)
        if ang is not None:
            assert all(bool(torch.isfinite(a).all()) for a in ang)


# ---------------------------------------------------------------- positional encoding


@pytest.mark.parametrize("m", L.POSENC_ROWS)
@pytest.mark.parametrize("name", [c[0] for c in L.POSENC_CONFIGS])
def test_posenc_oracle_fp32_within_half_bound(name, m):
    c = L.posenc_case(name, m)
    enc, dx = L.posenc_reference(c["x"], c["freqs"], c["inc"], c["g"])
    own = L.O.posenc(c["x"], c["freqs"], c["inc"])
    assert own.shape == enc.shape == c["g"].shape
    assert (own.double() - enc).abs().max().item() <= 0.5 * L.POSENC_FWD_ATOL
    x = c["x"].clone().requires_grad_(True)
    (L.O.posenc(x, c["freqs"], c["inc"]) * c["g"]).sum().backward()
    assert L.rel_err(x.grad, dx) <= 0.5 * L.POSENC_BWD_RTOL
    if name == "identity":
        assert torch.equal(own, c["x"]) and torch.equal(dx.float(), c["g"])
    if name == "xyz10_far":
        assert c["x"].abs().max().item() * 2 ** 9 > 1e4          # arguments far past any fast-sine range
    if name == "linear6":
        assert bool((c["freqs"][1:-1] != 2 ** torch.log2(c["freqs"][1:-1]).round()).all())   # products round


# ---------------------------------------------------------------- SE3


def test_se3_degenerate_branches():
    gt, cam = L.se3_degenerate()
    assert gt.shape == cam.shape == (224, 4, 4) and 224 > 3 * 64
    assert bool((gt[:, :3, :3] == torch.eye(3)).all()) and bool((gt[:, :3, 3].abs() > 0).all())
    ax = L.se3_axes()
    assert ax.shape == (32, 3) and bool((ax == 0).any()) and bool((ax < 0).any())
    # inverse(gt) @ cam keeps cam's rotation block exactly
    g = torch.matmul(torch.inverse(gt), cam)
    assert torch.equal(g[:, :3, :3], cam[:, :3, :3])
    pi_branch, taylor = L.se3_branches(gt, cam)
    assert int(pi_branch[:64].sum()) == 64 and int(pi_branch[64:].sum()) == 0      # pi and pi - 1e-4
    assert int(taylor[96:192].sum()) == 96                                          # 0, 1e-4, 5e-4
    assert int(taylor[:96].sum()) == 0 and int(taylor[192:].sum()) == 0            # near pi and 2e-3: the sine form
    tw, err = L.se3_reference(gt, cam, F32)
    assert tw.dtype == F32 and bool(torch.isfinite(tw).all()) and bool(torch.isfinite(err).all())
    assert bool((tw[:64, :3].norm(dim=1) > 3).all())                                # a rotation by ~pi came out


def test_se3_general_poses():
    gt, cam = L.se3_general()
    assert gt.shape == (32, 4, 4)
    ang = [L.se3_relative_angle(a, b) for a, b in zip(gt, cam)]
    assert min(ang) >= 0.3 and max(ang) <= 2.5
    assert not bool((gt[:, :3, :3] == torch.eye(3)).all(dim=(1, 2)).any())
    tw, err = L.se3_reference(gt, cam, F64)
    tw32, err32 = L.se3_reference(gt, cam, F32)
    assert tw.dtype == F64
    assert L.rel_err(tw32, tw) <= 0.5 * L.SE3_TWIST_RTOL
    assert bool(((err32.double() - err).abs() <= 0.5 * (L.SE3_ERR_RTOL * err.abs() + L.SE3_ERR_ATOL)).all())
    assert math.isfinite(err.sum().item())
