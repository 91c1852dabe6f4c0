"""The weight-culling rule (include/codenerf.h, "Weight-bounded colour culling") as the numpy model of
tests/weight_cull_cases.py states it: the dropped weight stays within the tolerance, ties at both
thresholds are kept, NaN and zero rows, S = 1 -- and the render scene the GPU tests use sits where
they need it (part of the samples kept, no tail near the threshold), computed with the CPU oracle."""
import os
import struct

import numpy as np
import pytest
import torch

import occupancy_cases as OC
import weight_cull_cases as WC
from conftest import GOLDEN

F = np.float32


# ---------------------------------------------------------------- thresholds


@pytest.mark.parametrize("tol", [1e-3, 1e-2, 3e-5, 0.5, 1.0, 2.0 ** -10])
@pytest.mark.parametrize("s", [1, 2, 3, 64, 128, 160, 512])
def test_thresholds(tol, s):
    """eps_weight is the largest float32 <= tol / (2 S) (so S of them sum to <= tol / 2), and the
    package's own helper agrees with the model's bit for bit."""
    from codenerf import ops
    ew, et = WC.thresholds(tol, s)
    assert ew.dtype == F and et == tol / 2.0
    assert float(ew) <= tol / (2.0 * s) < float(np.nextafter(ew, F(np.inf)))
    pw, pt = ops.weight_cull_thresholds(tol, s)
    assert struct.pack("<f", pw) == ew.tobytes() and pt == et
    assert ops.weight_cull_thresholds(0.0, s) == (0.0, 0.0)


# ---------------------------------------------------------------- the bound


def _render_like_rows(r, s, seed):
    """Weights of random densities: alpha_i prod (1 - alpha_k), in float32 -- sums to <= 1 per ray."""
    rng = np.random.default_rng(seed)
    alpha = (rng.random((r, s)) ** rng.uniform(1.0, 8.0, size=(r, 1))).astype(F)
    alpha[rng.random((r, s)) < 0.2] = 0.0
    trans = np.cumprod(np.concatenate([np.ones((r, 1), F), (F(1) - alpha)[:, :-1]], axis=-1), axis=-1, dtype=F)
    return (alpha * trans).astype(F)


@pytest.mark.parametrize("tol", [1e-3, 1e-2, 3e-5, 0.25])
@pytest.mark.parametrize("s", [1, 3, 64, 65, 128, 160, 512])
def test_dropped_weight_within_tolerance(tol, s):
    ew, et = WC.thresholds(tol, s)
    for w in (_render_like_rows(200, s, seed=s), WC.adversarial_weights(s)(tol)):
        keep = WC.keep_mask(w, ew, et)
        dropped = WC.dropped_weight(w, keep)
        assert dropped.max() <= tol, (dropped.max(), tol)
        # its two parts, as the header argues them: the culled tail, and the others below eps_weight
        t = WC.tails(w)
        in_tail = t < et
        assert np.where(in_tail, w.astype(np.float64), 0.0).sum(axis=-1).max() < tol / 2.0 or et == 0
        assert np.where(~in_tail & ~keep, w.astype(np.float64), 0.0).sum(axis=-1).max() <= tol / 2.0
    w = WC.adversarial_weights(s)(tol)
    assert WC.dropped_weight(w, WC.keep_mask(w, ew, et)).max() > 0.3 * tol or s == 1      # the rows do press on it


def test_zero_tolerance_keeps_every_positive_weight():
    w = _render_like_rows(50, 64, seed=1)
    keep = WC.keep_mask(w, 0.0, 0.0)
    assert np.array_equal(keep, w > 0) and (~keep).any() and keep.any()
    assert WC.dropped_weight(w, keep).max() == 0.0


# ---------------------------------------------------------------- ties, NaN, zero rows, S = 1


def test_dyadic_ties():
    ew, et = F(2.0 ** -12), 2.0 ** -7
    d = WC.DYADIC
    #          w == eps_weight    just below     zero   big            tail == eps_tail
    w = np.array([[2.0 ** -12, 2.0 ** -12 - d, 0.0, 0.25, 2.0 ** -8, 2.0 ** -8]], dtype=F)
    assert np.array_equal(WC.keep_mask(w, ew, et)[0], [True, False, False, True, True, False])
    # the last sample alone is below eps_tail (2^-8); the pair before it sums to exactly eps_tail: kept
    w2 = np.array([[0.5, 2.0 ** -7 - d]], dtype=F)
    assert np.array_equal(WC.keep_mask(w2, ew, et)[0], [True, False])
    w3 = np.array([[0.5, 2.0 ** -7]], dtype=F)
    assert np.array_equal(WC.keep_mask(w3, ew, et)[0], [True, True])
    # every order of a dyadic row's additions gives the same tails
    row = WC.dyadic_weights(8, 192, seed=3)[5:]
    rev = np.cumsum(row.astype(np.float64)[:, ::-1], axis=-1)[:, ::-1]
    fwd = row.astype(np.float64).sum(axis=-1, keepdims=True) - np.cumsum(row.astype(np.float64), axis=-1) + row
    assert np.array_equal(rev, fwd)


def test_nan_and_zero_rows():
    ew, et = F(2.0 ** -12), 2.0 ** -7
    w = np.array([[0.25, np.nan, 0.25, 0.125], [0.0, 0.0, 0.0, 0.0], [np.nan] * 4, [0.5, 0.0, 0.25, 0.0]], dtype=F)
    keep = WC.keep_mask(w, ew, et)
    assert np.array_equal(keep, [[False, False, True, True], [False] * 4, [False] * 4, [True, False, True, False]])
    assert np.array_equal(WC.keep_mask(w, 0.0, 0.0), keep)      # NaN and 0 fall out at tolerance 0 too
    assert WC.band_count(w, et) == 0


def test_single_sample_rays():
    ew, et = WC.thresholds(1e-3, 1)
    w = np.array([[1.0], [0.0], [4e-4], [6e-4], [np.nan]], dtype=F)
    assert np.array_equal(WC.keep_mask(w, ew, et)[:, 0], [True, False, False, True, False])
    ro, rd, z = OC.random_rays(5, 1, seed=0)
    out = WC.cull(w, ro, rd, z, 2, np.array([4, 3, 2, 1, 0]), ew, et)
    assert out["count"] == 2 and out["sample_index"].tolist() == [0, 3] and out["code_out"].tolist() == [4, 1]
    assert np.array_equal(out["vdir"], rd[[0, 3]])              # S = 1: each sample's own ray (Q1 is the identity)


def test_shared_rows_cover_the_branches():
    """The rows the GPU tests run hold each special case where the shape has room for it."""
    w = WC.dyadic_weights(37, 64, seed=0)
    keep = WC.keep_mask(w, WC.EPS_WEIGHT, WC.EPS_TAIL)
    assert not keep[0].any() and keep[1].all()
    assert np.isnan(w[2, 32]) and not keep[2, :33].any()
    assert keep[3, 0] and not keep[3, 1] and keep[3, -1] and w[3, 0] == WC.EPS_WEIGHT and w[3, -1] == F(WC.EPS_TAIL)
    assert not keep[4].any() and w[4, -1] > 0
    assert 0.1 < keep[5:].mean() < 0.9
    out = WC.cull(w, *OC.random_rays(37, 64, seed=1), 16, None, WC.EPS_WEIGHT, WC.EPS_TAIL)
    assert out["count"] == int(keep.sum()) and np.all(np.diff(out["sample_index"]) > 0)


# ---------------------------------------------------------------- the render scene


def _oracle_fine_weights(nc, nf, sigma_bias):
    """The GPU render tests' scene on the CPU oracle -> the fine pass's weights (1024, nc + nf): 32 x 32
    rays of the render_small.npz pose, coarse model seed 0, fine model seed 1 with fc_out.bias[0]
    (sigma_raw's bias) raised by ``sigma_bias``.  Densities do not depend on the chunking (Q1 touches
    view directions only), so the rays go through in slices of any size."""
    from codenerf import synthetic
    from oracle import codenerf_oracle as O
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "render_small.npz")).items()}
    k = torch.tensor([[28.0, 0, 16.0, 0], [0, 28.0, 16.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    ro, rd = O.ray_bundle(O.ray_directions(32, 32, k), g["pose"].reshape(-1, 4, 4)[:1])
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    pc, pf = synthetic.codenerf_params(0), dict(synthetic.codenerf_params(1))
    pf["fc_out.bias"] = pf["fc_out.bias"].clone()
    pf["fc_out.bias"][0] += sigma_bias
    smp, emb = O.Sampling(nc, nf, 0.8, 1.8), O.EmbedCfg()
    out = []
    with torch.no_grad():
        for a in range(0, ro.shape[0], 256):
            o, d = ro[a:a + 256], rd[a:a + 256]
            zs, zt = g["z_s"].expand(o.shape[0], -1), g["z_t"].expand(o.shape[0], -1)
            pts, z = O.sample_uniform(o, d, smp.bins)
            w_c = O.volume_render(O.forward_pass(pc, emb, d, pts, zs, zt), z, d)[3]
            pts_f, z_f = O.sample_pdf(o, d, w_c[..., 1:-1], z, nf)
            out.append(O.volume_render(O.forward_pass(pf, emb, d, pts_f, zs, zt), z_f, d)[3])
    return torch.cat(out).numpy()


@pytest.mark.parametrize("nc,nf,expect", [(64, 64, 0.297), (32, 128, 0.338)])
def test_render_scene_kept_range(nc, nf, expect):
    """At tol = 1e-3 the scene keeps a part of every ray -- about 0.30 / 0.34 of the fine samples -- the
    dropped weight per ray is about tol / 2, and no tail sits near eps_tail, so the device's own
    summation order decides nothing (the GPU tests assert the same on the device's weights)."""
    tol = 1e-3
    w = _oracle_fine_weights(nc, nf, 60.0)
    ew, et = WC.thresholds(tol, nc + nf)
    keep = WC.keep_mask(w, ew, et)
    kept = keep.mean()
    print(f"kept {kept:.4f}  max dropped {WC.dropped_weight(w, keep).max():.3e}")
    assert 0.1 < kept < 0.8
    assert abs(kept - expect) < 0.03
    per_ray = keep.sum(axis=-1)
    assert per_ray.min() > 0 and per_ray.max() < nc + nf         # no ray fully culled or fully kept
    assert WC.dropped_weight(w, keep).max() <= tol
    assert WC.band_count(w, et) == 0
