"""Oracles of the scene render with uniform scale (include/codenerf.h, "Scene composition with uniform scale"):
cn_object_rays_scaled in float32 numpy (every operation rounded), the composition rule with each object's
density divided by its scale (the fp32 densities the header states, the rest in float64), the same rule in torch
float64 under autograd with frozen active sets and the scales as a differentiable tensor, and a float64 model of
cn_object_rays_scaled_backward with the magnitudes its fp32 bound needs; plus the cases the CPU and GPU tests
share."""
import numpy as np
import torch

import scene_cases as SC
import scene_grad_cases as GC

F = np.float32
SCALES = (0.5, 1.0, 2.0, 0.37, 3.1)              # two exact binary factors, one, and two ordinary values
S_LIST = (2, 17, 64, 65, 129, 300)               # all four <K, L> instances and their ragged runs
K_LIST = (1, 2, 3, 8)                            # all NOBJ
RAYS = 53


def scales_for(n_objects, seed):
    """One scale per object drawn from SCALES; the first object's is never 1, so every case is a scaled one."""
    rng = np.random.default_rng(seed)
    s = rng.choice(np.asarray(SCALES, dtype=F), size=n_objects)
    if s[0] == 1.0:
        s[0] = F(0.37)
    return s.astype(F)


def similarity_poses(n_objects, seed):
    """scene_cases.poses with a 13th column from scales_for."""
    return np.concatenate([SC.poses(n_objects), scales_for(n_objects, seed)[:, None]], axis=1).astype(F)


# ---------------------------------------------------------------- object rays


def object_rays(ro, rd, poses):
    """cn_object_rays_scaled in float32: scene_cases.object_rays for (R, t), then one rounded division by s.
    poses (K, 13) -> ro_out, rd_out (K, R, 3)."""
    poses = np.asarray(poses, dtype=F)
    assert poses.shape[1] == 13
    uo, uv = SC.object_rays(ro, rd, poses[:, :12])
    with np.errstate(invalid="ignore", over="ignore"):
        s = poses[:, 12][:, None, None]
        return (uo / s).astype(F), (uv / s).astype(F)


# ---------------------------------------------------------------- the composition rule


def densities(raws, scales):
    """sigma_k = softplus20(xs - 1) / s_k: the fp32 density, then the division rounded in fp32 -> (K, R, S)."""
    raws, scales = np.asarray(raws, dtype=F), np.asarray(scales, dtype=F)
    with np.errstate(invalid="ignore"):
        sigma = SC.softplus20(raws[..., 3].astype(np.float64) - 1.0).astype(F)
        return (sigma / scales[:, None, None]).astype(F)


def mix(raws, scales):
    """scene_cases.mix on the scaled densities -> (sigma (R, S) float32, colour (R, S, 3), share (K, R, S), active)."""
    raws = np.asarray(raws, dtype=F)
    sigma_k = densities(raws, scales)
    with np.errstate(invalid="ignore"):
        c_k = SC.widened_sigmoid(raws[..., :3])
        sigma = np.zeros(raws.shape[1:3], dtype=F)
        for k in range(raws.shape[0]):
            sigma = (sigma + sigma_k[k]).astype(F)
        active = sigma_k != 0
        count = active.sum(axis=0)
        s64 = sigma_k.astype(np.float64)
        numerator = np.where(active[..., None], s64[..., None] * c_k, 0.0).sum(axis=0)
        lone = np.where(active[..., None], c_k, 0.0).sum(axis=0)
        sig64 = sigma.astype(np.float64)
        safe = np.where(count > 1, sig64, 1.0)
        colour = np.where((count > 1)[..., None], numerator / safe[..., None],
                          np.where((count == 1)[..., None], lone, 0.0))
        share = np.where(active, np.where(count > 1, s64 / safe, 1.0), 0.0)
    return sigma, colour, share, active


def compose(raws, scales, z, rd):
    """The whole rule -> scene_cases.integrate's dict."""
    sigma, colour, share, _ = mix(raws, scales)
    return SC.integrate(sigma, colour, share, z, rd)


# ---------------------------------------------------------------- the rule under autograd


def compose_torch(raws, scales, z, rd, keep=None):
    """scene_grad_cases.compose_torch with sigma_k = softplus(xs - 1) / s_k, the active sets those of mix() (fp32
    test on the detached values), frozen.  ``scales`` (K,) may require grad.  ``keep``: a dict that receives
    "sigma_k" (K, R, S), the scaled densities with their gradient retained."""
    raws, z, rd, scales = raws.double(), z.double(), rd.double(), scales.double()
    k, n, s = raws.shape[:3]
    active = torch.from_numpy(mix(raws.detach().float().numpy(), scales.detach().float().numpy())[3])
    count = active.sum(dim=0)
    many, one = count > 1, count == 1
    sigma_k = torch.nn.functional.softplus(raws[..., 3] - 1.0, beta=1.0, threshold=20.0) / scales[:, None, None]
    if keep is not None:
        if sigma_k.requires_grad:
            sigma_k.retain_grad()
        keep["sigma_k"] = sigma_k
    c_k = torch.sigmoid(raws[..., :3]) * 1.002 - 0.001
    zero = torch.zeros((), dtype=torch.float64)
    s_act = torch.where(active, sigma_k, zero)
    sigma = s_act.sum(dim=0)
    safe = torch.where(many, sigma, torch.ones_like(sigma))
    numerator = torch.where(active[..., None], sigma_k[..., None] * c_k, zero).sum(dim=0)
    lone = torch.where(active[..., None], c_k, zero).sum(dim=0)
    colour = torch.where(many[..., None], numerator / safe[..., None], torch.where(one[..., None], lone, zero))
    share = torch.where(active, torch.where(many, sigma_k / safe, torch.ones_like(sigma_k)), zero)
    if s == 1:
        return dict(rgb=torch.zeros(n, 3, dtype=torch.float64), disp=torch.full((n,), float("nan"), dtype=torch.float64),
                    acc=torch.zeros(n, dtype=torch.float64), weights=torch.zeros(n, 0, dtype=torch.float64),
                    depth=torch.zeros(n, dtype=torch.float64), acc_objects=torch.zeros(k, n, dtype=torch.float64))
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((n, 1), 1e10, dtype=torch.float64)], dim=1)
    sd = sigma * (dist * torch.linalg.vector_norm(rd, dim=-1)[:, None])
    before = torch.cat([torch.zeros(n, 1, dtype=torch.float64), torch.cumsum(sd[:, :-1], dim=1)], dim=1)
    w = (1.0 - torch.exp(-sd)) * torch.exp(-before)
    depth, acc = (w * z).sum(dim=1), w.sum(dim=1)
    seen = acc.detach() != 0                      # see scene_grad_cases.compose_torch: a NaN disp is a constant
    q = depth / torch.where(seen, acc, torch.ones_like(acc))
    disp = torch.where(seen, 1.0 / torch.max(torch.full_like(q, 1e-10), q), torch.full_like(q, float("nan")))
    return dict(rgb=(w[..., None] * colour).sum(dim=1), disp=disp, acc=acc, weights=w, depth=depth,
                acc_objects=(w[None] * share).sum(dim=2))


def compose_gradients(raws, scales, z, rd, g, without=()):
    """d raws (K, R, S, 4), d rd (R, 3) and d scales (K,) of scene_grad_cases.compose_loss under the float64 rule,
    as numpy float64, and what d_scales' bound needs, per object: ``max_d_sigma`` = max |d sigma_k|,
    ``sum_sigma`` = sum sigma_k / s_k, ``terms`` = the number of active slots, ``abs_terms`` = sum |d sigma_k
    sigma_k / s_k|."""
    raws_t = torch.from_numpy(np.asarray(raws, dtype=F)).double().requires_grad_(True)
    rd_t = torch.from_numpy(np.asarray(rd, dtype=F)).double().requires_grad_(True)
    sc_t = torch.from_numpy(np.asarray(scales, dtype=F)).double().requires_grad_(True)
    keep = {}
    out = compose_torch(raws_t, sc_t, torch.from_numpy(np.asarray(z, dtype=F)), rd_t, keep)
    loss = GC.compose_loss(out, g, without)
    k = raws_t.shape[0]
    zeros = dict(max_d_sigma=np.zeros(k), sum_sigma=np.zeros(k), terms=np.zeros(k), abs_terms=np.zeros(k))
    if not isinstance(loss, torch.Tensor) or not loss.requires_grad:
        return np.zeros(raws_t.shape), np.zeros(rd_t.shape), np.zeros(k), zeros
    loss.backward()

    def grad(t):
        return (t.grad if t.grad is not None else torch.zeros(t.shape, dtype=torch.float64)).numpy()

    sigma_k = keep["sigma_k"].detach().numpy()
    d_sigma = grad(keep["sigma_k"])
    active = mix(raws, scales)[3]
    d_sigma = np.where(active, d_sigma, 0.0)
    s = np.asarray(scales, dtype=np.float64)[:, None, None]
    terms = d_sigma * np.where(active, sigma_k, 0.0) / s
    model = dict(max_d_sigma=np.abs(d_sigma).max(axis=(1, 2)), sum_sigma=(np.where(active, sigma_k, 0.0) / s).sum(axis=(1, 2)),
                 terms=active.sum(axis=(1, 2)).astype(np.float64), abs_terms=np.abs(terms).sum(axis=(1, 2)),
                 d_scales_from_terms=-terms.sum(axis=(1, 2)))
    return grad(raws_t), grad(rd_t), grad(sc_t), model


def d_scales_bound(model, rtol):
    """|d_scales[k] - exact| <= rtol max|d sigma_k| sum sigma_k / s_k + (n_terms + 4) 2^-24 sum |term|: the
    per-term error the d_raws bound allows (rtol of the largest gradient), summed, plus an fp32 sum of n_terms
    terms in any order with the roundings of each term's product and division."""
    return rtol * model["max_d_sigma"] * model["sum_sigma"] + (model["terms"] + 4) * 2.0 ** -24 * model["abs_terms"]


# ---------------------------------------------------------------- cn_object_rays_scaled_backward


def object_rays_backward(g_ro, g_rd, ro, rd, poses):
    """scene_grad_cases.object_rays_backward for similarity poses (K, 13), in float64 from float32 inputs:
    g' = g / s, the rigid formulas on g', and ds_k = - sum_r sum_i (ro_out g_ro + rd_out g_rd) / s_k.  d_poses,
    abs_d_poses and terms_d_poses have 13 columns; terms_d_ro / terms_d_rd count one more rounding per term, the
    division."""
    ro, rd, poses = (np.asarray(a, dtype=F).astype(np.float64) for a in (ro, rd, poses))
    k, n = poses.shape[0], ro.shape[0]
    g_ro = np.zeros((k, n, 3)) if g_ro is None else np.asarray(g_ro, dtype=F).astype(np.float64)
    g_rd = np.zeros((k, n, 3)) if g_rd is None else np.asarray(g_rd, dtype=F).astype(np.float64)
    rot, t, s = poses[:, :9].reshape(k, 3, 3), poses[:, 9:12], poses[:, 12]
    go, gv = g_ro / s[:, None, None], g_rd / s[:, None, None]
    out = {}
    for name, g in (("d_ro", go), ("d_rd", gv)):
        out[name] = np.einsum("kji,kri->rj", rot, g)
        out["abs_" + name] = np.einsum("kji,kri->rj", np.abs(rot), np.abs(g))
    d = ro[None] - t[:, None, :]                                     # (K, R, 3)
    d_rot = np.einsum("krj,kri->kji", d, go) + np.einsum("rj,kri->kji", rd, gv)
    a_rot = np.einsum("krj,kri->kji", np.abs(d), np.abs(go)) + np.einsum("rj,kri->kji", np.abs(rd), np.abs(gv))
    d_t = -np.einsum("kji,kri->kj", rot, go)
    a_t = np.einsum("kji,kri->kj", np.abs(rot), np.abs(go))
    # ds: ro_out = R^T d / s, rd_out = R^T rd / s; 18 elementary products per ray
    ro_out = np.einsum("krj,kji->kri", d, rot) / s[:, None, None]
    rd_out = np.einsum("rj,kji->kri", rd, rot) / s[:, None, None]
    d_s = -((ro_out * g_ro).sum(axis=(1, 2)) + (rd_out * g_rd).sum(axis=(1, 2))) / s
    a_ro = np.einsum("krj,kji->kri", np.abs(d), np.abs(rot)) / s[:, None, None]
    a_rd = np.einsum("rj,kji->kri", np.abs(rd), np.abs(rot)) / s[:, None, None]
    a_s = ((a_ro * np.abs(g_ro)).sum(axis=(1, 2)) + (a_rd * np.abs(g_rd)).sum(axis=(1, 2))) / s
    out["d_poses"] = np.concatenate([d_rot.reshape(k, 9), d_t, d_s[:, None]], axis=1)
    out["abs_d_poses"] = np.concatenate([a_rot.reshape(k, 9), a_t, a_s[:, None]], axis=1)
    out["terms_d_ro"] = out["terms_d_rd"] = 3 * k + 1
    out["terms_d_poses"] = np.concatenate([np.full((k, 9), 2 * n), np.full((k, 3), 3 * n), np.full((k, 1), 18 * n)],
                                          axis=1)
    return out
