"""Oracles of the scene render's backward (include/codenerf.h, "Scene composition, backward"): the composition
rule in torch float64 under autograd with every sample's active set frozen, and numpy models of
cn_object_rays_backward (float64, with the magnitudes its fp32 bound needs), cn_occupancy_gather and
cn_occupancy_cull_backward (float32, every operation rounded, in the header's order), plus the upstream
gradients the CPU and GPU tests share."""
import numpy as np
import torch

import occupancy_cases as OC
import scene_cases as SC

F = np.float32
OUTPUTS = ("rgb", "disp", "acc", "weights", "depth", "acc_objects")
G_DISP_SCALE = 1e-2      # as test_gpu_grad.test_volume_render_backward weighs disp: d disp / d w grows as 1 / acc^2


# ---------------------------------------------------------------- the composition rule under autograd


def compose_torch(raws, z, rd):
    """The rule of scene_cases.mix / integrate in torch float64.  raws (K, R, S, 4), z (R, S), rd (R, 3) tensors
    (raws and rd may require grad) -> dict of OUTPUTS.  An object is active where its fp32 density is not 0
    (scene_cases.mix's test, on the detached values); the masks enter through torch.where, so the active sets
    and counts are constants of the derivative."""
    raws, z, rd = raws.double(), z.double(), rd.double()
    k, n, s = raws.shape[:3]
    active = torch.from_numpy(SC.mix(raws.detach().float().numpy())[3])
    count = active.sum(dim=0)
    many, one = count > 1, count == 1
    sigma_k = torch.nn.functional.softplus(raws[..., 3] - 1.0, beta=1.0, threshold=20.0)
    c_k = torch.sigmoid(raws[..., :3]) * 1.002 - 0.001
    zero = torch.zeros((), dtype=torch.float64)
    s_act = torch.where(active, sigma_k, zero)
    sigma = s_act.sum(dim=0)
    safe = torch.where(many, sigma, torch.ones_like(sigma))
    numerator = torch.where(active[..., None], sigma_k[..., None] * c_k, zero).sum(dim=0)
    lone = torch.where(active[..., None], c_k, zero).sum(dim=0)
    colour = torch.where(many[..., None], numerator / safe[..., None], torch.where(one[..., None], lone, zero))
    share = torch.where(active, torch.where(many, sigma_k / safe, torch.ones_like(sigma_k)), zero)
    if s == 1:      # the reference's sample-free ray: nothing depends on the inputs
        return dict(rgb=torch.zeros(n, 3, dtype=torch.float64), disp=torch.full((n,), float("nan"), dtype=torch.float64),
                    acc=torch.zeros(n, dtype=torch.float64), weights=torch.zeros(n, 0, dtype=torch.float64),
                    depth=torch.zeros(n, dtype=torch.float64), acc_objects=torch.zeros(k, n, dtype=torch.float64))
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((n, 1), 1e10, dtype=torch.float64)], dim=1)
    sd = sigma * (dist * torch.linalg.vector_norm(rd, dim=-1)[:, None])
    before = torch.cat([torch.zeros(n, 1, dtype=torch.float64), torch.cumsum(sd[:, :-1], dim=1)], dim=1)
    w = (1.0 - torch.exp(-sd)) * torch.exp(-before)
    depth, acc = (w * z).sum(dim=1), w.sum(dim=1)
    # disp = 1 / max(1e-10, depth / acc), NaN where acc == 0 -- written so that such a ray's NaN is a constant
    # (0 / 0 under autograd would send NaN into every gradient of the ray, where the kernels route nothing)
    seen = acc.detach() != 0
    q = depth / torch.where(seen, acc, torch.ones_like(acc))
    disp = torch.where(seen, 1.0 / torch.max(torch.full_like(q, 1e-10), q), torch.full_like(q, float("nan")))
    return dict(rgb=(w[..., None] * colour).sum(dim=1), disp=disp, acc=acc, weights=w, depth=depth,
                acc_objects=(w[None] * share).sum(dim=2))


def upstream(n_objects, n_rays, n_samples, seed):
    """Random upstream gradients of the six outputs, float32 (g_disp scaled by G_DISP_SCALE)."""
    rng = np.random.default_rng(seed)
    g = dict(rgb=rng.standard_normal((n_rays, 3)), disp=G_DISP_SCALE * rng.standard_normal(n_rays),
             acc=rng.standard_normal(n_rays), weights=rng.standard_normal((n_rays, n_samples)),
             depth=rng.standard_normal(n_rays), acc_objects=rng.standard_normal((n_objects, n_rays)))
    return {key: v.astype(F) for key, v in g.items()}


def compose_loss(out, g, without=()):
    """sum over the outputs of <output, its upstream gradient>; a ray's NaN disp (acc == 0) is left out, as the
    kernel routes no gradient through it."""
    total = 0.0
    for key in OUTPUTS:
        if key in without or out[key].numel() == 0:
            continue
        v, gk = out[key], torch.as_tensor(g[key]).to(out[key].dtype).to(out[key].device)
        if key == "disp":
            fin = torch.isfinite(v.detach())
            v, gk = v[fin], gk[fin]
        total = total + (v * gk).sum()
    return total


def compose_gradients(raws, z, rd, g, without=()):
    """d raws (K, R, S, 4) and d rd (R, 3) of compose_loss under the float64 rule, as numpy float64."""
    raws_t = torch.from_numpy(np.asarray(raws, dtype=F)).double().requires_grad_(True)
    rd_t = torch.from_numpy(np.asarray(rd, dtype=F)).double().requires_grad_(True)
    loss = compose_loss(compose_torch(raws_t, torch.from_numpy(np.asarray(z, dtype=F)), rd_t), g, without)
    if not isinstance(loss, torch.Tensor) or not loss.requires_grad:
        return np.zeros(raws_t.shape), np.zeros(rd_t.shape)
    loss.backward()
    none = torch.zeros(())
    return ((raws_t.grad if raws_t.grad is not None else none.expand(raws_t.shape)).numpy(),
            (rd_t.grad if rd_t.grad is not None else none.expand(rd_t.shape)).numpy())


# ---------------------------------------------------------------- cn_object_rays_backward


def object_rays_backward(g_ro, g_rd, ro, rd, poses):
    """The rule in float64 from float32 inputs.  g_ro, g_rd (K, R, 3) or None; poses (K, 12) ->
    dict(d_ro, d_rd (R, 3), d_poses (K, 12)) and, for the fp32 bound of a sum computed in any order,
    ``abs_*``: the sums of the terms' magnitudes, and ``terms_*``: the number of products summed per element."""
    ro, rd, poses = (np.asarray(a, dtype=F).astype(np.float64) for a in (ro, rd, poses))
    k, n = poses.shape[0], ro.shape[0]
    g_ro = np.zeros((k, n, 3)) if g_ro is None else np.asarray(g_ro, dtype=F).astype(np.float64)
    g_rd = np.zeros((k, n, 3)) if g_rd is None else np.asarray(g_rd, dtype=F).astype(np.float64)
    rot, t = poses[:, :9].reshape(k, 3, 3), poses[:, 9:]
    out = {}
    for name, g in (("d_ro", g_ro), ("d_rd", g_rd)):
        out[name] = np.einsum("kji,kri->rj", rot, g)
        out["abs_" + name] = np.einsum("kji,kri->rj", np.abs(rot), np.abs(g))
    d = ro[None] - t[:, None, :]                                     # (K, R, 3)
    d_rot = np.einsum("krj,kri->kji", d, g_ro) + np.einsum("rj,kri->kji", rd, g_rd)
    a_rot = np.einsum("krj,kri->kji", np.abs(d), np.abs(g_ro)) + np.einsum("rj,kri->kji", np.abs(rd), np.abs(g_rd))
    d_t = -np.einsum("kji,kri->kj", rot, g_ro)
    a_t = np.einsum("kji,kri->kj", np.abs(rot), np.abs(g_ro))
    out["d_poses"] = np.concatenate([d_rot.reshape(k, 9), d_t], axis=1)
    out["abs_d_poses"] = np.concatenate([a_rot.reshape(k, 9), a_t], axis=1)
    out["terms_d_ro"] = out["terms_d_rd"] = 3 * k
    out["terms_d_poses"] = np.concatenate([np.full((k, 9), 2 * n), np.full((k, 3), 3 * n)], axis=1)
    return out


# ---------------------------------------------------------------- the compact rows


def gather(g_raw, keep):
    """cn_occupancy_gather: the kept samples' rows of g_raw (R, S, 4), ascending sample order -> (M', 4)."""
    return np.asarray(g_raw, dtype=F).reshape(-1, 4)[np.asarray(keep).reshape(-1)]


def cull_backward(g_pts, g_vdir, z, keep, chunk_rows):
    """cn_occupancy_cull_backward in float32, every operation rounded, every sum sequential in the header's
    order.  g_pts, g_vdir (M', 3) or None, z (R, S), keep (R, S) bool -> d_ro, d_rd (R, 3) float32."""
    z, keep = np.asarray(z, dtype=F), np.asarray(keep, dtype=bool)
    n, s = z.shape
    row = np.cumsum(keep.reshape(-1)) - 1                            # a kept sample's compact row
    m = int(keep.sum())
    g_pts = np.zeros((m, 3), dtype=F) if g_pts is None else np.asarray(g_pts, dtype=F)
    g_vdir = np.zeros((m, 3), dtype=F) if g_vdir is None else np.asarray(g_vdir, dtype=F)
    d_ro, p, v = (np.zeros((n, 3), dtype=F) for _ in range(3))
    for r in range(n):
        for k in np.nonzero(keep[r])[0]:
            g = g_pts[row[r * s + k]]
            d_ro[r] = d_ro[r] + g                                     # float32 + float32: one rounding
            p[r] = p[r] + z[r, k] * g
        base = (r // chunk_rows) * chunk_rows
        rcnt = min(chunk_rows, n - base)
        for i in range(s):
            kk = (r - base) + i * rcnt
            rr, ss = base + kk // s, kk % s
            if keep[rr, ss]:
                v[r] = v[r] + g_vdir[row[rr * s + ss]]
    return d_ro, (p + v).astype(F)


def cull_case(kind, n_rays, n_samples, seed, g=32):
    """Rays against one of occupancy_cases' grids ("sphere", "empty", "full") -> ro, rd, z, bits, keep."""
    ro, rd, z = OC.random_rays(n_rays, n_samples, seed)
    bits = OC.grid_bits(kind, g, bound=1.0, radius=0.6)
    keep = OC.lookup(OC.ray_points(ro, rd, z), bits, g, 1.0)
    return ro, rd, z, bits, keep
