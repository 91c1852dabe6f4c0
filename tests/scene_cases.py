"""A numpy oracle of scene composition (include/codenerf.h, "Scene composition"): the per-sample rule
that turns K objects' raw rows at shared depths into one ray integral, in float64 with the fp32 density
sum the header states, and cn_object_rays' rule in float32 (numpy rounds every float32 operation on its
own, which is the arithmetic the header states), plus the cases the CPU and GPU tests share."""
import numpy as np

F = np.float32
EMPTY_ROW = np.array([0.0, 0.0, 0.0, -1.0e4], dtype=F)          # cn_occupancy_expand's culled slot
MAX_OBJECTS = 8


# ---------------------------------------------------------------- the composition rule


def softplus20(x):
    """torch's softplus (beta 1, threshold 20) in float64."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def widened_sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x)) * 1.002 - 0.001


def mix(raws):
    """The per-sample part of the rule.  raws (K, R, S, 4) float32 -> (sigma (R, S) float32 -- the fp32
    sum, ascending k, from 0 -- colour (R, S, 3) float64, share (K, R, S) float64, active (K, R, S))."""
    raws = np.asarray(raws, dtype=F)
    with np.errstate(invalid="ignore"):
        sigma_k = softplus20(raws[..., 3].astype(np.float64) - 1.0).astype(F)      # each object's fp32 density
        c_k = widened_sigmoid(raws[..., :3])
        sigma = np.zeros(raws.shape[1:3], dtype=F)
        for k in range(raws.shape[0]):
            sigma = (sigma + sigma_k[k]).astype(F)
        active = sigma_k != 0                                                      # a NaN is active
        count = active.sum(axis=0)
        s64 = sigma_k.astype(np.float64)
        numerator = np.where(active[..., None], s64[..., None] * c_k, 0.0).sum(axis=0)
        lone = np.where(active[..., None], c_k, 0.0).sum(axis=0)                   # the one active colour
        sig64 = sigma.astype(np.float64)
        safe = np.where(count > 1, sig64, 1.0)
        colour = np.where((count > 1)[..., None], numerator / safe[..., None],
                          np.where((count == 1)[..., None], lone, 0.0))
        share = np.where(active, np.where(count > 1, s64 / safe, 1.0), 0.0)
    return sigma, colour, share, active


def integrate(sigma, colour, share, z, rd):
    """cn_volume_render's integral of a density (R, S) and a colour (R, S, 3) in float64 -> dict of
    rgb, disp, acc, weights, depth, acc_objects (K, R).  S == 1 is the reference's sample-free ray."""
    z = np.asarray(z, dtype=np.float64)
    rd = np.asarray(rd, dtype=np.float64)
    n, s = z.shape
    if s == 1:
        nan = np.full(n, np.nan)
        return dict(rgb=np.zeros((n, 3)), disp=nan, acc=np.zeros(n), weights=np.zeros((n, 0)), depth=np.zeros(n),
                    acc_objects=np.zeros((share.shape[0], n)))
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((n, 1), 1e10)], axis=1)
    sd = sigma.astype(np.float64) * (dist * np.linalg.norm(rd, axis=-1)[:, None])
    before = np.concatenate([np.zeros((n, 1)), np.cumsum(sd[:, :-1], axis=1)], axis=1)
    w = (1.0 - np.exp(-sd)) * np.exp(-before)
    depth, acc = (w * z).sum(axis=1), w.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = depth / acc
        disp = np.where(np.isnan(q), q, 1.0 / np.maximum(1e-10, q))
    return dict(rgb=(w[..., None] * colour).sum(axis=1), disp=disp, acc=acc, weights=w, depth=depth,
                acc_objects=(w[None] * share).sum(axis=2))


def compose(raws, z, rd):
    """The whole rule: raws (K, R, S, 4), z (R, S), rd (R, 3) -> integrate()'s dict."""
    sigma, colour, share, _ = mix(raws)
    return integrate(sigma, colour, share, z, rd)


# ---------------------------------------------------------------- object rays


def object_rays(ro, rd, poses):
    """cn_object_rays in float32, every operation rounded: poses (K, 12) = R row-major (object to
    world), then t -> ro_out, rd_out (K, R, 3)."""
    ro, rd, poses = (np.asarray(a, dtype=F) for a in (ro, rd, poses))
    outs = ([], [])
    with np.errstate(invalid="ignore", over="ignore"):
        for p in poses:
            rot, t = p[:9].reshape(3, 3), p[9:]
            for out, v in zip(outs, (ro - t, rd)):
                out.append(np.stack([(v[:, 0] * rot[0, i] + v[:, 1] * rot[1, i]) + v[:, 2] * rot[2, i]
                                     for i in range(3)], axis=-1))
    return np.stack(outs[0]).astype(F), np.stack(outs[1]).astype(F)


def rotation(axis, angle):
    """Rodrigues' rotation about ``axis`` in float64, rounded to float32 (orthonormal to ~1e-7)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)).astype(F)


IDENTITY = np.eye(3, dtype=F)
FLIP = np.diag([-1.0, -1.0, 1.0]).astype(F)                     # a half turn about z: exact in every format


def pose_row(rot, t):
    return np.concatenate([np.asarray(rot, dtype=F).reshape(9), np.asarray(t, dtype=F)])


def poses(n_objects):
    """n_objects poses cycling through the identity, the half turn with a translation, and general
    rotations with translations."""
    rows = []
    for k in range(n_objects):
        if k % 3 == 0:
            rows.append(pose_row(IDENTITY if k == 0 else rotation([1, -2, 0.5 * k], 0.4 * k), [0.1 * k, 0, -0.05 * k]))
        elif k % 3 == 1:
            rows.append(pose_row(FLIP, [0.25, -0.5, 0.125 * k]))
        else:
            rows.append(pose_row(rotation([0.3, 1.0, -0.4 * k], 1.1 + k), [-0.7, 0.2 * k, 1.3]))
    return np.stack(rows)


def pose_rays(n_rays, seed):
    """Rays with -0.0 components and magnitudes near 1e4 among ordinary ones."""
    rng = np.random.default_rng(seed)
    ro = rng.standard_normal((n_rays, 3)).astype(F)
    rd = rng.standard_normal((n_rays, 3)).astype(F)
    ro[0, 0], rd[0, 1] = F(-0.0), F(-0.0)
    ro[n_rays // 2] = (F(9876.543), F(-10001.25), F(1.0e4))
    rd[n_rays - 1, 2] = F(-9999.5)
    return ro, rd


# ---------------------------------------------------------------- compose cases


def depths(n_rays, n_samples, rng):
    """z sorted in [1, 2] and rd ~ N(0, 1)."""
    z = np.sort(1.0 + rng.random((n_rays, n_samples)), axis=-1).astype(F)
    return z, rng.standard_normal((n_rays, 3)).astype(F)


def exclusive_case(n_objects, n_rays, n_samples, seed):
    """Every sample's rows are EMPTY_ROW in all objects but the one a hash of (r, s) picks, or in all of
    them; the last ray is empty throughout.  -> raws (K, R, S, 4), z, rd, selected (R, S, 4): the tensor
    holding each sample's active row (EMPTY_ROW where there is none), owner (R, S) (-1: none)."""
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((n_rays, n_samples, 4)) * 2).astype(F)
    r, s = np.meshgrid(np.arange(n_rays), np.arange(n_samples), indexing="ij")
    owner = ((r * 73856093) ^ (s * 19349663) ^ seed) % (n_objects + 1)
    owner = np.where(owner == n_objects, -1, owner)
    owner[n_rays - 1] = -1
    raws = np.broadcast_to(EMPTY_ROW, (n_objects, n_rays, n_samples, 4)).copy()
    for k in range(n_objects):
        raws[k][owner == k] = rows[owner == k]
    selected = np.where((owner >= 0)[..., None], rows, EMPTY_ROW).astype(F)
    z, rd = depths(n_rays, n_samples, rng)
    return raws, z, rd, selected, owner


def overlap_case(n_objects, n_rays, n_samples, seed):
    """Raw colours randn * 2, sigma_raw randn * 2 with about half the slots emptied."""
    rng = np.random.default_rng(seed)
    raws = (rng.standard_normal((n_objects, n_rays, n_samples, 4)) * 2).astype(F)
    raws[rng.random((n_objects, n_rays, n_samples)) < 0.5] = EMPTY_ROW
    z, rd = depths(n_rays, n_samples, rng)
    return raws, z, rd
