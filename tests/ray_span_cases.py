"""A numpy float32 statement of the per-ray depth spans (include/codenerf.h, "Per-ray depth spans"), built on
occupancy_cases' point lookup, plus the cases the CPU and GPU tests share.  numpy rounds every float32
operation on its own, which is the arithmetic the header states; every device result equals this file's bit
for bit."""
import numpy as np

import occupancy_cases as C

F = np.float32
TAU_MAX = np.nextafter(F(1), F(0))            # the largest float below 1


class Grid:
    """One object's grid as the rule reads it: the bit words, G and the cube's half-width."""

    def __init__(self, bits, g, bound=1.0):
        self.bits, self.g, self.bound = np.asarray(bits), int(g), float(bound)

    @classmethod
    def of(cls, kind, g=32, bound=1.0, radius=0.5):
        return cls(C.grid_bits(kind, g, bound, radius), g, bound)


# ---------------------------------------------------------------- the rule


def probe_depths(near, far, n_probes):
    """d_j = near + float(j) step, step = (far - near) / float(P - 1); d_{P-1} = far exactly -> (P,)."""
    near, far = F(near), F(far)
    step = (far - near) / F(n_probes - 1)
    d = near + np.arange(n_probes).astype(F) * step
    d[n_probes - 1] = far
    return d.astype(F)


def probe_mask(ro, rd, grids, near, far, n_probes):
    """(R, P) bool: probe j of ray r occupied in some object's grid.  ro, rd (K, R, 3) or (R, 3) for one grid."""
    ro, rd = np.asarray(ro, dtype=F), np.asarray(rd, dtype=F)
    if isinstance(grids, Grid):
        grids, ro, rd = [grids], ro[None], rd[None]
    assert ro.shape == rd.shape and ro.shape[0] == len(grids)
    d = np.tile(probe_depths(near, far, n_probes)[None, :], (ro.shape[1], 1))
    occ = np.zeros(d.shape, dtype=bool)
    for k, grid in enumerate(grids):
        occ |= C.lookup(C.ray_points(ro[k], rd[k], d), grid.bits, grid.g, grid.bound)
    return occ


def span_of_mask(occ, near, far):
    """(R, P) probe mask -> probe_range (R, 2) int32 (first, last; -1, -1 for a miss) and span (R, 2) float32
    (t_lo, t_hi) = (d_a, d_b), a = max(first - 1, 0), b = min(last + 1, P - 1); a miss keeps (near, far)."""
    n_probes = occ.shape[1]
    d = probe_depths(near, far, n_probes)
    hit = occ.any(axis=1)
    first = np.where(hit, occ.argmax(axis=1), -1)
    last = np.where(hit, n_probes - 1 - occ[:, ::-1].argmax(axis=1), -1)
    a = np.where(hit, np.maximum(first - 1, 0), 0)
    b = np.where(hit, np.minimum(last + 1, n_probes - 1), n_probes - 1)
    return np.stack([first, last], axis=1).astype(np.int32), np.stack([d[a], d[b]], axis=1).astype(F)


def span_depths(span, nc, t_rand=None):
    """z_i = min(t_lo + (float(i) + tau_i) w, t_hi), w = (t_hi - t_lo) / float(Nc - 1), for i <= Nc - 2;
    z_{Nc-1} = t_hi -> (R, Nc).  t_rand (R, Nc): columns 0 .. Nc - 2 are used."""
    t_lo, t_hi = span[:, :1].astype(F), span[:, 1:].astype(F)
    w = (t_hi - t_lo) / F(nc - 1)
    i = np.arange(nc).astype(F)[None, :]
    tau = np.zeros((span.shape[0], nc), dtype=F) if t_rand is None else np.asarray(t_rand, dtype=F)
    z = np.minimum(t_lo + (i + tau) * w, t_hi).astype(F)
    z[:, nc - 1] = t_hi[:, 0]
    return z


def sample_span(ro, rd, grids, near, far, n_probes, nc, t_rand=None):
    """cn_sample_span's outputs -> z (R, Nc), span (R, 2), probe_range (R, 2)."""
    probe_range, span = span_of_mask(probe_mask(ro, rd, grids, near, far, n_probes), near, far)
    return span_depths(span, nc, t_rand), span, probe_range


# ---------------------------------------------------------------- shared cases


def pose_rows(angle, axis, t):
    """A rigid pose as 12 floats (rotation row-major, then translation): ``angle`` about coordinate ``axis``."""
    c, s = np.cos(angle), np.sin(angle)
    rot = np.eye(3)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    rot[i, i], rot[i, j], rot[j, i], rot[j, j] = c, -s, s, c
    return [float(F(v)) for v in rot.reshape(-1)] + [float(F(v)) for v in t]


def object_rays(ro, rd, pose):
    """cn_object_rays' rule for one pose in fp32: d = ro - t; out_i = (d_0 R_0i + d_1 R_1i) + d_2 R_2i."""
    rot = np.asarray(pose[:9], dtype=F).reshape(3, 3)
    t = np.asarray(pose[9:], dtype=F)

    def into(v):
        return ((v[:, 0:1] * rot[0][None, :] + v[:, 1:2] * rot[1][None, :]) + v[:, 2:3] * rot[2][None, :]).astype(F)
    return into(np.asarray(ro, dtype=F) - t[None, :]), into(np.asarray(rd, dtype=F))


def camera_rays(n_rays, seed, distance=1.3, spread=0.45):
    """Unit-ish rays from points at ``distance`` from the origin towards it, jittered: most cross the unit
    cube's middle, some miss a radius-0.5 sphere."""
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((n_rays, 3))
    o = distance * o / np.linalg.norm(o, axis=1, keepdims=True)
    target = rng.uniform(-spread, spread, (n_rays, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F), d.astype(F)


def pinhole_rays(side=24, distance=1.3, fov=0.9):
    """A side x side pinhole camera on the -z axis at ``distance`` looking at the origin -> (side^2, 3) x 2."""
    c = (np.arange(side) + 0.5) / side - 0.5
    x, y = np.meshgrid(c * fov, c * fov, indexing="xy")
    d = np.stack([x, y, np.ones_like(x)], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.tile(np.array([[0.0, 0.0, -distance]]), (d.shape[0], 1))
    return o.astype(F), d.astype(F)


def scene_case(n_objects, n_rays, seed):
    """K objects with distinct poses and grids of different G and kind -> world rays, the poses (K rows of 12),
    the grids, and each object's rays (K, R, 3) by cn_object_rays' rule."""
    kinds = ("sphere", "half", "full", "sphere", "empty", "half", "sphere", "full")
    sizes = (32, 64, 32, 96, 32, 64, 32, 64)
    ro, rd = camera_rays(n_rays, seed, distance=1.6, spread=0.8)
    poses, grids, ro_k, rd_k = [], [], [], []
    for k in range(n_objects):
        t = [0.45 * np.cos(2.1 * k), 0.45 * np.sin(2.1 * k), 0.2 * (k % 3 - 1)] if n_objects > 1 else [0.0, 0.0, 0.0]
        poses.append(pose_rows(0.7 * k, k % 3, t))
        grids.append(Grid.of(kinds[k], sizes[k], bound=0.5 + 0.25 * (k % 2), radius=0.3))
        o, d = object_rays(ro, rd, poses[-1])
        ro_k.append(o)
        rd_k.append(d)
    return ro, rd, poses, grids, np.stack(ro_k), np.stack(rd_k)


def face_case():
    """occupancy_cases.face_rays with near 0, far 63/16 and P = 64: the probes are exactly j / 16, on the cell
    faces of a G = 32 grid of bound 1."""
    ro, rd, _ = C.face_rays(64)
    return ro, rd, 0.0, 63.0 / 16.0, 64
