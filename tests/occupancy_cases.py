"""A numpy float32 oracle of the occupancy grid (include/codenerf.h, "Occupancy-grid sample culling"):
the point lookup, the build rule and the Q1 view-direction map, written from the stated formulas,
plus the grids and rays the CPU and GPU tests share.  numpy rounds every float32 operation on its
own, which is the arithmetic the header states."""
import itertools

import numpy as np

F = np.float32
EMPTY_SIGMA_RAW = F(-1.0e4)
EMPTY_ROW = np.array([0.0, 0.0, 0.0, -1.0e4], dtype=F)


# ---------------------------------------------------------------- lookup


def grid_scale(g, bound):
    """(lo, inv_cell) as the Python layer passes them: -bound and float32(G / (2 bound))."""
    return F(-bound), F(g / (2.0 * bound))


def lookup_cells(p, g, bound):
    """p (..., 3) -> (inside (...,) bool, linear cell index c (...,) int64, 0 where outside)."""
    p = np.asarray(p, dtype=F)
    lo, inv = grid_scale(g, bound)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (p - lo) * inv                                    # two roundings
        inside = np.all((u >= F(0)) & (u < F(g)), axis=-1)    # NaN fails
    i = np.floor(np.where(inside[..., None], u, F(0))).astype(np.int64)
    return inside, (i[..., 0] * g + i[..., 1]) * g + i[..., 2]


def bit_of(bits, c):
    """Bit c & 31 of word c >> 5 of the uint32 words ``bits``."""
    bits = np.asarray(bits).view(np.uint32)
    return ((bits[c >> 5] >> (c & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def lookup(p, bits, g, bound):
    """Occupied? per point: inside the cube and its cell's bit set."""
    inside, c = lookup_cells(p, g, bound)
    return inside & bit_of(bits, c)


def lookup_cells_f64(p, g, bound):
    """The same lookup in float64 -> (inside, c, distance of u to the nearest cell face in cells)."""
    u = (np.asarray(p, dtype=np.float64) + bound) * (g / (2.0 * bound))
    inside = np.all((u >= 0) & (u < g), axis=-1)
    i = np.floor(np.where(inside[..., None], u, 0.0)).astype(np.int64)
    face = np.abs(u - np.round(u)).min(axis=-1)
    return inside, (i[..., 0] * g + i[..., 1]) * g + i[..., 2], face


# ---------------------------------------------------------------- bits


def pack_cells(occ):
    """(G, G, G) bool [ix, iy, iz] -> uint32 words (G^3 / 32,)."""
    return np.packbits(np.asarray(occ, dtype=bool).reshape(-1), bitorder="little").view("<u4").copy()


def unpack_cells(bits, g):
    return np.unpackbits(np.asarray(bits).view(np.uint8), bitorder="little").astype(bool).reshape(g, g, g)


def build_cells(nodes, threshold, dilate):
    """The build rule: cell i is occupied iff a node of [i - dilate, i + 1 + dilate] per axis, clamped
    to the node grid, is > threshold or NaN.  nodes (G+1, G+1, G+1) -> (G, G, G) bool."""
    nodes = np.asarray(nodes, dtype=F)
    g = nodes.shape[0] - 1
    with np.errstate(invalid="ignore"):
        hot = (nodes > F(threshold)) | np.isnan(nodes)
    occ = np.zeros((g, g, g), dtype=bool)
    cell = np.arange(g)
    for dx, dy, dz in itertools.product(range(-dilate, dilate + 2), repeat=3):
        ix, iy, iz = (np.clip(cell + d, 0, g) for d in (dx, dy, dz))      # clamped: a node met twice
        occ |= hot[np.ix_(ix, iy, iz)]
    return occ


def build_bits(nodes, threshold, dilate):
    return pack_cells(build_cells(nodes, threshold, dilate))


def cell_centres(g, bound):
    c = (np.arange(g) + 0.5) * (2.0 * bound / g) - bound
    return np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1)


def grid_bits(kind, g, bound=1.0, radius=0.5):
    """The shared grids: "full", "empty", "half" (ix < G/2: x < 0) and "sphere" (cell centre within
    ``radius`` of the origin)."""
    if kind == "full":
        occ = np.ones((g, g, g), dtype=bool)
    elif kind == "empty":
        occ = np.zeros((g, g, g), dtype=bool)
    elif kind == "half":
        occ = np.zeros((g, g, g), dtype=bool)
        occ[: g // 2] = True
    elif kind == "sphere":
        occ = np.linalg.norm(cell_centres(g, bound), axis=-1) < radius
    else:
        raise ValueError(kind)
    return pack_cells(occ)


# ---------------------------------------------------------------- cull


def ray_points(ro, rd, z):
    """p = rd * z + ro, the product and the sum each rounded (cn::mul_add_rn) -> (R, S, 3)."""
    ro, rd, z = (np.asarray(a, dtype=F) for a in (ro, rd, z))
    with np.errstate(invalid="ignore", over="ignore"):
        return rd[:, None, :] * z[:, :, None] + ro[:, None, :]


def q1_ray(n_rays, n_samples, chunk_rows):
    """(R, S) int64: the ray whose direction sample (r, s) takes (decode_sample, ragged last chunk)."""
    r = np.arange(n_rays, dtype=np.int64)[:, None]
    s = np.arange(n_samples, dtype=np.int64)[None, :]
    base = (r // chunk_rows) * chunk_rows
    rcnt = np.minimum(chunk_rows, n_rays - base)
    return base + ((r - base) * n_samples + s) % rcnt


def cull(ro, rd, z, chunk_rows, code_index, bits, g, bound):
    """cn_occupancy_cull's outputs -> dict(keep (R, S), count, sample_index, pts, vdir, code_out)."""
    rd = np.asarray(rd, dtype=F)
    n, s = np.asarray(z).shape
    p = ray_points(ro, rd, z)
    keep = lookup(p, bits, g, bound)
    k = np.nonzero(keep.reshape(-1))[0]                       # ascending sample order
    code = np.arange(n, dtype=np.int64) if code_index is None else np.asarray(code_index, dtype=np.int64)
    return dict(keep=keep, count=int(k.size), sample_index=k.astype(np.int32), pts=p.reshape(-1, 3)[k],
                vdir=rd[q1_ray(n, s, chunk_rows).reshape(-1)[k]], code_out=code[k // s])


def random_rays(n_rays, n_samples, seed, spread=1.3):
    """Rays whose samples fall inside and outside the cube [-1, 1]^3."""
    rng = np.random.default_rng(seed)
    ro = (rng.standard_normal((n_rays, 3)) * 0.4).astype(F)
    rd = rng.standard_normal((n_rays, 3)).astype(F)
    z = np.sort(rng.random((n_rays, n_samples)) * spread, axis=-1).astype(F)
    return ro, rd, z


def face_rays(n_samples, g=32):
    """Axis-aligned rays from the cube's corner region whose samples land exactly on cell faces and on
    the cube's faces (bound 1, G = 32: faces at multiples of 1/16, all exactly representable, so is
    every product and sum): one ray along each axis (+ and -), depths k / 16 from 0 on."""
    ro, rd = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            o = np.array([0.03125, -0.46875, 0.21875])        # inside cells, off their faces
            o[axis] = -1.0 * sign                              # starts on a cube face
            d = np.zeros(3)
            d[axis] = sign
            ro.append(o)
            rd.append(d)
    z = np.tile((np.arange(n_samples) / 16.0)[None, :], (6, 1))
    return np.asarray(ro, dtype=F), np.asarray(rd, dtype=F), z.astype(F)
