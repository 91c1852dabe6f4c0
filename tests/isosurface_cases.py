"""The iso-surface extraction's semantics in numpy -- the yardstick of cn_isosurface_count /
cn_isosurface_emit (include/codenerf.h holds the normative text) -- and the grids the tests share.

Marching tetrahedra on the Kuhn split of each cell.  ``extract`` is vectorised (N = 33 in about a
second) and looks triangles up in ``TRI_TABLE``, which ``derive_table`` builds from the orientation
rule; ``extract_naive`` walks the cells in plain loops and applies the rule to each triangle, with no
table: the two must agree (tests/test_isosurface_cpu.py)."""
import itertools

import numpy as np

MIN_N, MAX_N = 2, 513
BLOCK_NODES = 256        # nodes per workgroup of the classify / offsets / emit kernels (kBlock, isosurface.hip)
SCAN_PART = 4096         # workgroup sums per round of the scan kernel (kScanPart, isosurface.hip)

# cube corner k -> its (x, y, z) offset, x the most significant bit
OFF = np.array([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], dtype=np.int64)
AXIS_BIT = (4, 2, 1)
# tetrahedron tau = the tau-th permutation (a, b, c) of the axes in lexicographic order: cube corners
# 0, bit(a), bit(a) | bit(b), 7
TETS = [(0, AXIS_BIT[a], AXIS_BIT[a] | AXIS_BIT[b], 7) for a, b, _ in itertools.permutations(range(3))]


def rule_triangles(ins):
    """The unoriented triangles of one tetrahedron whose corners (in tetrahedron order) are inside as
    ``ins`` -> a list of triangles, each three edges (i, j), i < j, of tetrahedron corner indices."""
    edge = lambda i, j: (min(i, j), max(i, j))
    inside = [i for i in range(4) if ins[i]]
    outside = [i for i in range(4) if not ins[i]]
    if len(inside) in (0, 4):
        return []
    if len(inside) in (1, 3):
        (l,) = inside if len(inside) == 1 else outside
        p, q, r = [i for i in range(4) if i != l]
        return [[edge(l, p), edge(l, q), edge(l, r)]]
    (a, b), (c, d) = inside, outside
    return [[edge(a, c), edge(a, d), edge(b, d)], [edge(a, c), edge(b, d), edge(b, c)]]


def orient(tet, ins, tri):
    """``tri`` with its last two edges swapped where its normal -- the vertices at their edges' midpoints
    in index space -- does not point from the centroid of the inside corners to that of the outside ones."""
    corners = OFF[list(TETS[tet])].astype(np.float64)
    mid = [(corners[i] + corners[j]) / 2.0 for i, j in tri]
    normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
    sel = np.asarray(ins, dtype=bool)
    s = float(normal @ (corners[~sel].mean(axis=0) - corners[sel].mean(axis=0)))
    assert s != 0.0, (tet, ins, tri)
    return tri if s > 0.0 else [tri[0], tri[2], tri[1]]


def derive_table():
    """(count[6][16], owner corner k[6][16][2][3], direction d[6][16][2][3]) of the oriented triangles
    of tetrahedron tau under inside pattern p (bit j = corner j of the tetrahedron inside): edge
    (i, j) runs from cube corner k_i to k_j, so its owner is the cell's corner k_i and d = k_j - k_i - 1."""
    count = np.zeros((6, 16), dtype=np.int64)
    own = np.zeros((6, 16, 2, 3), dtype=np.int64)
    dirn = np.zeros((6, 16, 2, 3), dtype=np.int64)
    for tet in range(6):
        for p in range(16):
            ins = [(p >> j) & 1 for j in range(4)]
            tris = [orient(tet, ins, t) for t in rule_triangles(ins)]
            count[tet, p] = len(tris)
            for t, tri in enumerate(tris):
                for e, (i, j) in enumerate(tri):
                    own[tet, p, t, e] = TETS[tet][i]
                    dirn[tet, p, t, e] = TETS[tet][j] - TETS[tet][i] - 1
    return count, own, dirn


TRI_TABLE = derive_table()


def _interp(va, vb, pa, pb, iso):
    """t = (iso - v_a) / (v_b - v_a) and pos = p_a + t (p_b - p_a), each fp32 operation rounded."""
    with np.errstate(all="ignore"):
        t = (np.float32(iso) - va) / (vb - va)
        return (pa + t * (pb - pa)).astype(np.float32)


def _check(nodes, axis):
    nodes = np.ascontiguousarray(nodes, dtype=np.float32)
    axis = np.ascontiguousarray(axis, dtype=np.float32)
    n = nodes.shape[0]
    assert nodes.shape == (n, n, n) and axis.shape == (n,) and MIN_N <= n <= MAX_N
    return nodes, axis, n


def extract(nodes, axis, iso):
    """-> (vertices (V, 3) float32, faces (T, 3) int32)."""
    nodes, axis, n = _check(nodes, axis)
    iso = np.float32(iso)
    inside = nodes > iso
    ii = np.arange(n)
    coord = np.stack(np.meshgrid(ii, ii, ii, indexing="ij"), axis=-1).reshape(-1, 3)       # node -> (ix, iy, iz)
    active = np.zeros((n, n, n, 7), dtype=bool)
    for d in range(7):
        ox, oy, oz = OFF[d + 1]
        lo = inside[:n - ox, :n - oy, :n - oz]
        hi = inside[ox:, oy:, oz:]
        active[:n - ox, :n - oy, :n - oz, d] = lo != hi
    flat = active.reshape(-1)
    keys = np.flatnonzero(flat)                    # a * 7 + d, ascending: the vertex ids are their ranks
    vid = np.full(flat.shape, -1, dtype=np.int64)
    vid[keys] = np.arange(keys.size)
    a, d = keys // 7, keys % 7
    ca = coord[a]
    cb = ca + OFF[d + 1]
    flat_nodes = nodes.reshape(-1)
    va, vb = flat_nodes[a], flat_nodes[(cb[:, 0] * n + cb[:, 1]) * n + cb[:, 2]]
    vertices = np.stack([_interp(va, vb, axis[ca[:, c]], axis[cb[:, c]], iso) for c in range(3)], axis=-1)
    vertices = vertices.reshape(-1, 3).astype(np.float32)

    m = n - 1
    cell_node = (np.arange(m)[:, None, None] * n + np.arange(m)[None, :, None]) * n + np.arange(m)[None, None, :]
    cell_node = cell_node.reshape(-1)              # ascending in the cell index c
    step = (OFF[:, 0] * n + OFF[:, 1]) * n + OFF[:, 2]
    flat_in = inside.reshape(-1)
    corner_in = np.stack([flat_in[cell_node + step[k]] for k in range(8)], axis=-1).astype(np.int64)
    cut = corner_in.sum(axis=1) % 8 != 0           # only a cell with both kinds of corner has a triangle
    cell_node, corner_in = cell_node[cut], corner_in[cut]
    count, own, dirn = TRI_TABLE
    tri = np.full((cell_node.size, 6, 2, 3), -1, dtype=np.int64)
    valid = np.zeros((cell_node.size, 6, 2), dtype=bool)
    for tet in range(6):
        p = sum(corner_in[:, TETS[tet][j]] << j for j in range(4))
        for t in range(2):
            valid[:, tet, t] = count[tet][p] > t
            for e in range(3):
                node = cell_node + step[own[tet][p, t, e]]
                tri[:, tet, t, e] = vid[node * 7 + dirn[tet][p, t, e]]
    faces = tri[valid]                             # (c, tau, triangle) order
    assert (faces >= 0).all()
    first = faces.argmin(axis=1)
    rows = np.arange(faces.shape[0])
    faces = np.stack([faces[rows, (first + j) % 3] for j in range(3)], axis=-1)
    return vertices, faces.reshape(-1, 3).astype(np.int32)


def extract_naive(nodes, axis, iso):
    """``extract`` in plain loops, straight from the rule: no table, no vectorisation.  Small N only."""
    nodes, axis, n = _check(nodes, axis)
    iso = np.float32(iso)
    inside = lambda q: bool(nodes[q[0], q[1], q[2]] > iso)
    lin = lambda q: (int(q[0]) * n + int(q[1])) * n + int(q[2])
    vid, vertices = {}, []
    for a in itertools.product(range(n), repeat=3):
        for d in range(7):
            b = tuple(int(x) for x in np.asarray(a) + OFF[d + 1])
            if max(b) >= n or inside(a) == inside(b):
                continue
            vid[(lin(a), d)] = len(vertices)
            vertices.append([_interp(nodes[a], nodes[b], axis[a[c]], axis[b[c]], iso) for c in range(3)])
    faces = []
    for cell in itertools.product(range(n - 1), repeat=3):
        for tet in range(6):
            corners = [np.asarray(cell) + OFF[k] for k in TETS[tet]]
            ins = [inside(q) for q in corners]
            for tri in rule_triangles(ins):
                ids = [vid[(lin(corners[i]), TETS[tet][j] - TETS[tet][i] - 1)] for i, j in orient(tet, ins, tri)]
                k = ids.index(min(ids))
                faces.append(ids[k:] + ids[:k])
    return (np.asarray(vertices, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3))


def workspace_bytes(n):
    """cn_isosurface_workspace_bytes: three 32-bit words per node (the classify word, the vertex offset,
    the face offset) and two per workgroup of 256 nodes (its vertex and face sums), each of the five
    arrays padded to 16 bytes."""
    if not MIN_N <= n <= MAX_N:
        return -1
    pad16 = lambda b: (b + 15) // 16 * 16
    nodes = n ** 3
    return 3 * pad16(4 * nodes) + 2 * pad16(4 * ((nodes + BLOCK_NODES - 1) // BLOCK_NODES))


# ---------------------------------------------------------------- mesh properties


def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_oriented(faces):
    """Every directed edge exactly once, and its reverse exactly once."""
    e = directed_edges(faces)
    top = int(e.max()) + 1 if e.size else 1
    fwd = e[:, 0] * top + e[:, 1]
    rev = e[:, 1] * top + e[:, 0]
    return np.unique(fwd).size == fwd.size and np.array_equal(np.sort(fwd), np.sort(rev))


def euler_characteristic(n_vertices, faces):
    return n_vertices - 3 * len(faces) // 2 + len(faces)


def enclosed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def face_keys(nodes, iso):
    """The (cell, tetrahedron) of every face, in emission order, from the per-tetrahedron counting rule."""
    nodes = np.asarray(nodes, dtype=np.float32)
    n = nodes.shape[0]
    inside = nodes > np.float32(iso)
    out = []
    for c, cell in enumerate(itertools.product(range(n - 1), repeat=3)):
        for tet in range(6):
            k = sum(bool(inside[tuple(np.asarray(cell) + OFF[q])]) for q in TETS[tet])
            out += [(c, tet)] * {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[k]
    return out


# ---------------------------------------------------------------- grids


def linspace(n, bound=1.0):
    return np.linspace(-bound, bound, n, dtype=np.float32)


def _grid(n, bound=1.0):
    x = np.linspace(-bound, bound, n)
    return np.meshgrid(x, x, x, indexing="ij")


def sphere(n=13, radius=0.7):
    """radius - |p|: inside (positive) within the sphere; iso 0."""
    x, y, z = _grid(n)
    return (radius - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


def torus(n=17, major=0.6, minor=0.25):
    x, y, z = _grid(n)
    return (minor - np.sqrt((np.sqrt(x * x + y * y) - major) ** 2 + z * z)).astype(np.float32)


def ellipsoid(axis, radii=(0.8, 0.5, 0.3)):
    """1 - sum (p_c / r_c)^2 on an arbitrary (uneven) axis: three different radii, so a transposed axis
    or index shows."""
    a = np.asarray(axis, dtype=np.float64)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    return (1.0 - (x / radii[0]) ** 2 - (y / radii[1]) ** 2 - (z / radii[2]) ** 2).astype(np.float32)


def uneven_axis(n, seed=0):
    rng = np.random.default_rng(seed)
    a = np.cumsum(0.5 + rng.random(n))
    return (2.0 * (a - a[0]) / (a[-1] - a[0]) - 1.0).astype(np.float32)


def tie_grid(n, seed=0, border=True):
    """Random integers in [-3, 3] (many nodes equal to iso = 0), with a -1 border when asked."""
    g = np.random.default_rng(seed).integers(-3, 4, size=(n, n, n)).astype(np.float32)
    if border:
        g[[0, -1], :, :] = g[:, [0, -1], :] = g[:, :, [0, -1]] = -1.0
    return g


def smooth_field(n, seed=0):
    """A few random low-frequency waves: a smooth field with a surface through most of the grid."""
    rng = np.random.default_rng(seed)
    x, y, z = _grid(n)
    f = np.zeros_like(x)
    for _ in range(6):
        k = rng.uniform(-4.0, 4.0, size=3)
        f += rng.uniform(0.3, 1.0) * np.sin(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0.0, 6.28))
    return f.astype(np.float32)


def corner_pattern(p):
    """The single cell (N = 2) whose corner k is inside (1.0, against iso 0.5) iff bit k of ``p``; the
    outside values differ per corner, so the vertices are not all at midpoints."""
    g = np.empty(8, dtype=np.float32)
    for k in range(8):
        g[k] = 1.0 if (p >> k) & 1 else 0.125 * (k % 3)
    return g.reshape(2, 2, 2)
