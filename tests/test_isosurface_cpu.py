"""The iso-surface semantics as the numpy model states them (tests/isosurface_cases.py): the vectorised
model against the naive loops, the topology of what it extracts, the triangle table against the
orientation rule it is derived from, and nerf.Mesh's two file formats.  No GPU."""
import itertools
import math
import struct

import numpy as np
import pytest

import isosurface_cases as IC


def _same(got, want):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32))      # bits: NaN positions included
    assert np.array_equal(got[1], want[1])


@pytest.mark.parametrize("case", ["sphere7", "ties5", "ties7", "smooth6", "uneven5", "nan4", "inf4", "n2"])
def test_vectorised_model_equals_naive_loops(case):
    iso, axis = 0.0, None
    if case == "sphere7":
        nodes = IC.sphere(7, 0.6)
    elif case in ("ties5", "ties7"):
        nodes = IC.tie_grid(int(case[-1]), seed=3, border=case == "ties7")
    elif case == "smooth6":
        nodes, iso = IC.smooth_field(6, seed=1), 0.25
    elif case == "uneven5":
        axis = IC.uneven_axis(5, seed=2)
        nodes = IC.ellipsoid(axis)
    elif case in ("nan4", "inf4"):
        nodes = IC.smooth_field(4, seed=4)
        nodes[1, 2, 1] = np.nan if case == "nan4" else np.inf
    else:
        nodes, iso = IC.corner_pattern(0b10010110), 0.5
    axis = IC.linspace(nodes.shape[0]) if axis is None else axis
    want = IC.extract_naive(nodes, axis, iso)
    assert len(want[1]) > 0
    _same(IC.extract(nodes, axis, iso), want)


def _check_closed_surface(nodes, iso, euler):
    n = nodes.shape[0]
    vertices, faces = IC.extract(nodes, IC.linspace(n), iso)
    assert vertices.dtype == np.float32 and faces.dtype == np.int32
    assert IC.is_closed_oriented(faces)
    assert IC.euler_characteristic(len(vertices), faces) == euler
    assert np.array_equal(np.unique(faces), np.arange(len(vertices)))          # every vertex referenced
    assert (faces[:, 0] < faces[:, 1]).all() and (faces[:, 0] < faces[:, 2]).all()
    return vertices, faces


def test_sphere():
    nodes = IC.sphere(13, 0.7)
    vertices, faces = _check_closed_surface(nodes, 0.0, euler=2)
    assert (len(vertices), len(faces)) == (998, 1992)
    # the faces' (cell, tetrahedron) keys ascend and are those of the counting rule
    assert IC.face_keys(nodes, 0.0) == sorted(IC.face_keys(nodes, 0.0))
    assert len(IC.face_keys(nodes, 0.0)) == len(faces)
    # outward normals: the signed volume is positive, and an inscribed polyhedron's is a little low
    volume, exact = IC.enclosed_volume(vertices, faces), 4.0 / 3.0 * math.pi * 0.7 ** 3
    print(f"sphere volume {volume:.4f} against {exact:.4f}")
    assert 0.95 * exact <= volume <= exact


def test_faces_in_cell_tetrahedron_order():
    """Each face lies in the tetrahedron its position in the list says: all three of its vertices sit on
    edges of that (cell, tetrahedron), for a grid where most cells are cut."""
    nodes = IC.tie_grid(5, seed=11, border=False)
    n = 5
    vertices, faces = IC.extract(nodes, IC.linspace(n), 0.0)
    keys = IC.face_keys(nodes, 0.0)
    assert len(keys) == len(faces) and keys == sorted(keys)
    inside = nodes > 0
    owner = []                                     # vertex id -> its edge's key a * 7 + d
    for a in itertools.product(range(n), repeat=3):
        for d in range(7):
            b = tuple(np.asarray(a) + IC.OFF[d + 1])
            if max(b) < n and inside[a] != inside[b]:
                owner.append(((a[0] * n + a[1]) * n + a[2]) * 7 + d)
    assert owner == sorted(owner) and len(owner) == len(vertices)
    for (c, tet), face in zip(keys, faces):
        cell = np.array([c // 16, (c // 4) % 4, c % 4])
        corners = [tuple(cell + IC.OFF[k]) for k in IC.TETS[tet]]
        for v in face:
            a, d = divmod(int(owner[v]), 7)
            pa = (a // 25, (a // 5) % 5, a % 5)
            pb = tuple(np.asarray(pa) + IC.OFF[d + 1])
            assert pa in corners and pb in corners, (c, tet, face)


def test_torus():
    _check_closed_surface(IC.torus(17, 0.6, 0.25), 0.0, euler=0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_tie_grid_is_closed(seed):
    nodes = IC.tie_grid(7, seed=seed)
    assert (nodes == 0.0).sum() > 10
    vertices, faces = IC.extract(nodes, IC.linspace(7), 0.0)
    assert len(faces) and IC.is_closed_oriented(faces)
    assert np.array_equal(np.unique(faces), np.arange(len(vertices)))


def test_single_cell_patterns():
    """All 256 corner patterns of one cell: the triangle count is the per-tetrahedron rule's, and each
    normal -- the vertices at their edges' midpoints -- points from the inside corners to the outside ones."""
    axis = IC.linspace(2)
    for p in range(256):
        nodes = IC.corner_pattern(p)
        vertices, faces = IC.extract(nodes, axis, 0.5)
        ins = [(p >> k) & 1 for k in range(8)]
        keys = IC.face_keys(nodes, 0.5)
        want = sum({0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[sum(ins[k] for k in tet)] for tet in IC.TETS)
        assert len(faces) == want == len(keys), p
        edges = [(0, d) for d in range(7)] + [(k, j - k - 1) for k in range(1, 7) for j in range(k + 1, 8) if j & k == k]
        active = sorted((a * 7 + d) for a, d in edges if ins[a] != ins[a + d + 1])
        assert len(vertices) == len(active), p
        mids = {i: (IC.OFF[key // 7] + IC.OFF[key // 7 + key % 7 + 1]) / 2.0 for i, key in enumerate(active)}
        for (_, tet), face in zip(keys, faces):
            corners = IC.OFF[list(IC.TETS[tet])].astype(np.float64)
            sel = np.array([ins[k] for k in IC.TETS[tet]], dtype=bool)
            m = [mids[int(v)] for v in face]
            normal = np.cross(m[1] - m[0], m[2] - m[0])
            assert normal @ (corners[~sel].mean(axis=0) - corners[sel].mean(axis=0)) > 0.0, (p, tet, face)
            assert face[0] == face.min()


def test_table_is_the_rule():
    """TRI_TABLE, which the vectorised model looks triangles up in, re-derived entry by entry."""
    count, own, dirn = IC.TRI_TABLE
    perms = list(itertools.permutations("xyz"))
    assert perms == sorted(perms) and len(IC.TETS) == 6
    for tet, p in itertools.product(range(6), range(16)):
        ins = [(p >> j) & 1 for j in range(4)]
        tris = [IC.orient(tet, ins, t) for t in IC.rule_triangles(ins)]
        assert count[tet, p] == len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[sum(ins)]
        for t, tri in enumerate(tris):
            for e, (i, j) in enumerate(tri):
                assert ins[i] != ins[j] and i < j
                assert (own[tet, p, t, e], dirn[tet, p, t, e]) == (IC.TETS[tet][i], IC.TETS[tet][j] - IC.TETS[tet][i] - 1)


def test_workspace_formula():
    assert IC.workspace_bytes(2) == 3 * 32 + 2 * 16
    assert IC.workspace_bytes(1) == IC.workspace_bytes(514) == -1


# ---------------------------------------------------------------- Mesh files


def _mesh():
    import torch
    from codenerf.nerf import Mesh
    vertices, faces = IC.extract(IC.sphere(7, 0.6), IC.linspace(7), 0.0)
    vertices[0, 0] = np.float32(1.0) / np.float32(3.0)         # needs all nine digits
    return Mesh(torch.from_numpy(vertices), torch.from_numpy(faces)), vertices, faces


def test_mesh_save_obj(tmp_path):
    mesh, vertices, faces = _mesh()
    assert (mesh.n_vertices, mesh.n_faces) == (len(vertices), len(faces))
    path = str(tmp_path / "m.obj")
    mesh.save_obj(path)
    lines = open(path).read().splitlines()
    v = np.array([[np.float32(x) for x in l.split()[1:]] for l in lines if l.startswith("v ")], dtype=np.float32)
    f = np.array([[int(x) for x in l.split()[1:]] for l in lines if l.startswith("f ")], dtype=np.int32)
    assert len(lines) == len(vertices) + len(faces)
    assert np.array_equal(v.view(np.int32), vertices.view(np.int32))
    assert np.array_equal(f - 1, faces) and f.min() == 1


def test_mesh_save_ply(tmp_path):
    mesh, vertices, faces = _mesh()
    path = str(tmp_path / "m.ply")
    mesh.save_ply(path)
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    head = head.decode("ascii").splitlines()
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    assert f"element vertex {len(vertices)}" in head and f"element face {len(faces)}" in head
    assert "property list uchar int vertex_indices" in head
    assert len(body) == 12 * len(vertices) + 13 * len(faces)
    v = np.frombuffer(body, dtype="<f4", count=3 * len(vertices)).reshape(-1, 3)
    assert np.array_equal(v.view(np.int32), vertices.view(np.int32))
    off = 12 * len(vertices)
    for row in faces:
        assert struct.unpack_from("<Biii", body, off) == (3, *[int(x) for x in row])
        off += 13


def test_mesh_refuses_other_layouts():
    import torch
    from codenerf.nerf import Mesh
    with pytest.raises(ValueError):
        Mesh(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(ValueError):
        Mesh(torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        Mesh(torch.zeros(4, 2), torch.zeros(1, 3, dtype=torch.int32))
