"""Iso-surface extraction on the device: cn_isosurface_count / cn_isosurface_emit (ops.isosurface,
nerf.extract_mesh) against the numpy model of tests/isosurface_cases.py.

Every comparison is exact: the vertices as bits (the int32 view, a NaN where the model has a NaN), the
faces as integers -- the semantics fix every rounding, every id and the order of both lists.
"""
import functools

import numpy as np
import pytest
import torch

import isosurface_cases as IC
from test_gpu_parity import dev, embedders, models  # noqa: F401

pytestmark = pytest.mark.gpu

# The kernels' tiles (isosurface.hip): a workgroup covers kBlock consecutive nodes, and the scan kernel
# takes kScanPart workgroup sums -- kScanPart * kBlock nodes -- per round.
BLOCK_NODES = 256
SCAN_PART = 4096


def T(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)          # a copy: the shared cases are read-only


@functools.lru_cache(maxsize=None)
def case(name):
    """(nodes, axis, iso) and the model's (vertices, faces): computed once, shared, never written."""
    iso, axis = 0.0, None
    if name.startswith("pattern"):
        nodes, iso = IC.corner_pattern(int(name[7:])), 0.5
    elif name in ("ties3", "ties5"):
        nodes = IC.tie_grid(int(name[-1]), seed=4, border=False)
    elif name == "sphere":
        nodes = IC.sphere(13, 0.7)
    elif name == "torus":
        nodes = IC.torus(17, 0.6, 0.25)
    elif name in ("smooth33", "smooth129"):
        nodes = IC.smooth_field(int(name[6:]), seed=5)
    elif name == "iso":
        nodes, iso = IC.smooth_field(9, seed=6), 0.375
    elif name == "ellipsoid":
        axis = IC.uneven_axis(11, seed=1)
        nodes = IC.ellipsoid(axis)
    elif name in ("nan", "inf"):
        nodes = IC.smooth_field(6, seed=7)
        nodes[2, 3, 1] = np.nan if name == "nan" else np.inf
    elif name in ("outside", "inside"):
        nodes = np.full((4, 4, 4), -1.0 if name == "outside" else 1.0, dtype=np.float32)
    else:
        raise KeyError(name)
    axis = IC.linspace(nodes.shape[0]) if axis is None else axis
    out = (nodes, axis, iso) + IC.extract(nodes, axis, iso)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _bits(x):
    """The floats as their bit patterns, every NaN as one value: a NaN has to sit where the model has one,
    but which NaN (sign, payload) IEEE arithmetic leaves open, and the host's and the device's differ."""
    return torch.where(torch.isnan(x), torch.full_like(x, float("nan")), x).view(torch.int32)


def _same(vertices, faces, want_v, want_f, dev):
    assert vertices.dtype == torch.float32 and faces.dtype == torch.int32
    assert vertices.shape == want_v.shape and faces.shape == want_f.shape
    assert torch.equal(_bits(vertices), _bits(T(want_v, dev)))
    assert torch.equal(faces, T(want_f, dev))


def _run(name, dev):
    from codenerf import ops
    nodes, axis, iso, want_v, want_f = case(name)
    vertices, faces = ops.isosurface(T(nodes, dev), iso, T(axis, dev))
    _same(vertices, faces, want_v, want_f, dev)
    return vertices, faces


def test_single_cell_patterns(dev):
    """N = 2: all 256 corner patterns; every node is a boundary node of some kind."""
    total = 0
    for p in range(256):
        _, faces = _run(f"pattern{p}", dev)
        total += faces.shape[0]
    assert total == sum(len(case(f"pattern{p}")[4]) for p in range(256)) > 0


@pytest.mark.parametrize("name", ["ties3", "ties5", "sphere", "torus", "iso", "ellipsoid", "inf"])
def test_matches_model(dev, name):
    nodes, _, iso, want_v, want_f = case(name)
    if name.startswith("ties"):
        assert (nodes == iso).sum() > 2
    if name == "iso":
        assert iso != 0.0
    if name == "ellipsoid":
        assert len(np.unique(np.diff(case(name)[1]))) > 3
    assert len(want_f) > 0
    _run(name, dev)


def test_crosses_workgroups(dev):
    """N = 33: 35,937 nodes, many workgroups and a last partial one, the surface through most of them."""
    nodes = case("smooth33")[0]
    assert nodes.size == 35937 and nodes.size > 2 * BLOCK_NODES and nodes.size % BLOCK_NODES
    blocks = (nodes.size + BLOCK_NODES - 1) // BLOCK_NODES
    inside = (nodes > 0.0).reshape(-1)
    mixed = sum(0 < inside[b * BLOCK_NODES:(b + 1) * BLOCK_NODES].sum() < BLOCK_NODES for b in range(blocks))
    assert mixed > blocks // 2
    # the scan's round is SCAN_PART workgroup sums: this case is one partial round (the next test has three)
    assert blocks < SCAN_PART
    _run("smooth33", dev)


def test_crosses_scan_rounds(dev):
    """N = 129: the smallest N whose workgroup sums take more than two rounds of the scan kernel, so the
    running total is carried over twice, with a partial last round."""
    nodes = case("smooth129")[0]
    blocks = (nodes.size + BLOCK_NODES - 1) // BLOCK_NODES
    assert 2 * SCAN_PART < blocks < 3 * SCAN_PART and (128 ** 3 + BLOCK_NODES - 1) // BLOCK_NODES <= 2 * SCAN_PART
    vertices, faces = _run("smooth129", dev)
    assert faces.shape[0] > 100000


@pytest.mark.parametrize("name", ["outside", "inside"])
def test_no_surface(dev, name):
    vertices, faces = _run(name, dev)
    assert vertices.shape == (0, 3) and faces.shape == (0, 3)


def test_nan_node(dev):
    """A NaN node is outside; the vertices on its edges are NaN exactly where the model's are."""
    _, _, _, want_v, want_f = case("nan")
    vertices, faces = _run("nan", dev)
    nan_rows = np.isnan(want_v).any(axis=1)
    assert 0 < nan_rows.sum() <= 14 and np.isnan(want_v[nan_rows]).all()
    assert torch.equal(torch.isnan(vertices).any(dim=1), T(nan_rows, dev))


def _raw_calls(dev, name, max_vertices, max_faces, canary_rows=8):
    """cn_isosurface_count then cn_isosurface_emit with the given capacities into buffers that end in
    canary rows -> (counts, vertices buffer, faces buffer)."""
    from codenerf import _lib
    lib = _lib.load()
    nodes, axis, iso, _, _ = case(name)
    tn, ta = T(nodes, dev), T(axis, dev)
    n = nodes.shape[0]
    workspace = torch.empty(lib.cn_isosurface_workspace_bytes(n) // 8 + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    st = _lib.stream_of(tn)
    _lib.check(lib.cn_isosurface_count(_lib.ptr(tn), n, iso, _lib.ptr(workspace), _lib.ptr(counts), st), "count")
    vbuf = torch.full((max_vertices + canary_rows, 3), -7.0, dtype=torch.float32, device=dev)
    fbuf = torch.full((max_faces + canary_rows, 3), -7, dtype=torch.int32, device=dev)
    _lib.check(lib.cn_isosurface_emit(_lib.ptr(tn), _lib.ptr(ta), n, iso, _lib.ptr(workspace), max_vertices, max_faces,
                                      _lib.ptr(vbuf) if max_vertices else None, _lib.ptr(fbuf) if max_faces else None,
                                      st), "emit")
    return counts, vbuf, fbuf


def test_capacity(dev):
    """One row short on both outputs: the stored rows are the model's first rows and the rows from the
    capacity on keep the canary value."""
    _, _, _, want_v, want_f = case("sphere")
    v, t = len(want_v), len(want_f)
    counts, vbuf, fbuf = _raw_calls(dev, "sphere", v - 1, t - 1)
    assert counts.tolist() == [v, t]
    assert torch.equal(vbuf[:v - 1].view(torch.int32), T(want_v[:v - 1], dev).view(torch.int32))
    assert torch.equal(fbuf[:t - 1], T(want_f[:t - 1], dev))
    assert (vbuf[v - 1:] == -7.0).all() and (fbuf[t - 1:] == -7).all()


def test_capacity_zero_skips_an_output(dev):
    _, _, _, want_v, want_f = case("torus")
    v, t = len(want_v), len(want_f)
    _, vbuf, fbuf = _raw_calls(dev, "torus", 0, t)
    assert torch.equal(fbuf[:t], T(want_f, dev)) and (fbuf[t:] == -7).all() and (vbuf == -7.0).all()
    _, vbuf, fbuf = _raw_calls(dev, "torus", v, 0)
    assert torch.equal(vbuf[:v].view(torch.int32), T(want_v, dev).view(torch.int32))
    assert (vbuf[v:] == -7.0).all() and (fbuf == -7).all()


def test_two_runs_are_identical(dev):
    a, b = _run("smooth33", dev), _run("smooth33", dev)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_non_default_stream(dev):
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        _run("torus", dev)
    stream.synchronize()


def test_cpu_tensor_raises(dev):
    from codenerf import ops
    nodes, axis, iso, _, _ = case("sphere")
    with pytest.raises(ValueError):
        ops.isosurface(torch.from_numpy(np.array(nodes)), iso, T(axis, dev))
    with pytest.raises(ValueError):
        ops.isosurface(T(nodes, dev), iso, torch.from_numpy(np.array(axis)))
    with pytest.raises(ValueError):
        ops.isosurface(T(nodes, dev), float("nan"), T(axis, dev))


def test_extract_mesh_end_to_end(dev):
    from codenerf import ops, synthetic
    from codenerf.nerf import Mesh, density_grid, extract_mesh
    m = models(dev)[0]
    emb, d, bound = embedders(dev), 17, 1.0
    zs = synthetic.latent_codes(5, 1).to(dev)
    grid = density_grid(m, emb, zs, d, bound)
    level = float(grid.median())
    mesh = extract_mesh(m, emb, zs, d, bound, level)
    assert isinstance(mesh, Mesh) and mesh.n_vertices > 0 and mesh.n_faces > 0
    lin = torch.linspace(-bound, bound, d, dtype=torch.float32, device=dev)       # density_grid's own
    vertices, faces = ops.isosurface(grid, level, lin)
    assert torch.equal(mesh.vertices.view(torch.int32), vertices.view(torch.int32)) and torch.equal(mesh.faces, faces)
    assert (mesh.vertices.abs() <= bound).all()
    want_v, want_f = IC.extract(grid.cpu().numpy(), lin.cpu().numpy(), level)
    _same(mesh.vertices, mesh.faces, want_v, want_f, dev)
    raw = extract_mesh(m, emb, zs, d, bound, float(density_grid(m, emb, zs, d, bound, activated=False).median()),
                       activated=False, max_points=1000)
    assert raw.n_faces > 0


def test_extract_mesh_other_precisions_refuse(dev):
    """extract_mesh raises what density_grid raises for a model without a density kernel."""
    from codenerf import synthetic
    from codenerf.nerf import extract_mesh
    m = models(dev, precision="bf16x3")[0]
    with pytest.raises(NotImplementedError, match="f32"):
        extract_mesh(m, embedders(dev), synthetic.latent_codes(5, 1).to(dev), 5, 1.0, 0.5)
