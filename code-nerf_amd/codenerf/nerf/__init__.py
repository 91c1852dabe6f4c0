"""Render orchestration on the gfx950 kernels (view_synthesis/nerf/__init__.py).

Same entry points, argument meaning and return values as the reference:
prepare_samplers (:15), prepare_embedders (:42), predict_radiance_and_render
(:74), forward_pass (:94), parallel_image_render (:137).  Underneath, a whole
ray list (a rank's full slice, not one 4096-ray chunk at a time) goes through
one launch per stage -- depth sampling, the fused encode+MLP field kernel,
compositing, inverse-CDF resampling -- with the reference's per-chunk
semantics (quirk Q1) reproduced inside the field kernel's index math from
``chunk_rows``.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple, Union

import torch
import torch.distributed as dist

from .. import ops
from ..utils import get_minibatches, split_sizes  # noqa: F401
from .point_sampler import PointSampler
from .position_embed import PositionalEmbedder
from .ray_sampler import RaySampler
from .volumetric_render import volume_render

__all__ = ["RaySampler", "PointSampler", "PositionalEmbedder", "volume_render", "prepare_samplers",
           "prepare_embedders", "predict_radiance_and_render", "forward_pass", "parallel_image_render",
           "render_rays", "gather_rows", "gather_views", "density", "density_grid", "OccupancyGrid", "Mesh", "extract_mesh",
           "density_gradient", "normals", "SceneObject", "render_scene", "render_scene_autograd", "rigid_pose",
           "similarity_pose"]


def prepare_samplers(cfg, height: int, width: int, intrinsics, datatype, device) -> Tuple[RaySampler, PointSampler]:
    """nerf/__init__.py:15-39."""
    ray_sampler = RaySampler(height, width, intrinsics, sample_size=cfg.nerf.ray_sampler.num_random_rays,
                             device=device, datatype=datatype)
    ps = cfg.nerf.point_sampler
    point_sampler = PointSampler(ps.num_coarse, ps.num_fine, ps.near_limit, ps.far_limit,
                                 spacing_mode=ps.spacing_mode, perturb=ps.perturb, dtype=datatype, device=device)
    return ray_sampler, point_sampler


def prepare_embedders(cfg, datatype, device) -> Tuple[PositionalEmbedder, Optional[PositionalEmbedder]]:
    """nerf/__init__.py:42-71."""
    e = cfg.nerf.embedder
    exyz = PositionalEmbedder(e.num_encoding_fn_xyz, e.log_sampling_xyz, e.include_input_xyz, datatype, device)
    edir = None
    if e.use_viewdirs:
        edir = PositionalEmbedder(e.num_encoding_fn_dir, e.log_sampling_dir, e.include_input_dir, datatype, device)
    return exyz, edir


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


def _check_embedders(embedders):
    exyz, edir = embedders
    if edir is None:
        raise NotImplementedError("CodeNeRFModel consumes view directions; use_viewdirs=False has no runnable "
                                  "reference path (layer_dir1 expects dim_dir inputs)")
    if not (exyz.num_freq == 10 and exyz.include_input and edir.num_freq == 4 and edir.include_input):
        raise NotImplementedError("the field kernel implements L_xyz=10 / L_dir=4 with inputs included")
    return exyz.freqs, edir.freqs


def _codes(z_s: torch.Tensor, z_t: torch.Tensor):
    """Code rows for the field kernels -> (z_s rows, z_t rows, per-ray code index or None):
    the distinct rows when the codes came from ShapeTextureEmbedding (train), one row when
    they are an expand() of one row (eval / render), else one row per ray."""
    tag = getattr(z_s, "_cn_code_rows", None)
    if tag is not None and getattr(z_t, "_cn_code_rows", None) is tag:
        if tag.index is None and tag.shape_rows.shape[0] == 1:      # one object: every ray's row 0
            return tag.shape_rows, tag.texture_rows, None
        if tag.index is not None and tag.index.shape[0] == z_s.shape[0]:
            return tag.shape_rows, tag.texture_rows, (None if tag.shape_rows.shape[0] == 1 else tag.index)
    if z_s.stride(0) == 0 and z_t.stride(0) == 0:
        # an expand() of one code row: hand the field its base row, so the code gradient (already
        # the sum over the rays, from g_code) lands on it directly instead of through a slice + expand
        # backward (a zero-filled (R, 256) tensor and a column sum per model and step)
        return _expand_base(z_s), _expand_base(z_t), None
    return z_s, z_t, None


def _expand_base(z: torch.Tensor) -> torch.Tensor:
    b = z._base
    if b is not None and b.dim() == 2 and b.shape[0] == 1 and b.shape[1] == z.shape[1] and \
            b.stride(1) == z.stride(1) and b.data_ptr() == z.data_ptr():
        return b
    return z[:1]


def _field(model, embedders, rd, z_s, z_t, chunk_rows, pts=None, ro=None, z=None, pair=None):
    """The fused field of ``model`` (a CodeNeRFModel or a DDP wrapper of one): through the module's
    ``forward`` (its ``field`` form), so a DistributedDataParallel wrapper runs its forward
    bookkeeping and its gradient hooks fire in the backward, as in the reference's DDP training."""
    fx, fd = _check_embedders(embedders)
    cs, ct, code_index = _codes(z_s, z_t)
    if isinstance(model, torch.nn.parallel.DistributedDataParallel):
        return model(cs, ct, field=dict(rd=rd, chunk_rows=chunk_rows, fx=fx, fd=fd, pts=pts, ro=ro, z=z,
                                        code_index=code_index))
    from ..models.model import _field_op
    return _field_op(_unwrap(model), cs, ct, rd, chunk_rows, fx, fd, pts=pts, ro=ro, z=z, code_index=code_index,
                     pair=pair)


def _density_field_raw(model, embedders, rd, z_s, z_t, chunk_rows, pts=None, ro=None, z=None, pair=None):
    """_field's signature on the density kernel: raw rows [0, 0, 0, sigma_raw] (render_rays'
    coarse_rgb=False).  No gradient path, and no chunk_rows: density has no view direction (Q1)."""
    from ..models.model import density_code_bias
    fx, _ = _check_embedders(embedders)
    cs, _, code_index = _codes(z_s, z_t)
    m = _unwrap(model)
    with torch.no_grad():
        cb = density_code_bias(m, cs)
        return ops.density_field(m.packed(), cb, fx, pts=pts, ro=None if pts is not None else ro,
                                 rd=None if pts is not None else rd, z=None if pts is not None else z,
                                 code_index=code_index, want_sigma=False, want_raw=True)


def density(model, embedders, pts: torch.Tensor, z_s: torch.Tensor) -> torch.Tensor:
    """sigma_raw (model.py:174-186) at points of any leading shape (..., 3) for one shape code (1, 256) or
    one per row of the first dimension (pts.shape[0], 256) -> sigma_raw of the leading shape.  No view
    direction and no texture code enter a density.  Inference only."""
    from ..models.model import density_code_bias
    fx, _ = _check_embedders(embedders)
    assert pts.shape[-1] == 3, "pts must be (..., 3)"
    lead = tuple(pts.shape[:-1])
    n = lead[0] if lead else 1
    per_row = 1
    for k in lead[1:]:
        per_row *= k
    assert z_s.dim() == 2 and z_s.shape[0] in (1, n), "z_s must be (1, C) or one row per pts.shape[0]"
    m = _unwrap(model)
    with torch.no_grad():
        if z_s.shape[0] > 1 and z_s.stride(0) == 0:
            z_s = z_s[:1]
        cb = density_code_bias(m, z_s)
        sigma = ops.density_field(m.packed(), cb, fx, pts=pts.detach().reshape(n, per_row, 3))
    return sigma.reshape(lead)


def density_grid(model, embedders, z_s: torch.Tensor, resolution: int, bound: float, activated: bool = True,
                 max_points: int = 1 << 22) -> torch.Tensor:
    """The density of one shape code (1, 256) on a regular grid -- the input of an iso-surface
    extraction -> (D, D, D), D = ``resolution``, axis order [ix, iy, iz], the points
    ``linspace(-bound, bound, D)`` per axis (``meshgrid(indexing="ij")``), evaluated in slabs of at
    most ``max_points`` points.  ``activated``: softplus(sigma_raw - 1), the density the renderer
    integrates (volumetric_render.py:32); else sigma_raw."""
    from ..models.model import density_code_bias
    fx, _ = _check_embedders(embedders)
    d = int(resolution)
    assert d >= 1 and max_points >= 1 and z_s.dim() == 2 and z_s.shape[0] == 1, \
        "density_grid takes one shape code (1, C) and a positive resolution"
    m = _unwrap(model)
    with torch.no_grad():
        cb = density_code_bias(m, z_s)
        packed = m.packed()
        dev = cb.device
        lin = torch.linspace(-bound, bound, d, dtype=torch.float32, device=dev)
        out = torch.empty(d * d * d, dtype=torch.float32, device=dev)
        for start in range(0, d * d * d, max_points):
            k = torch.arange(start, min(start + max_points, d * d * d), device=dev)
            pts = torch.stack((lin[k // (d * d)], lin[(k // d) % d], lin[k % d]), dim=-1)
            out[start:start + k.numel()] = ops.density_field(packed, cb, fx, pts=pts)
        if activated:
            out = torch.nn.functional.softplus(out - 1.0)
    return out.view(d, d, d)


def _density_gradient_rows(model, embedders, cs, code_index, pts=None, ro=None, rd=None, z=None) -> torch.Tensor:
    """ops.density_gradient of ``model`` on distinct shape code rows ``cs`` -> (.., 4) rows
    [d sigma_raw / d point, sigma_raw], without gradients."""
    from ..models.model import density_code_bias
    fx, _ = _check_embedders(embedders)
    m = _unwrap(model)
    with torch.no_grad():
        cb = density_code_bias(m, cs)
        return ops.density_gradient(m.packed(), m.packed("f32_w16_t"), cb, fx, pts=pts, ro=ro, rd=rd, z=z,
                                    code_index=code_index)


def _activate_gradient(grad: torch.Tensor, sigma_raw: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d sigma_raw / d p, sigma_raw) -> (d sigma / d p, sigma) of the density the renderer integrates,
    sigma = softplus(sigma_raw - 1) (volumetric_render.py:32; torch's softplus, threshold 20):
    d sigma / d sigma_raw = sigmoid(sigma_raw - 1)."""
    x = sigma_raw - 1.0
    return grad * torch.sigmoid(x)[..., None], torch.nn.functional.softplus(x)


def _normals_from_gradient(g: torch.Tensor) -> torch.Tensor:
    """n = -g / |g| in fp32: exactly (0, 0, 0) where |g| is 0, NaN in all three where a component of g is
    not finite.  g is divided by its largest |component| first, so that the squares neither underflow (a
    tiny gradient still has a unit normal) nor overflow."""
    big = g.abs().amax(dim=-1, keepdim=True)
    u = g / torch.where(big == 0, torch.ones_like(big), big)
    n = torch.where(big == 0, torch.zeros_like(g), -u / torch.linalg.vector_norm(u, dim=-1, keepdim=True))
    return torch.where(torch.isfinite(g).all(dim=-1, keepdim=True), n, torch.full_like(g, float("nan")))


def _composite_normals(weights: torch.Tensor, n: torch.Tensor) -> torch.Tensor:
    """sum_s w_s n_s over the samples of each ray, (R, S) x (R, S, 3) -> (R, 3); a sample of weight
    exactly 0 contributes 0 whatever its normal (NaN included)."""
    w = weights[..., None]
    return torch.where(w == 0, torch.zeros_like(n), w * n).sum(dim=-2)


def density_gradient(model, embedders, pts: torch.Tensor, z_s: torch.Tensor,
                     activated: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The density's gradient with respect to the point, and the density, at points of any leading shape
    (..., 3) for one shape code (1, 256) or one per row of the first dimension (pts.shape[0], 256) ->
    (grad (..., 3), sigma (...)), from one kernel (ops.density_gradient).  ``activated``: of
    softplus(sigma_raw - 1), the density the renderer integrates; else of sigma_raw, whose values are
    bitwise ``density``'s.  Inference only."""
    assert pts.shape[-1] == 3, "pts must be (..., 3)"
    lead = tuple(pts.shape[:-1])
    n = lead[0] if lead else 1
    per_row = 1
    for k in lead[1:]:
        per_row *= k
    assert z_s.dim() == 2 and z_s.shape[0] in (1, n), "z_s must be (1, C) or one row per pts.shape[0]"
    with torch.no_grad():
        if z_s.shape[0] > 1 and z_s.stride(0) == 0:
            z_s = z_s[:1]
        gs = _density_gradient_rows(model, embedders, z_s, None, pts=pts.detach().reshape(n, per_row, 3))
        gs = gs.reshape(lead + (4,))
        grad, sigma = gs[..., :3], gs[..., 3]
        if activated:
            grad, sigma = _activate_gradient(grad, sigma)
    return grad, sigma


def normals(model, embedders, pts: torch.Tensor, z_s: torch.Tensor) -> torch.Tensor:
    """Unit normals of the density's level sets at ``pts`` (..., 3) -> (..., 3): -g / |g| of
    density_gradient's g (towards lower density; the activation only scales g by a positive factor, so
    sigma_raw's gradient is used), exactly (0, 0, 0) where |g| is 0 and NaN where g is not finite.
    Inference only."""
    with torch.no_grad():
        return _normals_from_gradient(density_gradient(model, embedders, pts, z_s)[0])


_point_normals = normals   # extract_mesh's and render_rays' keyword of the same name shadows the function there


class Mesh:
    """A triangle mesh: ``vertices`` (V, 3) float32 and ``faces`` (T, 3) int32 (0-based vertex ids,
    counter-clockwise seen from outside), optionally with per-vertex ``normals`` (V, 3) float32 and
    ``colors`` (V, 3) float32 in [0, 1], on any device.  Saving copies them to the host."""

    def __init__(self, vertices: torch.Tensor, faces: torch.Tensor, *, normals: Optional[torch.Tensor] = None,
                 colors: Optional[torch.Tensor] = None):
        if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
            raise ValueError(f"vertices must be (V, 3) float32, got {tuple(vertices.shape)} {vertices.dtype}")
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
            raise ValueError(f"faces must be (T, 3) int32, got {tuple(faces.shape)} {faces.dtype}")
        for name, t in (("normals", normals), ("colors", colors)):
            if t is not None and (t.dim() != 2 or tuple(t.shape) != tuple(vertices.shape) or t.dtype != torch.float32):
                raise ValueError(f"{name} must be (V, 3) float32 with V = {vertices.shape[0]}, got "
                                 f"{tuple(t.shape)} {t.dtype}")
        if colors is not None and colors.numel() and not bool(((colors >= 0.0) & (colors <= 1.0)).all()):
            raise ValueError("colors must lie in [0, 1]")
        self.vertices, self.faces, self.normals, self.colors = vertices, faces, normals, colors

    @property
    def n_vertices(self) -> int:
        return int(self.vertices.shape[0])

    @property
    def n_faces(self) -> int:
        return int(self.faces.shape[0])

    def _host(self):
        return (self.vertices.detach().cpu().contiguous().numpy(), self.faces.detach().cpu().contiguous().numpy())

    def _host_attrs(self):
        return tuple(None if t is None else t.detach().cpu().contiguous().numpy() for t in (self.normals, self.colors))

    def save_obj(self, path: str) -> None:
        """Wavefront OBJ text: ``v x y z`` (%.9g, which round-trips a float32) and ``f a b c``, 1-based.
        With colours: ``v x y z r g b`` (the common vertex-colour extension); with normals: a ``vn`` line
        per vertex after the vertices and faces as ``f a//a b//b c//c``."""
        v, f = self._host()
        nrm, col = self._host_attrs()
        with open(path, "w") as out:
            if col is None:
                out.writelines("v %.9g %.9g %.9g\n" % (float(x), float(y), float(z)) for x, y, z in v)
            else:
                out.writelines("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % tuple(float(t) for t in (*p, *c))
                               for p, c in zip(v, col))
            if nrm is None:
                out.writelines("f %d %d %d\n" % (a + 1, b + 1, c + 1) for a, b, c in f.tolist())
            else:
                out.writelines("vn %.9g %.9g %.9g\n" % (float(x), float(y), float(z)) for x, y, z in nrm)
                out.writelines("f %d//%d %d//%d %d//%d\n" % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1)
                               for a, b, c in f.tolist())

    def save_ply(self, path: str) -> None:
        """Binary little-endian PLY: float32 x, y, z per vertex, then float32 nx, ny, nz (with normals) and
        uchar red, green, blue (with colours: round(c * 255), clamped); a uchar count (3) and int32 indices
        per face."""
        import numpy as np
        v, f = self._host()
        nrm, col = self._host_attrs()
        props = "property float x\nproperty float y\nproperty float z\n"
        fields = [("p", "<f4", (3,))]
        if nrm is not None:
            props += "property float nx\nproperty float ny\nproperty float nz\n"
            fields.append(("n", "<f4", (3,)))
        if col is not None:
            props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            fields.append(("c", "u1", (3,)))
        header = ("ply\nformat binary_little_endian 1.0\n"
                  f"element vertex {v.shape[0]}\n{props}"
                  f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
        verts = np.empty(v.shape[0], dtype=fields)
        verts["p"] = v
        if nrm is not None:
            verts["n"] = nrm
        if col is not None:
            verts["c"] = np.clip(np.rint(col.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
        rows = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
        rows["n"], rows["i"] = 3, f
        with open(path, "wb") as out:
            out.write(header.encode("ascii"))
            out.write(verts.tobytes())
            out.write(rows.tobytes())


def extract_mesh(model, embedders, z_s: torch.Tensor, resolution: int, bound: float, level: float,
                 activated: bool = True, max_points: int = 1 << 22, normals: bool = False, colors: bool = False,
                 z_t: Optional[torch.Tensor] = None) -> Mesh:
    """The ``level`` iso-surface of one shape code's density as a triangle mesh, on the device:
    density_grid(resolution, bound, activated, max_points) followed by ops.isosurface with that grid's
    own ``linspace(-bound, bound, resolution)``, so every vertex lies on an edge of the sampled lattice.
    ``level`` is in the grid's unit (activated density, or sigma_raw) and has no default; face normals
    point towards lower density.  Inference only; reads the vertex and face counts back once (a host
    synchronisation, see ops.isosurface).  No simplification.
    ``normals``: ``Mesh.normals`` = ``normals(model, embedders, vertices, z_s)``, the density's own
    gradient direction at each vertex (not an average of face normals).
    ``colors`` (needs the texture code ``z_t`` (1, 256); computes the normals too): ``Mesh.colors`` =
    sigmoid of the colour channels of the model's no-grad field at the vertices, each seen along
    rd = -normal (the ray travels into the surface; (0, 0, -1) where the normal is zero or not finite).
    Vertices and faces are those of the plain call."""
    if colors and z_t is None:
        raise ValueError("colors=True needs the texture code z_t (1, C)")
    d = int(resolution)
    nodes = density_grid(model, embedders, z_s, d, bound, activated=activated, max_points=max_points)
    lin = torch.linspace(-bound, bound, d, dtype=torch.float32, device=nodes.device)
    vertices, faces = ops.isosurface(nodes, level, lin)
    if not (normals or colors):
        return Mesh(vertices, faces)
    nrm = _point_normals(model, embedders, vertices, z_s)
    col = None
    if colors:
        col = _vertex_colors(model, embedders, vertices, nrm, z_s, z_t)
    return Mesh(vertices, faces, normals=nrm, colors=col)


def _vertex_colors(model, embedders, vertices, nrm, z_s, z_t) -> torch.Tensor:
    """sigmoid(raw[..., :3]) of ``model``'s inference field at ``vertices`` (V, 3), one sample per ray,
    viewed along -``nrm`` ((0, 0, -1) where the normal is zero or not finite) -> (V, 3) in [0, 1]."""
    v = vertices.shape[0]
    if v == 0:
        return torch.empty(0, 3, dtype=torch.float32, device=vertices.device)
    with torch.no_grad():
        usable = torch.isfinite(nrm).all(dim=-1, keepdim=True) & (nrm != 0).any(dim=-1, keepdim=True)
        down = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float32, device=vertices.device).expand(v, 3)
        rd = torch.where(usable, -nrm, down).contiguous()
        raw = _field(model, embedders, rd, z_s.detach(), z_t.detach(), chunk_rows=v, pts=vertices.view(v, 1, 3))
        return torch.sigmoid(raw[:, 0, :3])


class OccupancyGrid:
    """One shape code's occupancy bits for sample culling in the inference render (render_rays'
    ``occupancy``): the cube [-bound, bound]^3 in ``resolution``^3 cells (a multiple of 32 in
    [32, 512]), one bit per cell in ``bits``, a device int32 tensor of resolution^3 / 32 words -- cell
    (ix, iy, iz) is bit c & 31 of word c >> 5, c = (ix G + iy) G + iz (include/codenerf.h).  A sample
    in an empty cell, or outside the cube, skips the field and counts as exactly zero density."""

    def __init__(self, bits: torch.Tensor, resolution: int, bound: float):
        g = int(resolution)
        if not (g % 32 == 0 and 32 <= g <= 512):
            raise ValueError(f"resolution must be a multiple of 32 in [32, 512], got {resolution}")
        if not float(bound) > 0.0:
            raise ValueError(f"bound must be positive, got {bound}")
        if bits.dtype != torch.int32 or bits.dim() != 1 or bits.numel() != g * g * g // 32:
            raise ValueError(f"bits must be {g * g * g // 32} int32 words, got {tuple(bits.shape)} {bits.dtype}")
        self.bits, self.resolution, self.bound = bits.contiguous(), g, float(bound)

    @classmethod
    def full(cls, resolution: int, bound: float, device) -> "OccupancyGrid":
        """Every cell occupied: culls only the samples outside the cube."""
        g = int(resolution)
        return cls(torch.full((g * g * g // 32,), -1, dtype=torch.int32, device=device), g, bound)

    @classmethod
    def from_nodes(cls, nodes: torch.Tensor, threshold: float, dilate: int = 1, *, bound: float) -> "OccupancyGrid":
        """From node densities (G+1, G+1, G+1) at linspace(-bound, bound, G+1) per axis (what
        density_grid(resolution=G + 1) returns): ops.occupancy_build."""
        return cls(ops.occupancy_build(nodes, threshold, dilate), nodes.shape[0] - 1, bound)

    @classmethod
    def from_density(cls, model, embedders, z_s: torch.Tensor, resolution: int = 128, *, bound: float,
                     threshold: float, dilate: int = 1) -> "OccupancyGrid":
        """From ``model``'s activated density of shape code ``z_s`` (1, 256): density_grid(resolution + 1,
        activated=True), then from_nodes.  ``threshold`` (in activated density) has no default."""
        nodes = density_grid(model, embedders, z_s, int(resolution) + 1, bound, activated=True)
        return cls.from_nodes(nodes, threshold, dilate, bound=bound)

    def occupied_fraction(self) -> float:
        """Share of the cells that are occupied (reads the bits back: a host synchronisation)."""
        b = self.bits.view(torch.uint8)
        set_bits = sum(int(((b >> k) & 1).sum()) for k in range(8))
        return set_bits / float(self.resolution ** 3)


def _check_sync_free(*models):
    """``sync_free=True`` runs the counted field entries, which exist for the fp32 16x16x4 kernels alone."""
    for m in models:
        if m is not None and _unwrap(m).kernel_format() != "f32_w16":
            raise ValueError(f"sync_free=True needs models of precision 'f32' (the counted field kernels are fp32); "
                             f"got precision {_unwrap(m).precision!r}")


def _culled_field(model, embedders, rd, z_s, z_t, chunk_rows, ro, z, occupancy: OccupancyGrid, density_only: bool,
                  sync_free: bool = False):
    """A render field call under an occupancy grid: cull -> ``model``'s inference field in points mode
    over the M' kept samples (the density kernel when ``density_only``) -> expand to raw (R, S, 4).
    Kept samples get the bits of the unculled call; culled ones the zero-density row.
    ``sync_free``: M' stays on the device -- the field runs its counted entry over the compact buffers at
    capacity and computes the first M' rows, the same bits."""
    from ..models.model import _field_op, density_code_bias
    fx, fd = _check_embedders(embedders)
    cs, ct, code_index = _codes(z_s, z_t)
    m = _unwrap(model)
    with torch.no_grad():
        many = cs.shape[0] > 1
        count, _, pts, vdir, code_out, state = ops.occupancy_cull(
            ro.detach(), rd.detach(), z, chunk_rows, occupancy.bits, occupancy.resolution, occupancy.bound,
            code_index=code_index, want_code=many, sync=not sync_free)
        raw = None
        if sync_free:
            index, cap = (code_out if many else None), pts.shape[0]
            if cap and density_only:
                raw = ops.density_field(m.packed(), density_code_bias(m, cs), fx, pts=pts, code_index=index,
                                        want_sigma=False, want_raw=True, count=count)
            elif cap:
                raw = _field_op(m, cs.detach(), ct.detach(), vdir, cap, fx, fd, pts=pts.view(cap, 1, 3),
                                code_index=index, count=count)
        elif count:
            index = code_out if many else None
            if density_only:
                raw = ops.density_field(m.packed(), density_code_bias(m, cs), fx, pts=pts, code_index=index,
                                        want_sigma=False, want_raw=True)
            else:
                raw = _field_op(m, cs.detach(), ct.detach(), vdir, count, fx, fd, pts=pts.view(count, 1, 3),
                                code_index=index)
        return ops.occupancy_expand(raw, state)


def _weight_culled_field(model, embedders, rd, z_s, z_t, chunk_rows, ro, z, tolerance: float,
                         occupancy: Optional[OccupancyGrid], sync_free: bool = False):
    """The fine field call under ``rgb_tolerance``: densities of every sample (the density kernel, under
    the grid when there is one) -> the render's own weights -> cull by weight -> ``model``'s inference
    field in points mode over the kept samples, its colours scattered into the density rows -> raw
    (R, S, 4).  Every row keeps its sigma_raw; a culled one has raw colours [0, 0, 0].
    ``sync_free``: as _culled_field's -- the kept count stays on the device for the field and the scatter."""
    from ..models.model import _field_op
    fx, fd = _check_embedders(embedders)
    cs, ct, code_index = _codes(z_s, z_t)
    m = _unwrap(model)
    with torch.no_grad():
        ro, rd = ro.detach(), rd.detach()
        if occupancy is None:
            raw = _density_field_raw(model, embedders, rd, z_s, z_t, chunk_rows, ro=ro, z=z)
        else:       # the grid's empty rows have weight exactly 0: they fall out by w > 0
            raw = _culled_field(model, embedders, rd, z_s, z_t, chunk_rows, ro, z, occupancy, density_only=True,
                                sync_free=sync_free)
        weights = ops.volume_render(raw, z, rd)[3]
        eps_weight, eps_tail = ops.weight_cull_thresholds(tolerance, z.shape[1])
        many = cs.shape[0] > 1
        count, sample_index, pts, vdir, code_out, _ = ops.weight_cull(
            weights, ro, rd, z, chunk_rows, eps_weight, eps_tail, code_index=code_index, want_code=many,
            sync=not sync_free)
        if sync_free:
            cap = pts.shape[0]
            if cap:
                kept = _field_op(m, cs.detach(), ct.detach(), vdir, cap, fx, fd, pts=pts.view(cap, 1, 3),
                                 code_index=code_out if many else None, count=count)
                ops.scatter_rgb(kept, sample_index, raw, count=count)
        elif count:
            kept = _field_op(m, cs.detach(), ct.detach(), vdir, count, fx, fd, pts=pts.view(count, 1, 3),
                             code_index=code_out if many else None)
            ops.scatter_rgb(kept, sample_index, raw)
        return raw


def forward_pass(model, embedders, rd: torch.Tensor, pts: torch.Tensor,
                 object_embedding: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
    """nerf/__init__.py:94-134: embed + MLP for one chunk -> (R, S, 4).

    Q1: sample row k = r*S + s takes the view direction of ray k mod R, R = this call's ray count.
    """
    if rd is None:
        _check_embedders((embedders[0], None))
    z_s, z_t = object_embedding
    return _field(model, embedders, rd, z_s, z_t, chunk_rows=pts.shape[0], pts=pts)


def render_rays(ro: torch.Tensor, rd: torch.Tensor, z_s: torch.Tensor, z_t: torch.Tensor,
                point_sampler: PointSampler, embedders, coarse_model, fine_model=None, chunk_rows: Optional[int] = None,
                t_rand: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None,
                coarse_only: bool = False, events: Optional[dict] = None,
                coarse_rgb: bool = True, occupancy: Optional[OccupancyGrid] = None,
                rgb_tolerance: Optional[float] = None, normals: bool = False,
                span_probes: Optional[int] = None, sync_free: bool = False) -> Dict[str, torch.Tensor]:
    """predict_radiance_and_render over a whole ray list, chunk semantics kept via ``chunk_rows``.

    Returns rgb/depth/acc for the coarse pass (+ weights) and, unless
    ``coarse_only``, the fine pass.  Equal to running the reference's
    predict_radiance_and_render on every ``chunk_rows`` slice and concatenating.
    ``events`` (bench instrumentation): a dict that receives (start, end)
    torch.cuda.Event pairs around each field-kernel launch under key "field".
    ``coarse_rgb=False`` (inference only): the coarse pass exists to give ``weights_coarse`` to the
    resampling, which read densities alone, so the coarse field runs the density kernel (raw rows
    [0, 0, 0, sigma_raw], the same sigma bits) and the result has no "rgb_coarse"; everything else
    in it is bitwise the default call's.
    ``occupancy`` (inference only): an OccupancyGrid of the rendered object.  Each field call then
    culls its samples against the grid, runs the field over the kept ones alone and expands the result;
    a culled sample has exactly zero density (not the reference's softplus tail), a kept one the
    unculled call's bits.  The kept count is read back on the host once per field call, so this
    render is not graph-capturable unless ``sync_free=True``.
    ``rgb_tolerance`` (inference only; needs a fine pass): a bound on the weight the fine pass may leave
    uncoloured per ray.  The fine pass then runs the density kernel over every fine sample, forms the
    render's weights from those densities, and runs the colour layers only for the samples kept by
    include/codenerf.h's rule with eps_tail = tol / 2 and eps_weight = the largest float32 <=
    tol / (2 S); a culled sample keeps its density and composites the colour 0.5.  "depth_fine",
    "acc_fine", "disp_fine" and the coarse entries are bitwise the plain call's; each channel of
    "rgb_fine" is within 0.501 x (the ray's culled weight, <= tol) of it, plus fp32 summation rounding.
    0.0 culls only samples of weight 0 or NaN.  Composes with ``occupancy``.  The kept count is read
    back on the host once (ops.weight_cull), so this render is not graph-capturable either unless
    ``sync_free=True``.
    ``normals`` (inference only; needs a fine pass): adds "normal_fine" (R, 3) = sum_s w_s n_s, w the fine
    pass's compositing weights and n_s the unit normals (``normals``' rule) of the fine model's density at
    the fine samples, from one ops.density_gradient launch over (ro, rd, z_fine).  Not normalised: its
    length is at most "acc_fine".  A sample of weight exactly 0 -- every culled one -- contributes 0 even
    where its normal is NaN.  Every other entry is bitwise the call's without ``normals``; composes with
    ``occupancy`` and ``rgb_tolerance`` (the gradient kernel still runs over every fine sample).
    ``span_probes`` (needs ``occupancy`` and a sampler linear in depth, spacing_mode "lindisp"): a probe count,
    a multiple of 64 in [64, 1024].  The coarse depths then come from PointSampler.sample_span in place of
    sample_uniform: each ray's Nc depths are stratified inside its own span of the sampler's [near, far], from
    the probe before its first occupied cell to the probe after its last (include/codenerf.h's rule), with
    ``t_rand`` as before; a ray that meets no occupied cell keeps the whole range.  Everything after the coarse
    depths is the same code path.  Adds "ray_span" (R, 2), the rays' (t_lo, t_hi), and "ray_hit" (R,) bool.
    The span is not strictly conservative (a corner clipped between two probes), which a grid dilated by one
    cell -- OccupancyGrid.from_density's default -- covers.
    ``sync_free`` (models of precision "f32" only: ValueError otherwise): the culled field calls leave their kept
    counts on the device.  Each runs the counted form of its kernel (include/codenerf.h) over the compact
    buffers at capacity, sized for every sample and computing the kept rows alone, so nothing is read back
    and the render can be captured in a graph and replayed on new inputs.  Every entry is bitwise the
    ``sync_free=False`` result; composes with ``occupancy``, ``rgb_tolerance``, ``coarse_rgb=False``,
    ``normals`` and ``span_probes``; without ``occupancy`` and ``rgb_tolerance`` nothing is culled and it
    changes nothing.
    """
    if sync_free:
        _check_sync_free(coarse_model, None if coarse_only else fine_model)
    if span_probes is not None:
        if occupancy is None:
            raise ValueError("span_probes places the coarse samples by the occupancy grid: pass occupancy=")
        point_sampler.check_span_probes(span_probes)
    if normals and (coarse_only or fine_model is None):
        raise ValueError("normals=True composites the fine pass's normals: there is no fine pass with "
                         "coarse_only=True (or without a fine model)")
    if rgb_tolerance is not None:
        rgb_tolerance = float(rgb_tolerance)
        if not rgb_tolerance >= 0.0:
            raise ValueError(f"rgb_tolerance must be >= 0 and not NaN, got {rgb_tolerance}")
        if coarse_only or fine_model is None:
            raise ValueError("rgb_tolerance bounds the fine pass's colours: there is none to apply it to with "
                             "coarse_only=True (or without a fine model)")
    if not coarse_rgb or occupancy is not None or rgb_tolerance is not None or normals:
        if torch.is_grad_enabled() and (
                any(t is not None and t.requires_grad for t in (ro, rd, z_s, z_t)) or
                any(p.requires_grad for m in (coarse_model, fine_model) if m is not None
                    for p in _unwrap(m).param_list())):
            if rgb_tolerance is not None:
                raise ValueError("rgb_tolerance is an inference render: the two-phase fine pass has no backward "
                                 "(render under torch.no_grad(), or pass rgb_tolerance=None)")
            if normals:
                raise ValueError("normals=True is an inference render: the density-gradient kernel has no "
                                 "backward (render under torch.no_grad(), or pass normals=False)")
            if coarse_rgb:
                raise ValueError("occupancy culling is an inference render: the compacted field has no backward "
                                 "(render under torch.no_grad(), or pass occupancy=None)")
            raise ValueError("coarse_rgb=False is the inference render: the density kernel has no backward "
                             "(render under torch.no_grad(), or keep coarse_rgb=True)")

    def timed_field(*a, field=_field, **kw):
        if events is None:
            return field(*a, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = field(*a, **kw)
        e1.record()
        events.setdefault("field", []).append((e0, e1))
        return r

    n = ro.shape[0]
    chunk_rows = n if chunk_rows is None else chunk_rows
    ps = point_sampler
    if ps.perturb and t_rand is None:
        t_rand = torch.rand(n, ps.num_samples_coarse, dtype=torch.float32, device=ro.device)
    if span_probes is None:
        _, z_c = ops.sample_uniform(ro.detach(), rd.detach(), ps.z_vals, ps.lower, ps.upper,
                                    t_rand if ps.perturb else None, want_pts=False)
    else:
        z_c, ray_span, probe_range = ps.sample_span(ro, rd, occupancy, t_rand, span_probes)
    pair = None
    if occupancy is not None:
        def culled(density_only):
            def field(model, embedders, rd, z_s, z_t, chunk_rows, ro=None, z=None, pair=None):
                return _culled_field(model, embedders, rd, z_s, z_t, chunk_rows, ro, z, occupancy, density_only,
                                     sync_free)
            return field
        coarse_field, fine_field = culled(not coarse_rgb), culled(False)
    else:
        coarse_field, fine_field = (_field if coarse_rgb else _density_field_raw), _field
    if rgb_tolerance is not None:
        def fine_field(model, embedders, rd, z_s, z_t, chunk_rows, ro=None, z=None, pair=None):
            return _weight_culled_field(model, embedders, rd, z_s, z_t, chunk_rows, ro, z, rgb_tolerance, occupancy,
                                        sync_free)
    if fine_model is not None and not coarse_only and coarse_rgb and occupancy is None and rgb_tolerance is None:
        # the two differentiable fields' pre-field launches (code terms, packs, zeroed accumulators) as
        # one launch; each field takes its part (no launch when either runs without gradients)
        from ..autograd import new_field_pair, prefetch_render_prepares
        if not any(isinstance(m, torch.nn.parallel.DistributedDataParallel) for m in (coarse_model, fine_model)):
            pair = new_field_pair()     # train_minibatch: the two training backwards in shared launches
        fx, fd = _check_embedders(embedders)
        cs, ct, code_index = _codes(z_s, z_t)
        prefetch_render_prepares(_unwrap(coarse_model), _unwrap(fine_model), rd, ro, cs, ct, ps.num_samples_coarse,
                                 ps.num_samples_coarse + ps.num_samples_fine, chunk_rows, fx, fd, code_index)
    # pts = ro + rd z is formed inside the field kernel (z detached, point_sampler.py:115); with
    # gradients on, the field's backward returns d ro / d rd through both the points and the view dirs
    raw_c = timed_field(coarse_model, embedders, rd, z_s, z_t, chunk_rows, ro=ro, z=z_c, pair=pair,
                        field=coarse_field)
    rgb_c, disp_c, acc_c, w_c, depth_c = volume_render(raw_c, z_c, rd)
    out = {"rgb_coarse": rgb_c, "disp_coarse": disp_c, "acc_coarse": acc_c, "weights_coarse": w_c,
           "depth_coarse": depth_c, "z_coarse": z_c}
    if not coarse_rgb:
        del out["rgb_coarse"]       # composited from zero colours: not a result
    if span_probes is not None:
        out.update({"ray_span": ray_span, "ray_hit": probe_range[:, 0] >= 0})
    if coarse_only:
        return out
    if ps.perturb and u is None:
        u = torch.rand(n, ps.num_samples_fine, dtype=torch.float32, device=ro.device)
    _, z_f = ops.sample_pdf(ro.detach(), rd.detach(), w_c.detach()[..., 1:-1], z_c, ps.num_samples_fine,
                            u if ps.perturb else ps.u_lin, want_pts=False)
    raw_f = timed_field(fine_model, embedders, rd, z_s, z_t, chunk_rows, ro=ro, z=z_f, pair=pair, field=fine_field)
    rgb_f, disp_f, acc_f, w_f, depth_f = volume_render(raw_f, z_f, rd)
    out.update({"rgb_fine": rgb_f, "disp_fine": disp_f, "acc_fine": acc_f, "depth_fine": depth_f, "z_fine": z_f})
    if normals:
        cs, _, code_index = _codes(z_s, z_t)
        with torch.no_grad():
            gs = _density_gradient_rows(fine_model, embedders, cs, code_index, ro=ro.detach(), rd=rd.detach(), z=z_f)
            out["normal_fine"] = _composite_normals(w_f, _normals_from_gradient(gs[..., :3]))
    return out


class SceneObject:
    """One instance in a scene (render_scene): its codes ``z_s`` / ``z_t`` (one row each), its
    OccupancyGrid in the object's own frame, and its similarity pose, the object-to-world ``rotation`` (3, 3),
    ``translation`` (3,) and uniform ``scale`` -- host values (nested sequences or CPU tensors; a float), the
    identity at scale 1 by default.
    The grid is mandatory (``OccupancyGrid.full`` is the minimum): a field means nothing outside the region
    it was trained on and contributes exactly nothing there.  ``scale``: how many times larger than its
    canonical (unit-cube) size the object appears, finite and > 0.  It is kept apart from ``rotation``, which
    stays orthonormal: an enlarged medium has its densities divided by the scale, so that the opacity along a
    chord through the object does not depend on its size (include/codenerf.h's rule), and the object-frame
    rays are divided by it, which keeps the ray parameter.  ``coarse_model`` / ``fine_model``: this object's
    category models, the scene's by default."""

    def __init__(self, z_s: torch.Tensor, z_t: torch.Tensor, occupancy: OccupancyGrid, rotation=None, translation=None,
                 coarse_model=None, fine_model=None, scale: float = 1.0):
        if not isinstance(occupancy, OccupancyGrid):
            raise ValueError("a scene object needs its OccupancyGrid (OccupancyGrid.full(...) at the least): it "
                             "bounds the region the object's field is evaluated in")
        rot = [[float(v) for v in row] for row in ([[1, 0, 0], [0, 1, 0], [0, 0, 1]] if rotation is None else rotation)]
        t = [float(v) for v in ((0, 0, 0) if translation is None else translation)]
        if len(rot) != 3 or any(len(row) != 3 for row in rot) or len(t) != 3:
            raise ValueError("rotation must be (3, 3) and translation (3,)")
        flat = [v for row in rot for v in row] + t
        if any(v != v or v in (float("inf"), float("-inf")) for v in flat):
            raise ValueError("rotation and translation must be finite")
        gram = max(abs(sum(rot[k][i] * rot[k][j] for k in range(3)) - (1.0 if i == j else 0.0))
                   for i in range(3) for j in range(3))
        if gram > 1e-5:
            raise ValueError(f"rotation must be orthonormal (max |R^T R - I| = {gram:.3g} > 1e-5): a uniform size "
                             "goes in scale=, which rescales the densities with it")
        try:
            scale = float(scale)
        except (TypeError, ValueError):
            raise ValueError(f"scale must be one host number, got {scale!r}") from None
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"scale must be finite and > 0, got {scale}")
        for name, code in (("z_s", z_s), ("z_t", z_t)):
            if code.dim() != 2 or (code.shape[0] != 1 and code.stride(0) != 0):
                raise ValueError(f"{name} must be one code row (1, C) (or an expand() of one)")
        self.codes = (z_s, z_t)                     # as given: what render_scene's gradient check looks at
        self.z_s, self.z_t = (c if c.shape[0] == 1 else c[:1] for c in self.codes)
        self.occupancy, self.rotation, self.translation, self.scale = occupancy, rot, t, scale
        self.coarse_model, self.fine_model = coarse_model, fine_model


def render_scene(ro: torch.Tensor, rd: torch.Tensor, objects, point_sampler: PointSampler, embedders, coarse_model,
                 fine_model=None, *, coarse_only: bool = False, coarse_rgb: bool = True,
                 t_rand: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None,
                 span_probes: Optional[int] = None, sync_free: bool = False) -> Dict[str, torch.Tensor]:
    """Several posed objects (1..8 SceneObjects) in one image: render_rays' hierarchical render of the world
    rays ``ro`` / ``rd`` (R, 3), with the objects composed per sample.  A pose (rigid, or with a uniform scale:
    the object-frame ray divided by it) keeps the ray parameter, so one set of depths along the world ray serves
    every object: the coarse depths
    (ops.sample_uniform), each object's field on its own object-frame rays (ops.object_rays) under its grid
    (the density kernel when ``coarse_rgb=False``), ops.volume_render_compose with the world ``rd``,
    ops.sample_pdf on the composed weights, the objects' fine fields at the shared fine depths and the
    composition again.  Interpenetrating objects and partial transmittance are integrated as one medium
    (include/codenerf.h's rule), not blended per image.  An object of scale s has its densities divided by s (the
    scaled entries, taken when any object's scale is not 1; all scales 1 is the rigid render, bit for bit).
    Returns render_rays' entries plus "acc_objects_coarse" / "acc_objects_fine" (K, R): each object's share
    of "acc_*", its instance mask.  A sample's view direction is its own ray's (``chunk_rows`` is the whole
    ray list).  With one identity-posed object every shared entry is bitwise
    render_rays(..., occupancy=grid, chunk_rows=None)'s.
    ``span_probes``: render_rays' argument.  A ray's span is that of the union of the objects' occupied probes
    (each object's grid probed along its own object-frame ray), so the shared coarse depths cover every object the
    ray meets; adds "ray_span" and "ray_hit".
    Inference only.  Each object's kept count is read back once per field call -- 2 K host
    synchronisations per render (K with ``coarse_only``) -- so this render is not graph-capturable unless
    ``sync_free=True`` (render_rays' argument: the counted field calls, the same bits, models of precision
    "f32" only)."""
    objects = list(objects)
    if not 1 <= len(objects) <= 8 or not all(isinstance(o, SceneObject) for o in objects):
        raise ValueError(f"a scene holds 1..8 SceneObjects, got {len(objects)} entries")
    coarse_models = [o.coarse_model if o.coarse_model is not None else coarse_model for o in objects]
    fine_models = [o.fine_model if o.fine_model is not None else fine_model for o in objects]
    if not coarse_only and any(m is None for m in fine_models):
        raise ValueError("every object needs a fine model (its own or the scene's) unless coarse_only=True")
    if torch.is_grad_enabled() and (
            any(t is not None and t.requires_grad for t in [ro, rd] + [c for o in objects for c in o.codes]) or
            any(p.requires_grad for m in coarse_models + ([] if coarse_only else fine_models)
                for p in _unwrap(m).param_list())):
        raise ValueError("render_scene is an inference render: the compacted fields and the composition have no "
                         "backward (render under torch.no_grad())")
    if span_probes is not None:
        point_sampler.check_span_probes(span_probes)
    if sync_free:
        _check_sync_free(*(coarse_models + ([] if coarse_only else fine_models)))
    n = ro.shape[0]
    ps = point_sampler
    with torch.no_grad():
        if ps.perturb and t_rand is None:
            t_rand = torch.rand(n, ps.num_samples_coarse, dtype=torch.float32, device=ro.device)
        if span_probes is None:
            _, z_c = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, t_rand if ps.perturb else None,
                                        want_pts=False)
        scales = [o.scale for o in objects] if any(o.scale != 1.0 for o in objects) else None
        ro_k, rd_k = ops.object_rays(ro, rd, [(o.rotation, o.translation) + (() if scales is None else (o.scale,))
                                              for o in objects])
        if span_probes is not None:
            z_c, ray_span, probe_range = ps.sample_span(ro_k, rd_k, [o.occupancy for o in objects], t_rand,
                                                        span_probes)

        def fields(models, z, density_only):
            return [_culled_field(m, embedders, rd_k[k], o.z_s, o.z_t, n, ro_k[k], z, o.occupancy, density_only,
                                  sync_free)
                    for k, (o, m) in enumerate(zip(objects, models))]

        rgb_c, disp_c, acc_c, w_c, depth_c, obj_c = ops.volume_render_compose(fields(coarse_models, z_c, not coarse_rgb),
                                                                             z_c, rd, scales=scales)
        out = {"rgb_coarse": rgb_c, "disp_coarse": disp_c, "acc_coarse": acc_c, "weights_coarse": w_c,
               "depth_coarse": depth_c, "z_coarse": z_c, "acc_objects_coarse": obj_c}
        if not coarse_rgb:
            del out["rgb_coarse"]       # composited from zero colours: not a result
        if span_probes is not None:
            out.update({"ray_span": ray_span, "ray_hit": probe_range[:, 0] >= 0})
        if coarse_only:
            return out
        if ps.perturb and u is None:
            u = torch.rand(n, ps.num_samples_fine, dtype=torch.float32, device=ro.device)
        _, z_f = ops.sample_pdf(ro, rd, w_c[..., 1:-1], z_c, ps.num_samples_fine, u if ps.perturb else ps.u_lin,
                                want_pts=False)
        rgb_f, disp_f, acc_f, _, depth_f, obj_f = ops.volume_render_compose(fields(fine_models, z_f, False), z_f, rd,
                                                                           scales=scales)
        out.update({"rgb_fine": rgb_f, "disp_fine": disp_f, "acc_fine": acc_f, "depth_fine": depth_f, "z_fine": z_f,
                    "acc_objects_fine": obj_f})
    return out


def rigid_pose(omega: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """A rigid pose from 6 numbers: the rotation vector ``omega`` (3,) (axis times angle, Rodrigues' formula) and
    the translation ``t`` (3,) -> (12,): the object-to-world rotation row-major, then t -- a row of
    render_scene_autograd's ``poses``.  Plain torch ops, differentiable; at omega = 0 it is the identity with
    finite gradients (below |omega|^2 = 1e-8 the two coefficients are their Taylor series)."""
    if omega.shape != (3,) or t.shape != (3,):
        raise ValueError("omega and t must be (3,)")
    th2 = (omega * omega).sum()
    small = th2 < 1e-8
    safe = torch.where(small, torch.ones_like(th2), th2)
    th = safe.sqrt()
    half = 0.5 * th
    a = torch.where(small, 1.0 - th2 / 6.0, torch.sin(th) / th)                          # sin(th) / th
    b = torch.where(small, 0.5 - th2 / 24.0, 0.5 * (torch.sin(half) / half) ** 2)        # (1 - cos(th)) / th^2
    zero = torch.zeros_like(th2)
    k = torch.stack([torch.stack([zero, -omega[2], omega[1]]), torch.stack([omega[2], zero, -omega[0]]),
                     torch.stack([-omega[1], omega[0], zero])])
    rot = torch.eye(3, dtype=omega.dtype, device=omega.device) + a * k + b * (k @ k)
    return torch.cat([rot.reshape(9), t])


def similarity_pose(omega: torch.Tensor, t: torch.Tensor, log_scale: torch.Tensor) -> torch.Tensor:
    """A similarity pose from 7 numbers: ``rigid_pose(omega, t)`` and the uniform scale exp(``log_scale``) (a
    scalar or (1,) tensor) -> (13,), a row of render_scene_autograd's (K, 13) ``poses``.  Plain torch ops,
    differentiable; the exponential keeps the scale > 0 under any optimiser step."""
    if log_scale.numel() != 1:
        raise ValueError("log_scale must hold one number")
    return torch.cat([rigid_pose(omega, t), log_scale.reshape(1).exp()])


def render_scene_autograd(ro: torch.Tensor, rd: torch.Tensor, objects, point_sampler: PointSampler, embedders,
                          coarse_model, fine_model=None, *, poses: Optional[torch.Tensor] = None,
                          coarse_only: bool = False, t_rand: Optional[torch.Tensor] = None,
                          u: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """render_scene, differentiable: the same render and result dict (``coarse_rgb`` is always on), with
    gradients w.r.t. every object's ``z_s`` / ``z_t``, the world rays ``ro`` / ``rd`` and ``poses`` -- so a scene
    can be fitted to an image or to per-instance masks ("acc_objects_*").  ``poses``: an optional (K, 12) float32
    device tensor that overrides the objects' host poses, each row the object-to-world rotation row-major, then
    the translation (``rigid_pose`` builds one from 6 numbers); or (K, 13), each row with the object's uniform scale
    last (``similarity_pose``), whose gradient is the sum of its two paths: through the object-frame rays and
    through the densities.  With (K, 12) or None the objects' host scales are used, as constants.  The tensor is
    read to the host once per render (the scales' host values come from the same read), one host
    synchronisation more than render_scene's 2 K (there is no ``sync_free`` here: the backward sizes its buffers
    by the kept counts).
    The path per object and pass: autograd.CullRows -> the fused fp32 field in points mode over the kept rows
    (frozen weights: its deterministic fused backward) -> autograd.ExpandRows; then autograd.VolumeRenderCompose.
    Every backward kernel reduces in a fixed order, so two runs give the same gradients.  The kept sets, the fine
    depths and the coarse weights that feed sample_pdf are constants (detached, as in the reference).
    ValueError: a model parameter requires grad (frozen weights only), a model's precision is not "f32", or the
    scene does not hold 1..8 SceneObjects."""
    from ..autograd import culled_field_autograd, object_rays_autograd, volume_render_compose_autograd
    objects = list(objects)
    if not 1 <= len(objects) <= 8 or not all(isinstance(o, SceneObject) for o in objects):
        raise ValueError(f"a scene holds 1..8 SceneObjects, got {len(objects)} entries")
    coarse_models = [o.coarse_model if o.coarse_model is not None else coarse_model for o in objects]
    fine_models = [o.fine_model if o.fine_model is not None else fine_model for o in objects]
    if not coarse_only and any(m is None for m in fine_models):
        raise ValueError("every object needs a fine model (its own or the scene's) unless coarse_only=True")
    for m in coarse_models + ([] if coarse_only else fine_models):
        if any(p.requires_grad for p in _unwrap(m).param_list()):
            raise ValueError("render_scene_autograd differentiates codes, rays and poses with frozen weights: a "
                             "model parameter requires grad (call model.requires_grad_(False))")
        if getattr(_unwrap(m), "precision", "f32") != "f32":
            raise ValueError(f"render_scene_autograd runs the fp32 field (precision \"f32\"), got "
                             f"{_unwrap(m).precision!r}")
    rows = scales = scale_rows = None
    host_scales = [o.scale for o in objects] if any(o.scale != 1.0 for o in objects) else None
    if poses is None:
        rows = [[v for row in o.rotation for v in row] + list(o.translation) + ([] if host_scales is None else [o.scale])
                for o in objects]
        scale_rows = host_scales
    elif not (isinstance(poses, torch.Tensor) and poses.dim() == 2 and poses.shape[0] == len(objects)
              and poses.shape[1] in (12, 13) and poses.dtype == torch.float32 and poses.device == ro.device):
        raise ValueError(f"poses must be a ({len(objects)}, 12) or ({len(objects)}, 13) float32 tensor on the rays' "
                         "device")
    elif poses.shape[1] == 13:
        rows = poses.detach().cpu().tolist()            # the render's one pose read-back: the scales' host values too
        scales, scale_rows = poses[:, 12], [row[12] for row in rows]
        if not all(0.0 < v < float("inf") for v in scale_rows):
            raise ValueError(f"every scale (poses[:, 12]) must be finite and > 0, got {scale_rows}")
    elif host_scales is not None:
        # rigid rows with the objects' constant scales: one (K, 13) tensor, no gradient into its last column
        poses = torch.cat([poses, poses.new_tensor(host_scales)[:, None]], dim=1)
        scale_rows = host_scales
    fx, fd = _check_embedders(embedders)
    n = ro.shape[0]
    ps = point_sampler
    if ps.perturb and t_rand is None:
        t_rand = torch.rand(n, ps.num_samples_coarse, dtype=torch.float32, device=ro.device)
    _, z_c = ops.sample_uniform(ro.detach(), rd.detach(), ps.z_vals, ps.lower, ps.upper,
                                t_rand if ps.perturb else None, want_pts=False)
    ro_k, rd_k = (t.unbind(0) for t in object_rays_autograd(ro, rd, poses, rows))

    def fields(models, z):
        return [culled_field_autograd(_unwrap(m), ro_k[k], rd_k[k], z, o.z_s, o.z_t, o.occupancy, fx, fd)
                for k, (o, m) in enumerate(zip(objects, models))]

    rgb_c, disp_c, acc_c, w_c, depth_c, obj_c = volume_render_compose_autograd(fields(coarse_models, z_c), z_c, rd,
                                                                                  scales, scale_rows)
    out = {"rgb_coarse": rgb_c, "disp_coarse": disp_c, "acc_coarse": acc_c, "weights_coarse": w_c,
           "depth_coarse": depth_c, "z_coarse": z_c, "acc_objects_coarse": obj_c}
    if coarse_only:
        return out
    if ps.perturb and u is None:
        u = torch.rand(n, ps.num_samples_fine, dtype=torch.float32, device=ro.device)
    _, z_f = ops.sample_pdf(ro.detach(), rd.detach(), w_c.detach()[..., 1:-1], z_c, ps.num_samples_fine,
                            u if ps.perturb else ps.u_lin, want_pts=False)
    rgb_f, disp_f, acc_f, _, depth_f, obj_f = volume_render_compose_autograd(fields(fine_models, z_f), z_f, rd,
                                                                                scales, scale_rows)
    out.update({"rgb_fine": rgb_f, "disp_fine": disp_f, "acc_fine": acc_f, "depth_fine": depth_f, "z_fine": z_f,
                "acc_objects_fine": obj_f})
    return out


def predict_radiance_and_render(rays: Tuple[torch.Tensor, torch.Tensor], point_sampler: PointSampler,
                                embedders, coarse_model, fine_model,
                                latent_embedding: Tuple[torch.Tensor, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """nerf/__init__.py:74-91 -> (rgb_coarse, rgb_fine)."""
    ro, rd = rays
    z_s, z_t = latent_embedding
    out = render_rays(ro, rd, z_s, z_t, point_sampler, embedders, coarse_model, fine_model)
    return out["rgb_coarse"], out["rgb_fine"]


def parallel_image_render(cfg, pose: torch.Tensor, object_embedding, models, samplers, embedders, device,
                          key: str = "rgb_fine", coarse_only: bool = False,
                          coarse_rgb: bool = True, occupancy: Optional[OccupancyGrid] = None,
                          rgb_tolerance: Optional[float] = None,
                          span_probes: Optional[int] = None, sync_free: bool = False) -> Optional[torch.Tensor]:
    """nerf/__init__.py:137-226: shard the image's rays over ranks, render, gather on rank 0.

    The split is the reference's (Q5: truncating, the last rank takes the
    remainder); each rank renders its contiguous slice in ONE pass with the
    reference's chunking (``cfg.nerf.validation.chunksize``) kept as Q1
    semantics; one all-gather (RCCL over xGMI on MI355X) of the padded
    per-rank rows.  Rank 0 returns (H*W, 3); the others return None.
    ``coarse_rgb=False``: the coarse pass computes densities only (render_rays); ``key`` cannot then
    be "rgb_coarse".  ``occupancy``: an OccupancyGrid of the object, for render_rays' sample culling.
    ``rgb_tolerance``: render_rays' bound for the fine pass's weight-based colour culling.
    ``span_probes``: render_rays' probe count for per-ray coarse depth spans (needs ``occupancy``).
    ``sync_free``: render_rays' flag -- the culled field calls read no kept count back.
    """
    if not coarse_rgb and key == "rgb_coarse":
        raise ValueError('coarse_rgb=False renders no coarse colours: key="rgb_coarse" needs coarse_rgb=True')
    rank = 0
    is_distributed = bool(getattr(cfg, "is_distributed", False))
    n_gpus = int(getattr(cfg, "gpus", 1))
    if is_distributed:
        rank = dist.get_rank()
    for _, model in models.items():
        model.eval()
    with torch.no_grad():
        ray_sampler, point_sampler = samplers
        ro, rd = ray_sampler.get_bundle(tform_cam2world=pose)
        ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
        num_rays = ro.shape[0]
        per, pad = split_sizes(num_rays, n_gpus)
        start = sum(per[:rank])
        sl = slice(start, start + per[rank])
        z_s, z_t = object_embedding
        z_s = z_s.to(device).expand(num_rays, -1)[sl]
        z_t = z_t.to(device).expand(num_rays, -1)[sl]
        out = render_rays(ro[sl].to(device), rd[sl].to(device), z_s, z_t, point_sampler, embedders,
                          models["nerf_coarse"], models.get("nerf_fine"), cfg.nerf.validation.chunksize,
                          coarse_only=coarse_only, coarse_rgb=coarse_rgb, occupancy=occupancy,
                          rgb_tolerance=rgb_tolerance, span_probes=span_probes, sync_free=sync_free)
        rgb = out[key]
        if not is_distributed:
            return rgb
        return gather_rows(rgb, per, rank)


def gather_views(rows: torch.Tensor, per: List[int], rank: int, n_views: int) -> Optional[torch.Tensor]:
    """Many views sharded at once (parallel_image_render's split applied to every view): ``rows`` is
    this rank's (n_views * per[rank], C) slice rows, view-major.  One all-gather of the padded
    per-rank blocks (gather_rows), then rank 0 interleaves them back: rank r's view v block is
    pixels [sum(per[:r]), sum(per[:r+1])) of view v.  Rank 0 -> (n_views, sum(per), C); others None.
    Uneven shares (Q5: the last rank takes the remainder) are handled."""
    if rows.shape[0] != n_views * per[rank]:
        raise ValueError(f"gather_views: {rows.shape[0]} rows, expected {n_views} x {per[rank]}")
    allrows = gather_rows(rows, [p * n_views for p in per], rank)
    if allrows is None:
        return None
    c = tuple(rows.shape[1:])
    blocks = allrows.split([p * n_views for p in per])
    return torch.cat([b.view((n_views, p) + c) for b, p in zip(blocks, per)], dim=1)


def gather_rows(rows: torch.Tensor, per: List[int], rank: int, single_tensor: bool = True) -> Optional[torch.Tensor]:
    """Pad every rank's rows to the largest share, all-gather, trim on rank 0 (nerf/__init__.py:212-224).

    ``single_tensor`` (default): ONE ``all_gather_into_tensor`` into a (world * width, ...) buffer --
    RCCL's native form, and what gloo runs too, so the multi-rank tests exercise the branch a
    multi-GPU node executes; False: the reference's list ``all_gather`` (kept for backends without
    the single-tensor collective)."""
    world = len(per)
    width = max(per)
    padded = torch.zeros((width,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    padded[: rows.shape[0]] = rows
    if single_tensor:
        allrows = torch.empty((world * width,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
        dist.all_gather_into_tensor(allrows, padded)
        parts = list(allrows.split(width))
    else:
        parts = [torch.zeros_like(padded) for _ in range(world)]
        dist.all_gather(parts, padded)
    if rank != 0:
        return None
    return torch.cat([p[: per[i]] for i, p in enumerate(parts)], dim=0)
