"""Triangle meshes of a density's iso-surface: Mesh, extract_mesh and its vertex colours."""
from __future__ import annotations

from typing import Optional

import torch

from .. import ops
from .density import density_grid, normals as _point_normals   # extract_mesh's keyword shadows the function
from .fields import _field


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
