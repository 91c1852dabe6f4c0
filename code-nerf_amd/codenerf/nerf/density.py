"""Density queries without a view direction: sigma at points and on a grid, its gradient, and normals."""
from __future__ import annotations

from typing import Tuple

import torch

from .. import ops
from ..models.model import density_code_bias
from .fields import _check_embedders, _unwrap


def _point_rows(pts: torch.Tensor, z_s: torch.Tensor):
    """Points of any leading shape (..., 3) and their shape codes (1, C) or (pts.shape[0], C) as the density
    kernels take them -> (the leading shape, pts (n, per_row, 3) detached, the distinct code rows)."""
    assert pts.shape[-1] == 3, "pts must be (..., 3)"
    lead = tuple(pts.shape[:-1])
    n = lead[0] if lead else 1
    per_row = 1
    for k in lead[1:]:
        per_row *= k
    assert z_s.dim() == 2 and z_s.shape[0] in (1, n), "z_s must be (1, C) or one row per pts.shape[0]"
    if z_s.shape[0] > 1 and z_s.stride(0) == 0:
        z_s = z_s[:1]
    return lead, pts.detach().reshape(n, per_row, 3), z_s


def density(model, embedders, pts: torch.Tensor, z_s: torch.Tensor) -> torch.Tensor:
    """sigma_raw (model.py:174-186) at points of any leading shape (..., 3) for one shape code (1, 256) or
    one per row of the first dimension (pts.shape[0], 256) -> sigma_raw of the leading shape.  No view
    direction and no texture code enter a density.  Inference only."""
    fx, _ = _check_embedders(embedders)
    m = _unwrap(model)
    with torch.no_grad():
        lead, rows, z_s = _point_rows(pts, z_s)
        sigma = ops.density_field(m.packed(), density_code_bias(m, z_s), fx, pts=rows)
    return sigma.reshape(lead)


def density_grid(model, embedders, z_s: torch.Tensor, resolution: int, bound: float, activated: bool = True,
                 max_points: int = 1 << 22) -> torch.Tensor:
    """The density of one shape code (1, 256) on a regular grid -- the input of an iso-surface
    extraction -> (D, D, D), D = ``resolution``, axis order [ix, iy, iz], the points
    ``linspace(-bound, bound, D)`` per axis (``meshgrid(indexing="ij")``), evaluated in slabs of at
    most ``max_points`` points.  ``activated``: softplus(sigma_raw - 1), the density the renderer
    integrates (volumetric_render.py:32); else sigma_raw."""
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
    with torch.no_grad():
        lead, rows, z_s = _point_rows(pts, z_s)
        gs = _density_gradient_rows(model, embedders, z_s, None, pts=rows).reshape(lead + (4,))
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
