"""Scenes of posed objects: SceneObject, the inference and the differentiable scene render, pose builders."""
from __future__ import annotations

import functools
from typing import Dict, Optional

import torch

from .. import ops
from .fields import _check_embedders, _culled_field, _requires_grad, _unwrap
from .occupancy import OccupancyGrid, _check_sync_free
from .point_sampler import PointSampler
from .render import _hierarchical


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


def _scene_setup(objects, coarse_model, fine_model, coarse_only: bool):
    """A scene render's objects as a list and each one's coarse and fine model, its own or the scene's (no fine
    models with ``coarse_only``: there is no fine pass to run them)."""
    objects = list(objects)
    if not 1 <= len(objects) <= 8 or not all(isinstance(o, SceneObject) for o in objects):
        raise ValueError(f"a scene holds 1..8 SceneObjects, got {len(objects)} entries")
    coarse_models = [o.coarse_model if o.coarse_model is not None else coarse_model for o in objects]
    fine_models = [o.fine_model if o.fine_model is not None else fine_model for o in objects]
    if not coarse_only and any(m is None for m in fine_models):
        raise ValueError("every object needs a fine model (its own or the scene's) unless coarse_only=True")
    return objects, coarse_models, ([] if coarse_only else fine_models)


def _host_poses(objects):
    """The objects' host poses as ops.object_rays' rows -- the rotation row-major, the translation, and the scale
    when any is not 1 -- and those scales, or None when every one is 1."""
    scales = [o.scale for o in objects] if any(o.scale != 1.0 for o in objects) else None
    return [[v for row in o.rotation for v in row] + list(o.translation) + ([] if scales is None else [o.scale])
            for o in objects], scales


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
    objects, coarse_models, fine_models = _scene_setup(objects, coarse_model, fine_model, coarse_only)
    if _requires_grad([ro, rd] + [c for o in objects for c in o.codes], coarse_models + fine_models):
        raise ValueError("render_scene is an inference render: the compacted fields and the composition have no "
                         "backward (render under torch.no_grad())")
    if span_probes is not None:
        point_sampler.check_span_probes(span_probes)
    if sync_free:
        _check_sync_free(*(coarse_models + fine_models))
    n = ro.shape[0]
    rows, scales = _host_poses(objects)
    # the objects' rays (ro_k, rd_k) on first use: after the uniform coarse depths, before the span ones
    object_rays = functools.lru_cache(None)(lambda: ops.object_rays(ro, rd, rows))

    def render_pass(models, z, density_only):
        ro_k, rd_k = object_rays()
        raws = [_culled_field(m, embedders, rd_k[k], o.z_s, o.z_t, n, ro_k[k], z, o.occupancy, density_only, sync_free)
                for k, (o, m) in enumerate(zip(objects, models))]
        return ops.volume_render_compose(raws, z, rd, scales=scales)

    span = None if span_probes is None else (
        lambda t: point_sampler.sample_span(*object_rays(), [o.occupancy for o in objects], t, span_probes))
    with torch.no_grad():
        return _hierarchical(point_sampler, ro, rd, t_rand, u, coarse_only, coarse_rgb, span,
                             lambda z_c: render_pass(coarse_models, z_c, not coarse_rgb),
                             lambda z_f: render_pass(fine_models, z_f, False))[0]


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
    objects, coarse_models, fine_models = _scene_setup(objects, coarse_model, fine_model, coarse_only)
    for m in coarse_models + fine_models:
        if any(p.requires_grad for p in _unwrap(m).param_list()):
            raise ValueError("render_scene_autograd differentiates codes, rays and poses with frozen weights: a "
                             "model parameter requires grad (call model.requires_grad_(False))")
        if getattr(_unwrap(m), "precision", "f32") != "f32":
            raise ValueError(f"render_scene_autograd runs the fp32 field (precision \"f32\"), got "
                             f"{_unwrap(m).precision!r}")
    rows = scales = None
    host_rows, scale_rows = _host_poses(objects)
    if poses is None:
        rows = host_rows
    elif not (isinstance(poses, torch.Tensor) and poses.dim() == 2 and poses.shape[0] == len(objects)
              and poses.shape[1] in (12, 13) and poses.dtype == torch.float32 and poses.device == ro.device):
        raise ValueError(f"poses must be a ({len(objects)}, 12) or ({len(objects)}, 13) float32 tensor on the rays' "
                         "device")
    elif poses.shape[1] == 13:
        rows = poses.detach().cpu().tolist()            # the render's one pose read-back: the scales' host values too
        scales, scale_rows = poses[:, 12], [row[12] for row in rows]
        if not all(0.0 < v < float("inf") for v in scale_rows):
            raise ValueError(f"every scale (poses[:, 12]) must be finite and > 0, got {scale_rows}")
    elif scale_rows is not None:
        # rigid rows with the objects' constant scales: one (K, 13) tensor, no gradient into its last column
        poses = torch.cat([poses, poses.new_tensor(scale_rows)[:, None]], dim=1)
    fx, fd = _check_embedders(embedders)
    # the objects' rays on first use: after the coarse depths, render_scene's order
    object_rays = functools.lru_cache(None)(lambda: [t.unbind(0) for t in object_rays_autograd(ro, rd, poses, rows)])

    def render_pass(models, z):
        ro_k, rd_k = object_rays()
        raws = [culled_field_autograd(_unwrap(m), ro_k[k], rd_k[k], z, o.z_s, o.z_t, o.occupancy, fx, fd)
                for k, (o, m) in enumerate(zip(objects, models))]
        return volume_render_compose_autograd(raws, z, rd, scales, scale_rows)

    return _hierarchical(point_sampler, ro.detach(), rd.detach(), t_rand, u, coarse_only, True, None,
                         lambda z_c: render_pass(coarse_models, z_c), lambda z_f: render_pass(fine_models, z_f))[0]
