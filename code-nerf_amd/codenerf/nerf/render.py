"""The hierarchical render: one coarse -> resample -> fine loop, and render_rays on it."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .. import ops
from .density import _composite_normals, _density_gradient_rows, _normals_from_gradient
from .fields import (_check_embedders, _codes, _culled_field, _density_field_raw, _field, _requires_grad, _unwrap,
                     _weight_culled_field)
from .occupancy import OccupancyGrid, _check_sync_free
from .point_sampler import PointSampler
from .position_embed import PositionalEmbedder
from .ray_sampler import RaySampler
from .volumetric_render import volume_render


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


def _hierarchical(ps: PointSampler, ro, rd, t_rand, u, coarse_only: bool, coarse_rgb: bool, span, coarse_pass,
                  fine_pass):
    """The coarse -> resample -> fine loop of every render -> (the result dict, the fine pass's weights or None).
    ``ro`` / ``rd``: the rays the samplers see, detached.  ``span``: None for ops.sample_uniform's coarse depths,
    else a callable t_rand -> (z_c, ray_span, probe_range) (PointSampler.sample_span).  ``coarse_pass`` /
    ``fine_pass``: callables z -> (rgb, disp, acc, weights, depth[, acc_objects]), a field call and its composite.
    ``t_rand`` is drawn before any launch and ``u`` after the coarse pass, each only if the sampler perturbs and
    none was given; the coarse weights reach ops.sample_pdf detached."""
    n = ro.shape[0]
    if ps.perturb and t_rand is None:
        t_rand = torch.rand(n, ps.num_samples_coarse, dtype=torch.float32, device=ro.device)
    if span is None:
        _, z_c = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, t_rand if ps.perturb else None,
                                    want_pts=False)
    else:
        z_c, ray_span, probe_range = span(t_rand)
    rgb_c, disp_c, acc_c, w_c, depth_c, *obj_c = coarse_pass(z_c)
    out = {"rgb_coarse": rgb_c, "disp_coarse": disp_c, "acc_coarse": acc_c, "weights_coarse": w_c,
           "depth_coarse": depth_c, "z_coarse": z_c}
    if obj_c:
        out["acc_objects_coarse"] = obj_c[0]
    if not coarse_rgb:
        del out["rgb_coarse"]       # composited from zero colours: not a result
    if span is not None:
        out.update({"ray_span": ray_span, "ray_hit": probe_range[:, 0] >= 0})
    if coarse_only:
        return out, None
    if ps.perturb and u is None:
        u = torch.rand(n, ps.num_samples_fine, dtype=torch.float32, device=ro.device)
    _, z_f = ops.sample_pdf(ro, rd, w_c.detach()[..., 1:-1], z_c, ps.num_samples_fine, u if ps.perturb else ps.u_lin,
                            want_pts=False)
    rgb_f, disp_f, acc_f, w_f, depth_f, *obj_f = fine_pass(z_f)
    out.update({"rgb_fine": rgb_f, "disp_fine": disp_f, "acc_fine": acc_f, "depth_fine": depth_f, "z_fine": z_f})
    if obj_f:
        out["acc_objects_fine"] = obj_f[0]
    return out, w_f


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
    if (not coarse_rgb or occupancy is not None or rgb_tolerance is not None or normals) and \
            _requires_grad((ro, rd, z_s, z_t), (coarse_model, fine_model)):
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
    chunk_rows = ro.shape[0] if chunk_rows is None else chunk_rows
    ps = point_sampler
    pair = None
    paired = fine_model is not None and not coarse_only and coarse_rgb and occupancy is None and rgb_tolerance is None
    if paired:
        from ..autograd import new_field_pair, prefetch_render_prepares
        if not any(isinstance(m, torch.nn.parallel.DistributedDataParallel) for m in (coarse_model, fine_model)):
            pair = new_field_pair()     # train_minibatch: the two training backwards in shared launches

    def render_pass(model, z, fine: bool):
        """``model``'s field at the depths ``z``, in the form the render's arguments select, and its composite."""
        if paired and not fine:
            # the two differentiable fields' pre-field launches (code terms, packs, zeroed accumulators) as
            # one launch; each field takes its part (no launch when either runs without gradients)
            fx, fd = _check_embedders(embedders)
            cs, ct, code_index = _codes(z_s, z_t)
            prefetch_render_prepares(_unwrap(coarse_model), _unwrap(fine_model), rd, ro, cs, ct,
                                     ps.num_samples_coarse, ps.num_samples_coarse + ps.num_samples_fine, chunk_rows,
                                     fx, fd, code_index)
        args = (model, embedders, rd, z_s, z_t, chunk_rows)
        if events is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if fine and rgb_tolerance is not None:
            raw = _weight_culled_field(*args, ro, z, rgb_tolerance, occupancy, sync_free)
        elif occupancy is not None:
            raw = _culled_field(*args, ro, z, occupancy, not (fine or coarse_rgb), sync_free)
        else:
            # pts = ro + rd z is formed inside the field kernel (z detached, point_sampler.py:115); with
            # gradients on, the field's backward returns d ro / d rd through both the points and the view dirs
            raw = (_field if fine or coarse_rgb else _density_field_raw)(*args, ro=ro, z=z, pair=pair)
        if events is not None:
            e1.record()
            events.setdefault("field", []).append((e0, e1))
        return volume_render(raw, z, rd)

    span = None if span_probes is None else (lambda t: ps.sample_span(ro, rd, occupancy, t, span_probes))
    out, w_f = _hierarchical(ps, ro.detach(), rd.detach(), t_rand, u, coarse_only, coarse_rgb, span,
                             lambda z_c: render_pass(coarse_model, z_c, False),
                             lambda z_f: render_pass(fine_model, z_f, True))
    if normals:
        cs, _, code_index = _codes(z_s, z_t)
        with torch.no_grad():
            gs = _density_gradient_rows(fine_model, embedders, cs, code_index, ro=ro.detach(), rd=rd.detach(),
                                        z=out["z_fine"])
            out["normal_fine"] = _composite_normals(w_f, _normals_from_gradient(gs[..., :3]))
    return out


def predict_radiance_and_render(rays: Tuple[torch.Tensor, torch.Tensor], point_sampler: PointSampler,
                                embedders, coarse_model, fine_model,
                                latent_embedding: Tuple[torch.Tensor, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """nerf/__init__.py:74-91 -> (rgb_coarse, rgb_fine)."""
    ro, rd = rays
    z_s, z_t = latent_embedding
    out = render_rays(ro, rd, z_s, z_t, point_sampler, embedders, coarse_model, fine_model)
    return out["rgb_coarse"], out["rgb_fine"]
