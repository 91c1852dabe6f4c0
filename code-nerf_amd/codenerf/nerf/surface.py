"""Iso-surface ray casting: where each ray first meets a level set of the density, and what it shows there."""
from __future__ import annotations

import math
import struct
from typing import Dict, Optional

import torch

from .. import ops
from ..models.model import density_code_bias
from .density import _normals_from_gradient
from .fields import _check_embedders, _codes, _culled_field, _field, _requires_grad, _unwrap
from .occupancy import OccupancyGrid, _check_sync_free
from .point_sampler import PointSampler

MAX_REFINE = 24           # a bisection halves the bracket: 24 rounds exhaust an fp32 depth's mantissa


def _level_raw(level, activated: bool) -> float:
    """``level`` in the unit the kernels compare, sigma_raw, rounded to fp32 -- or ValueError."""
    try:
        level = float(level)
    except (TypeError, ValueError):
        raise ValueError(f"level must be a finite number, got {level!r}") from None
    if not math.isfinite(level):
        raise ValueError(f"level must be a finite number, got {level!r}")
    if activated:
        if not level > 0.0:
            raise ValueError(f"level must be > 0 with activated=True (softplus(sigma_raw - 1) is positive), got {level}")
        # the inverse of softplus(x - 1) in float64; past expm1's range log(expm1(level)) is level itself
        level = 1.0 + (math.log(math.expm1(level)) if level < 700.0 else level)
    return struct.unpack("f", struct.pack("f", level))[0]


def render_surface(ro: torch.Tensor, rd: torch.Tensor, z_s: torch.Tensor, z_t: torch.Tensor,
                   point_sampler: PointSampler, embedders, model, level: float, *, activated: bool = True,
                   refine: int = 6, z: Optional[torch.Tensor] = None, occupancy: Optional[OccupancyGrid] = None,
                   span_probes: Optional[int] = None, sync_free: bool = False, normals: bool = True,
                   background=(1.0, 1.0, 1.0)) -> Dict[str, torch.Tensor]:
    """Each ray's first crossing of the density's ``level`` set and the colour ``model`` shows there, seen along
    the ray: a crisp depth map and an oriented, coloured point per ray, from one colour evaluation per ray.

    The rule (include/codenerf.h, "Iso-surface ray casting"): the first of the ray's S search depths whose
    density is at or above the level brackets the crossing with the depth before it; ``refine`` bisections
    (an int in [0, 24]) halve the bracket, each one density evaluation per ray; the depth is then the linear
    interpolation of the level between the bracket's ends.  ``refine=0`` interpolates between the two search
    depths.  A ray that never reaches the level is a miss; one whose first search depth is already at or
    above it starts inside and reports that depth.

    ``level`` follows extract_mesh's convention: with ``activated`` it is in softplus(sigma_raw - 1) units, the
    density the renderer integrates, and must be > 0; else it is sigma_raw.  The kernels compare sigma_raw, so
    an activated level is converted once on the host, level_raw = 1 + log(expm1(level)) in float64, rounded to
    fp32; the softplus is monotone, so the crossing is the same one.
    Search depths: ``z`` (R, S) ascending, S in [2, 1024], if given; else ``point_sampler``'s coarse depths
    WITHOUT perturbation whatever ``point_sampler.perturb`` says (a surface has no use for jitter); with
    ``span_probes`` (needs ``occupancy``; render_rays' rule) the coarse depths stratified inside each ray's
    occupied span, unperturbed too, which adds "ray_span" and "ray_hit".
    ``occupancy``: the search densities come from the culled density call, a culled sample lies below every
    level and never counts as a bracket's known low end.  The kept count is read back once unless
    ``sync_free=True``, as documented for render_rays; that is the call's only host read-back: every other
    launch runs over exactly R rows whatever the rays hit (a missed ray computes harmless rows), so without a
    grid, or with ``sync_free``, the call can be captured in a graph and replayed on new inputs.

    -> "hit" (R,) int32: 0 miss, 1 crossing, 2 the ray starts at or above the level; "depth" (R,): the ray
    parameter of the crossing, +inf for a miss; "point" (R, 3) = ro + rd depth, NaN for a miss; "rgb" (R, 3):
    volume_render's colour of the field's row at the point viewed along ``rd``, ``background`` for a miss;
    "sigma" (R,): sigma_raw at the point and, with ``normals``, "normal" (R, 3), its unit normal (``normals``'
    rule), both from one density-gradient launch and both 0 for a miss; "bracket" (R, 2): the final (t_lo,
    t_hi); "z_search" (R, S).
    Inference only, models of precision "f32" only (the density kernel exists for no other); codes may be one
    row, an expand() of one, or a row per ray."""
    if isinstance(refine, bool) or not isinstance(refine, int) or not 0 <= refine <= MAX_REFINE:
        raise ValueError(f"refine must be an int in [0, {MAX_REFINE}], got {refine!r}")
    level_raw = _level_raw(level, activated)
    if _requires_grad((ro, rd, z_s, z_t, z), (model,)):
        raise ValueError("render_surface is an inference render: the per-ray search has no backward "
                         "(render under torch.no_grad(), and pass codes and depths that do not require grad)")
    ps = point_sampler
    if sync_free:
        _check_sync_free(model)
    if span_probes is not None:
        if occupancy is None:
            raise ValueError("span_probes places the search depths by the occupancy grid: pass occupancy=")
        if z is not None:
            raise ValueError("span_probes places the search depths itself: pass either z= or span_probes=")
        ps.check_span_probes(span_probes)
    n = ro.shape[0]
    if z is not None and (z.dim() != 2 or z.shape[0] != n or not 2 <= z.shape[1] <= 1024):
        raise ValueError(f"z must be (num_rays, num_samples) = ({n}, 2..1024), got {tuple(z.shape)}")
    fx, _ = _check_embedders(embedders)
    m = _unwrap(model)
    out = {}
    with torch.no_grad():
        ro, rd = ro.detach(), rd.detach()
        cs, _, code_index = _codes(z_s, z_t)
        cb = density_code_bias(m, cs)             # raises for a model of another precision
        packed = m.packed()
        if span_probes is not None:
            z, span, probe_range = ops.sample_span(ro, rd, occupancy, ps.near, ps.far, span_probes,
                                                   ps.num_samples_coarse, None)
            out.update({"ray_span": span, "ray_hit": probe_range[:, 0] >= 0})
        elif z is None:
            if not 2 <= ps.num_samples_coarse <= 1024:
                raise ValueError(f"the search needs 2..1024 depths per ray, the sampler has {ps.num_samples_coarse}")
            _, z = ops.sample_uniform(ro, rd, ps.z_vals, ps.lower, ps.upper, None, want_pts=False)
        if occupancy is None:
            raw = ops.density_field(packed, cb, fx, ro=ro, rd=rd, z=z, code_index=code_index, want_sigma=False,
                                    want_raw=True)
        else:
            raw = _culled_field(model, embedders, rd, z_s, z_t, n, ro, z, occupancy, density_only=True,
                                sync_free=sync_free)
        bracket, hit = ops.surface_bracket(raw[..., 3], z, level_raw)
        t, pts = ops.surface_step(ro, rd, hit, bracket, level_raw, finish=refine == 0)
        for i in range(refine):
            probe = ops.density_field(packed, cb, fx, pts=pts, code_index=code_index)
            ops.surface_step(ro, rd, hit, bracket, level_raw, t=t, probe=probe, finish=i == refine - 1, pts=pts)
        gs = ops.density_gradient(packed, m.packed("f32_w16_t"), cb, fx, pts=pts, code_index=code_index)
        missed = hit == 0
        field_raw = _field(model, embedders, rd, z_s, z_t, chunk_rows=n, pts=pts.view(n, 1, 3))
        rgb, depth = ops.surface_shade(field_raw, hit, t, pts, background)
        out.update({"rgb": rgb, "depth": depth, "hit": hit, "point": pts,
                    "sigma": torch.where(missed, torch.zeros_like(t), gs[:, 3]), "bracket": bracket[:, :2],
                    "z_search": z})
        if normals:
            nrm = _normals_from_gradient(gs[:, :3])
            out["normal"] = torch.where(missed[:, None], torch.zeros_like(nrm), nrm)
    return out
