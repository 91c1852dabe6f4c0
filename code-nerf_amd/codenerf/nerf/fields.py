"""The field call forms of the render: code rows, the fused field, the density kernel, and the two culled forms."""
from __future__ import annotations

import torch

from .. import ops
from ..models.model import _field_op, density_code_bias


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


def _requires_grad(tensors, models) -> bool:
    """Gradients are on and one of ``tensors`` or a parameter of one of ``models`` (Nones skipped) requires grad."""
    return torch.is_grad_enabled() and (
        any(t is not None and t.requires_grad for t in tensors) or
        any(p.requires_grad for m in models if m is not None for p in _unwrap(m).param_list()))


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
    return _field_op(_unwrap(model), cs, ct, rd, chunk_rows, fx, fd, pts=pts, ro=ro, z=z, code_index=code_index,
                     pair=pair)


def _density_field_raw(model, embedders, rd, z_s, z_t, chunk_rows, pts=None, ro=None, z=None, pair=None):
    """_field's signature on the density kernel: raw rows [0, 0, 0, sigma_raw] (render_rays'
    coarse_rgb=False).  No gradient path, and no chunk_rows: density has no view direction (Q1)."""
    fx, _ = _check_embedders(embedders)
    cs, _, code_index = _codes(z_s, z_t)
    m = _unwrap(model)
    with torch.no_grad():
        cb = density_code_bias(m, cs)
        return ops.density_field(m.packed(), cb, fx, pts=pts, ro=None if pts is not None else ro,
                                 rd=None if pts is not None else rd, z=None if pts is not None else z,
                                 code_index=code_index, want_sigma=False, want_raw=True)


def _compact_field(m, cs, ct, fx, fd, pts, vdir, code_out, density_only: bool, count, sync_free: bool):
    """The unwrapped model ``m``'s inference field in points mode over the compact rows of a cull (``pts``,
    ``vdir``, ``code_out``: ops.occupancy_cull's or ops.weight_cull's) -> raw (M, 4), or None for no rows.  The
    density kernel's raw rows when ``density_only``.  With ``sync_free`` the rows come at capacity and ``count``,
    the device row count, goes to the counted entry; else they are trimmed to the kept rows already."""
    rows = pts.shape[0]
    if not rows:
        return None
    count = count if sync_free else None
    if density_only:
        return ops.density_field(m.packed(), density_code_bias(m, cs), fx, pts=pts, code_index=code_out,
                                 want_sigma=False, want_raw=True, count=count)
    return _field_op(m, cs.detach(), ct.detach(), vdir, rows, fx, fd, pts=pts.view(rows, 1, 3), code_index=code_out,
                     count=count)


def _culled_field(model, embedders, rd, z_s, z_t, chunk_rows, ro, z, occupancy, density_only: bool,
                  sync_free: bool = False):
    """A render field call under an occupancy grid: cull -> ``model``'s inference field in points mode
    over the M' kept samples (the density kernel when ``density_only``) -> expand to raw (R, S, 4).
    Kept samples get the bits of the unculled call; culled ones the zero-density row.
    ``sync_free``: M' stays on the device -- the field runs its counted entry over the compact buffers at
    capacity and computes the first M' rows, the same bits."""
    fx, fd = _check_embedders(embedders)
    cs, ct, code_index = _codes(z_s, z_t)
    with torch.no_grad():
        count, _, pts, vdir, code_out, state = ops.occupancy_cull(
            ro.detach(), rd.detach(), z, chunk_rows, occupancy.bits, occupancy.resolution, occupancy.bound,
            code_index=code_index, want_code=cs.shape[0] > 1, sync=not sync_free)
        raw = _compact_field(_unwrap(model), cs, ct, fx, fd, pts, vdir, code_out, density_only, count, sync_free)
        return ops.occupancy_expand(raw, state)


def _weight_culled_field(model, embedders, rd, z_s, z_t, chunk_rows, ro, z, tolerance: float,
                         occupancy, sync_free: bool = False):
    """The fine field call under ``rgb_tolerance``: densities of every sample (the density kernel, under
    the grid when there is one) -> the render's own weights -> cull by weight -> ``model``'s inference
    field in points mode over the kept samples, its colours scattered into the density rows -> raw
    (R, S, 4).  Every row keeps its sigma_raw; a culled one has raw colours [0, 0, 0].
    ``sync_free``: as _culled_field's -- the kept count stays on the device for the field and the scatter."""
    fx, fd = _check_embedders(embedders)
    cs, ct, code_index = _codes(z_s, z_t)
    with torch.no_grad():
        ro, rd = ro.detach(), rd.detach()
        if occupancy is None:
            raw = _density_field_raw(model, embedders, rd, z_s, z_t, chunk_rows, ro=ro, z=z)
        else:       # the grid's empty rows have weight exactly 0: they fall out by w > 0
            raw = _culled_field(model, embedders, rd, z_s, z_t, chunk_rows, ro, z, occupancy, density_only=True,
                                sync_free=sync_free)
        weights = ops.volume_render(raw, z, rd)[3]
        eps_weight, eps_tail = ops.weight_cull_thresholds(tolerance, z.shape[1])
        count, sample_index, pts, vdir, code_out, _ = ops.weight_cull(
            weights, ro, rd, z, chunk_rows, eps_weight, eps_tail, code_index=code_index, want_code=cs.shape[0] > 1,
            sync=not sync_free)
        kept = _compact_field(_unwrap(model), cs, ct, fx, fd, pts, vdir, code_out, False, count, sync_free)
        if kept is not None:
            ops.scatter_rgb(kept, sample_index, raw, count=count if sync_free else None)
        return raw
