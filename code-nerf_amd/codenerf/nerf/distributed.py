"""The multi-rank image render: shard the rays over ranks, render, gather the rows on rank 0."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.distributed as dist

from ..utils import split_sizes
from .occupancy import OccupancyGrid


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
    from . import render_rays       # looked up at call time: a caller may have replaced the package's
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
