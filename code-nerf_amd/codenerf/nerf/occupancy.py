"""OccupancyGrid: one shape code's occupancy bits, for sample culling and ray spans."""
from __future__ import annotations

import torch

from .. import ops
from .density import density_grid
from .fields import _unwrap


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
