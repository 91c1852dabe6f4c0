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

import torch  # noqa: F401

from .. import ops  # noqa: F401
from ..utils import get_minibatches, split_sizes  # noqa: F401
from .density import (_activate_gradient, _composite_normals, _normals_from_gradient,  # noqa: F401
                      density, density_gradient, density_grid, normals)
from .distributed import gather_rows, gather_views, parallel_image_render
from .fields import (_codes, _culled_field, _density_field_raw, _expand_base, _field,  # noqa: F401
                     _weight_culled_field)
from .mesh import Mesh, extract_mesh
from .occupancy import OccupancyGrid
from .point_sampler import PointSampler
from .position_embed import PositionalEmbedder
from .ray_sampler import RaySampler
from .render import forward_pass, predict_radiance_and_render, prepare_embedders, prepare_samplers, render_rays
from .scene import SceneObject, render_scene, render_scene_autograd, rigid_pose, similarity_pose
from .surface import render_surface
from .volumetric_render import volume_render

__all__ = ["RaySampler", "PointSampler", "PositionalEmbedder", "volume_render", "prepare_samplers",
           "prepare_embedders", "predict_radiance_and_render", "forward_pass", "parallel_image_render",
           "render_rays", "gather_rows", "gather_views", "density", "density_grid", "OccupancyGrid", "Mesh", "extract_mesh",
           "density_gradient", "normals", "SceneObject", "render_scene", "render_scene_autograd", "rigid_pose",
           "similarity_pose", "render_surface"]
