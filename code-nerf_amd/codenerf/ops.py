"""Tensor-level wrappers of the C ABI: validate, allocate outputs, launch on the current stream.

Every function here is one entry point of include/codenerf.h; the reference
function it replaces is named in its docstring.  Inputs must be CUDA (HIP)
fp32 tensors; shape errors raise AssertionError like the reference's asserts,
and a failed launch raises ``CodeNerfError``.  Nothing here falls back to
PyTorch compute.
"""
from __future__ import annotations

import ctypes
import struct
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check, ptr, stream_of

Tensor = torch.Tensor


def _cuda(t: Tensor, name: str, dtype=torch.float32) -> Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be on a HIP device (got {t.device}); the MI355X path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype} (got {t.dtype})")
    return t.contiguous()


def _aligned16(t: Tensor) -> Tensor:
    """t itself when its data pointer is 16-B aligned (what the kernels' vector accesses need; every
    fresh allocation is), else an aligned copy (a contiguous view at an odd element offset)."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _opt(t: Optional[Tensor], name: str) -> Optional[Tensor]:
    return None if t is None else _cuda(t, name)


def _lib_ready():
    return _lib.load()


# ------------------------------------------------------------------ a field call's inputs
# The one place the field wrappers get their input checks from (field_api.hip's field_args is its C side):
# a new wrapper calls one of the two helpers below and adds what is its own.


def _freqs(freqs: Sequence[float], count: int, name: str):
    """The host float array the C side reads ``count`` floats from."""
    assert freqs is not None and len(freqs) == count, \
        f"the field kernel implements L_xyz=10, L_dir=4: {name} must have {count} entries"
    return _lib.host_floats(freqs)


def _code_rows(code_index: Optional[Tensor], n_codes: Optional[int], n: int) -> Optional[Tensor]:
    """The checked ``code_index`` (n,) int64, or without one the rule n_codes in (1, n) (n_codes None: no codes)."""
    if code_index is not None:
        code_index = _cuda(code_index, "code_index", torch.int64)
        assert code_index.shape == (n,), "code_index must be (num_rays,)"
    elif n_codes is not None:
        assert n_codes in (1, n), "codes must be one row or one row per ray"
    return code_index


def _ray_inputs(rd: Tensor, n_samples: int, freqs_xyz: Sequence[float], freqs_dir: Sequence[float],
                pts: Optional[Tensor], ro: Optional[Tensor], z: Optional[Tensor], code_index: Optional[Tensor],
                n_codes: Optional[int], n_rays: Optional[int] = None):
    """The ray form of a field call, checked: rd (R, 3) [R = n_rays where the wrapper is told it]; pts
    (R, S, 3), else ro (R, 3) and z (R, S); code_index (R,) int64, else one code row or one per ray; 10 and 4
    frequencies -> (rd, pts, ro, z, code_index, R, fx, fd): the tensors contiguous, fx / fd the host arrays."""
    rd = _cuda(rd, "rd")
    assert rd.dim() == 2 and rd.shape[1] == 3, "rd must be (num_rays, 3)"
    n = rd.shape[0]
    assert n_rays is None or n == n_rays, "rd must have one row per ray"
    if pts is not None:
        pts, ro, z = _cuda(pts, "pts"), _opt(ro, "ro"), _opt(z, "z")
        assert pts.shape == (n, n_samples, 3), "pts must be (num_rays, num_samples, 3)"
    else:
        ro, z = _cuda(ro, "ro"), _cuda(z, "z")
        assert ro.shape == (n, 3) and z.shape == (n, n_samples), \
            "ro must be (num_rays, 3) and z (num_rays, num_samples)"
    code_index = _code_rows(code_index, n_codes, n)
    return rd, pts, ro, z, code_index, n, _freqs(freqs_xyz, 10, "freqs_xyz"), _freqs(freqs_dir, 4, "freqs_dir")


def _point_inputs(freqs_xyz: Sequence[float], pts: Optional[Tensor], ro: Optional[Tensor], rd: Optional[Tensor],
                  z: Optional[Tensor], x: Optional[Tensor], code_index: Optional[Tensor], n_codes: int):
    """The density entries' form, checked: exactly one of pts (R, S, 3) or (M, 3) [R = M, S = 1]; ro, rd
    (R, 3) with z (R, S); x (M, 63) or (M, 90) encoded rows [R = M, S = 1]; the codes as in _ray_inputs; 10
    frequencies -> (pts, ro, rd, z, x, code_index, lead, R, S, fx): ``lead`` the outputs' leading shape."""
    modes = (pts is not None) + (x is not None) + (ro is not None or rd is not None or z is not None)
    assert modes == 1, "give exactly one of pts, (ro, rd, z) and x"
    if pts is not None:
        pts = _cuda(pts, "pts")
        assert pts.dim() in (2, 3) and pts.shape[-1] == 3, "pts must be (num_rays, num_samples, 3) or (M, 3)"
        lead = tuple(pts.shape[:-1])
    elif x is not None:
        x = _cuda(x, "x")
        assert x.dim() == 2 and x.shape[1] in (63, 90), "x must be (M, 63) or (M, 63 + 27)"
        lead = (x.shape[0],)
    else:
        assert ro is not None and rd is not None and z is not None, "the ray form takes ro, rd and z"
        ro, rd, z = _cuda(ro, "ro"), _cuda(rd, "rd"), _cuda(z, "z")
        assert z.dim() == 2 and ro.shape == (z.shape[0], 3) and rd.shape == (z.shape[0], 3), \
            "ro / rd must be (num_rays, 3) and z (num_rays, num_samples)"
        lead = tuple(z.shape)
    n, s = lead[0], (lead[1] if len(lead) == 2 else 1)
    return pts, ro, rd, z, x, _code_rows(code_index, n_codes, n), lead, n, s, _freqs(freqs_xyz, 10, "freqs_xyz")


def _count_arg(count: Tensor, op: str, supported: bool, form: str) -> Tensor:
    """The checked ``count`` of a counted call (include/codenerf.h): a (1,) int64 device tensor, which the
    kernel reads when it runs; ``supported``: the call is in the form the counted entries take."""
    if not supported:
        raise ValueError(f"{op}: count= (a device row count) takes {form}")
    count = _cuda(count, "count", torch.int64)
    if count.numel() != 1:
        raise ValueError(f"{op}: count must hold one int64, got shape {tuple(count.shape)}")
    return count


# ------------------------------------------------------------------ rays


def ray_directions(height: int, width: int, focal: float, cx: float, cy: float, device) -> Tensor:
    """RaySampler.__init__ directions (ray_sampler.py:35-51) -> (H, W, 3)."""
    lib = _lib_ready()
    out = torch.empty(height, width, 3, device=device, dtype=torch.float32)
    check(lib.cn_ray_directions(height, width, focal, cx, cy, ptr(out), stream_of(out)), "cn_ray_directions")
    return out


def ray_bundle(dirs: Tensor, c2w: Tensor) -> Tuple[Tensor, Tensor]:
    """RaySampler.get_bundle (ray_sampler.py:84-99): (H,W,3), (B,4,4) -> ro, rd (B,H,W,3)."""
    lib = _lib_ready()
    dirs = _cuda(dirs, "directions")
    c2w = _cuda(c2w, "tform_cam2world")
    assert c2w.dim() == 3 and c2w.shape[-2:] == (4, 4), "tform_cam2world must be (batch, 4, 4)"
    h, w = dirs.shape[0], dirs.shape[1]
    b = c2w.shape[0]
    ro = torch.empty(b, h, w, 3, device=dirs.device, dtype=torch.float32)
    rd = torch.empty_like(ro)
    check(lib.cn_ray_bundle(ptr(dirs), h * w, ptr(c2w), b, ptr(ro), ptr(rd), stream_of(dirs)), "cn_ray_bundle")
    return ro, rd


def gather_rays(ro: Tensor, rd: Tensor, select_inds: Tensor) -> Tuple[Tensor, Tensor]:
    """RaySampler.sample gather (ray_sampler.py:77-80): (B,HW,3) x2, (B,S) -> (B*S,3) x2."""
    lib = _lib_ready()
    ro, rd = _cuda(ro, "ray_origins"), _cuda(rd, "ray_directions")
    sel = _cuda(select_inds, "select_inds", torch.int64)
    b, s = sel.shape
    hw = ro.numel() // (3 * b)
    o = torch.empty(b * s, 3, device=ro.device, dtype=torch.float32)
    d = torch.empty_like(o)
    check(lib.cn_gather_rays(ptr(ro), ptr(rd), b, hw, ptr(sel), s, ptr(o), ptr(d), stream_of(o)), "cn_gather_rays")
    return o, d


# ------------------------------------------------------------------ fused pose path


def pose_rays(dirs: Tensor, theta: Optional[Tensor] = None, phi: Optional[Tensor] = None,
              rho: Optional[Tensor] = None, c2w: Optional[Tensor] = None, select_inds: Optional[Tensor] = None,
              target: Optional[Tensor] = None):
    """pose_spherical (eval.py:22-38) -> sample (ray_sampler.py:53-99) -> target gather
    (eval.py:147-148) in one launch.  theta, phi, rho (B,) each, or c2w (B,4,4); select_inds
    (B,S) int64 or None (whole bundle); target (B,HW,C) or None -> ro, rd (B*S,3), c2w (B,4,4),
    target rows (B*S,C) | None."""
    lib = _lib_ready()
    dirs = _cuda(dirs, "directions")
    hw = dirs.numel() // 3
    assert (theta is None) != (c2w is None), "give exactly one of (theta, phi, rho) and c2w"
    if theta is not None:
        theta, phi, rho = (_cuda(t, n).reshape(-1) for t, n in ((theta, "theta"), (phi, "phi"), (rho, "rho")))
        b = theta.numel()
        assert phi.numel() == b and rho.numel() == b, "theta, phi and rho must have one value per pose"
    else:
        c2w = _cuda(c2w, "tform_cam2world")
        assert c2w.dim() == 3 and c2w.shape[-2:] == (4, 4), "tform_cam2world must be (batch, 4, 4)"
        b = c2w.shape[0]
    if select_inds is not None:
        select_inds = _cuda(select_inds, "select_inds", torch.int64)
        assert select_inds.dim() == 2 and select_inds.shape[0] == b, "select_inds must be (batch, sample_size)"
        s = select_inds.shape[1]
    else:
        s = hw
    ch = 0
    tgt_out = None
    if target is not None:
        target = _cuda(target, "target")
        assert target.shape[0] == b and target.numel() % (b * hw) == 0, "target must be (batch, H*W, C)"
        ch = target.numel() // (b * hw)
        tgt_out = torch.empty(b * s, ch, device=dirs.device, dtype=torch.float32)
    ro = torch.empty(b * s, 3, device=dirs.device, dtype=torch.float32)
    rd = torch.empty_like(ro)
    c2w_out = torch.empty(b, 4, 4, device=dirs.device, dtype=torch.float32)
    check(lib.cn_pose_rays(ptr(theta), ptr(phi), ptr(rho), ptr(c2w), b, ptr(dirs), hw, ptr(select_inds), s,
                           ptr(target), ch, ptr(c2w_out), ptr(ro), ptr(rd), ptr(tgt_out), stream_of(ro)),
          "cn_pose_rays")
    return ro, rd, c2w_out, tgt_out


def pose_rays_backward(dirs: Tensor, batch: int, g_ro: Optional[Tensor], g_rd: Optional[Tensor],
                       theta: Optional[Tensor] = None, phi: Optional[Tensor] = None, rho: Optional[Tensor] = None,
                       select_inds: Optional[Tensor] = None, want_c2w: bool = False, out=None):
    """Backward of pose_rays -> (d_theta, d_phi, d_rho (B,) each | None, d_c2w (B,4,4) | None).  ``out``:
    three (B,) contiguous device tensors the angle gradients are written into (e.g. the optimiser's
    gradient slots)."""
    lib = _lib_ready()
    dirs = _cuda(dirs, "directions")
    hw = dirs.numel() // 3
    s = hw if select_inds is None else select_inds.shape[1]
    g_ro, g_rd = _opt(g_ro, "g_ro"), _opt(g_rd, "g_rd")
    angles = theta is not None
    if out is not None and angles:
        assert all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == batch for t in out)
        d = list(out)
    else:
        d = [torch.empty(batch, device=dirs.device, dtype=torch.float32) if angles else None for _ in range(3)]
    d_c2w = torch.empty(batch, 4, 4, device=dirs.device, dtype=torch.float32) if want_c2w else None
    check(lib.cn_pose_rays_backward(ptr(theta), ptr(phi), ptr(rho), batch, ptr(dirs), hw, ptr(select_inds), s,
                                    ptr(g_ro), ptr(g_rd), ptr(d_c2w), ptr(d[0]), ptr(d[1]), ptr(d[2]),
                                    stream_of(dirs)), "cn_pose_rays_backward")
    return (d[0], d[1], d[2]), d_c2w


def random_select(batch: int, hw: int, sample_size: int, seed: int, offset: int, device) -> Tensor:
    """On-device np.random.permutation(hw)[:sample_size] per image (ray_sampler.py:41-42, same
    distribution; Philox4x32-10) -> (batch, sample_size) int64."""
    lib = _lib_ready()
    out = torch.empty(batch, sample_size, device=device, dtype=torch.int64)
    check(lib.cn_random_select(batch, hw, sample_size, seed & (2 ** 64 - 1), offset & (2 ** 64 - 1), ptr(out),
                               stream_of(out)), "cn_random_select")
    return out


def pose_error(gt_c2w: Tensor, cam_c2w: Tensor) -> Tuple[Tensor, Tensor]:
    """eval.py:161-162: (SE3.Log(inverse(gt) @ cam) (B,6), its 2-norm (B,))."""
    lib = _lib_ready()
    gt, cam = _cuda(gt_c2w, "gt_pose").reshape(-1, 4, 4), _cuda(cam_c2w, "cam_pose").reshape(-1, 4, 4)
    assert gt.shape == cam.shape, "poses must both be (batch, 4, 4)"
    b = gt.shape[0]
    twist = torch.empty(b, 6, device=gt.device, dtype=torch.float32)
    err = torch.empty(b, device=gt.device, dtype=torch.float32)
    check(lib.cn_pose_error(ptr(gt), ptr(cam), b, ptr(twist), ptr(err), stream_of(gt)), "cn_pose_error")
    return twist, err


# ------------------------------------------------------------------ points


def sample_uniform(ro: Tensor, rd: Tensor, z_bins: Tensor, lower: Tensor, upper: Tensor,
                   t_rand: Optional[Tensor] = None, want_pts: bool = True):
    """PointSampler.sample_uniform (point_sampler.py:49-71) -> pts (R,Nc,3) | None, z (R,Nc)."""
    lib = _lib_ready()
    ro, rd = _cuda(ro, "ro"), _cuda(rd, "rd")
    n, nc = ro.shape[0], z_bins.shape[-1]
    if t_rand is not None:
        t_rand = _cuda(t_rand, "t_rand")
        assert t_rand.shape == (n, nc), "t_rand must be (num_rays, num_coarse)"
    z = torch.empty(n, nc, device=ro.device, dtype=torch.float32)
    pts = torch.empty(n, nc, 3, device=ro.device, dtype=torch.float32) if want_pts else None
    if n:      # no rays: empty outputs, as torch's ops give (the C ABI refuses n_rays == 0)
        check(lib.cn_sample_uniform(ptr(ro), ptr(rd), n, ptr(z_bins), ptr(lower), ptr(upper), nc, ptr(t_rand),
                                    ptr(z), ptr(pts), stream_of(z)), "cn_sample_uniform")
    return pts, z


def ray_points(ro: Tensor, rd: Tensor, z: Tensor) -> Tensor:
    """pts = ro + rd * z (point_sampler.py:70, :118): (R,3) x2, (R,S) -> (R,S,3)."""
    lib = _lib_ready()
    ro, rd, z = _cuda(ro, "ro"), _cuda(rd, "rd"), _cuda(z, "z_vals")
    n, s = z.shape
    assert ro.shape == (n, 3) and rd.shape == (n, 3), "ro / rd must be (num_rays, 3)"
    pts = torch.empty(n, s, 3, device=z.device, dtype=torch.float32)
    if n * s:
        check(lib.cn_ray_points(ptr(ro), ptr(rd), ptr(z), n, s, ptr(pts), stream_of(z)), "cn_ray_points")
    return pts


def sample_pdf(ro: Tensor, rd: Tensor, weights: Tensor, z: Tensor, num_fine: int,
               u: Optional[Tensor] = None, want_pts: bool = True):
    """PointSampler.sample_pdf (point_sampler.py:73-120) -> pts (R,Nc+Nf,3) | None, z (R,Nc+Nf).

    ``weights`` may be the strided view ``w[..., 1:-1]`` of a contiguous (R, Nc) tensor;
    ``u`` is (R, Nf) per-ray draws or one (Nf,) row shared by every ray.
    """
    lib = _lib_ready()
    ro, rd, z = _cuda(ro, "ro"), _cuda(rd, "rd"), _cuda(z, "z_vals")
    n, nc = z.shape
    assert nc - 2 == weights.shape[-1], f"Weights size {weights.shape} should match {nc - 1}"
    if weights.device.type != "cuda" or weights.dtype != torch.float32 or weights.stride(-1) != 1:
        weights = _cuda(weights, "weights")
    w_stride = weights.stride(0)
    u_stride = 0
    if u is not None:
        u = _cuda(u, "u")
        assert u.shape in ((n, num_fine), (num_fine,)), "u must be (num_rays, num_fine) or (num_fine,)"
        u_stride = num_fine if u.dim() == 2 else 0
    zo = torch.empty(n, nc + num_fine, device=z.device, dtype=torch.float32)
    pts = torch.empty(n, nc + num_fine, 3, device=z.device, dtype=torch.float32) if want_pts else None
    if n:
        check(lib.cn_sample_pdf(ptr(ro), ptr(rd), ptr(weights), w_stride, ptr(z), n, nc, num_fine, ptr(u), u_stride,
                                ptr(zo), ptr(pts), stream_of(zo)), "cn_sample_pdf")
    return pts, zo


# ------------------------------------------------------------------ encoding


def posenc(x: Tensor, freqs: Sequence[float], include_input: bool) -> Tensor:
    """PositionalEmbedder.embed (position_embed.py:35-53): (M, D) -> (M, D*(inc + 2L))."""
    lib = _lib_ready()
    x = _cuda(x, "tensor")
    assert x.dim() == 2, "tensor must be (N, num_dim)"
    m, d = x.shape
    out = torch.empty(m, d * (int(include_input) + 2 * len(freqs)), device=x.device, dtype=torch.float32)
    if m:
        check(lib.cn_posenc(ptr(x), m, d, _lib.host_floats(freqs), len(freqs), int(include_input), ptr(out),
                            stream_of(x)), "cn_posenc")
    return out


# ------------------------------------------------------------------ volume integration


def volume_render(raw: Tensor, z: Tensor, rd: Tensor, want_weights: bool = True):
    """volume_render (volumetric_render.py:36-66) -> rgb, disp, acc, weights, depth."""
    lib = _lib_ready()
    raw, z, rd = _cuda(raw, "radiance_field"), _cuda(z, "depth_values"), _cuda(rd, "ray_directions")
    raw, z = _aligned16(raw), _aligned16(z)
    n, s = z.shape
    assert raw.shape == (n, s, 4), "radiance_field must be (num_rays, num_samples, 4)"
    assert rd.shape == (n, 3), "ray_directions must be (num_rays, 3)"
    dev = raw.device
    rgb = torch.empty(n, 3, device=dev, dtype=torch.float32)
    disp = torch.empty(n, device=dev, dtype=torch.float32)
    acc = torch.empty_like(disp)
    depth = torch.empty_like(disp)
    w = torch.empty(n, s, device=dev, dtype=torch.float32) if want_weights else None
    if n:
        check(lib.cn_volume_render(ptr(raw), ptr(z), ptr(rd), n, s, ptr(rgb), ptr(disp), ptr(acc), ptr(w), ptr(depth),
                                   stream_of(raw)), "cn_volume_render")
    if w is not None and s == 1:
        w = w[:, :0]          # the reference's S == 1 weights are (R, 0) (see volume.hip)
    return rgb, disp, acc, w, depth


def _scale_values(scales, k: int) -> list:
    """K uniform scales as host floats, each finite and > 0."""
    vals = [float(v) for v in scales]
    assert len(vals) == k, f"scales must hold one value per object ({k}), got {len(vals)}"
    assert all(v > 0.0 and v != float("inf") for v in vals), f"every scale must be finite and > 0, got {vals}"
    return vals


def volume_render_compose(raws: Sequence[Tensor], z: Tensor, rd: Tensor, want_weights: bool = True,
                          want_acc_objects: bool = True, scales=None):
    """Several objects' raw rows at the same depths as one ray integral (cn_volume_render_compose; the rule
    is in include/codenerf.h): ``raws`` 1..8 tensors (R, S, 4), ``z`` (R, S), the world ``rd`` (R, 3) ->
    rgb, disp, acc, weights, depth as volume_render, and acc_objects (K, R): each object's share of acc, its
    instance mask.  One object gives volume_render's bits.  ``scales``: K host floats, the objects' uniform
    scales (cn_volume_render_compose_scaled: object k's density is divided by scales[k]); all 1 gives the
    unscaled bits."""
    lib = _lib_ready()
    raws = list(raws)
    assert 1 <= len(raws) <= _lib.CN_MAX_SCENE_OBJECTS, \
        f"a scene holds 1..{_lib.CN_MAX_SCENE_OBJECTS} objects, got {len(raws)}"
    if scales is not None:
        scales = _scale_values(scales, len(raws))
    z, rd = _aligned16(_cuda(z, "depth_values")), _cuda(rd, "ray_directions")
    n, s = z.shape
    raws = [_aligned16(_cuda(raw, f"raws[{k}]")) for k, raw in enumerate(raws)]
    for raw in raws:
        assert raw.shape == (n, s, 4), "every radiance field must be (num_rays, num_samples, 4)"
    assert rd.shape == (n, 3), "ray_directions must be (num_rays, 3)"
    dev = z.device
    rgb = torch.empty(n, 3, device=dev, dtype=torch.float32)
    disp = torch.empty(n, device=dev, dtype=torch.float32)
    acc = torch.empty_like(disp)
    depth = torch.empty_like(disp)
    w = torch.empty(n, s, device=dev, dtype=torch.float32) if want_weights else None
    acc_objects = torch.empty(len(raws), n, device=dev, dtype=torch.float32) if want_acc_objects else None
    if n:
        pointers, keep = _lib.pointer_array(raws)
        if scales is None:
            check(lib.cn_volume_render_compose(pointers, len(raws), ptr(z), ptr(rd), n, s, ptr(rgb), ptr(disp),
                                               ptr(acc), ptr(w), ptr(depth), ptr(acc_objects), stream_of(z)),
                  "cn_volume_render_compose")
        else:
            check(lib.cn_volume_render_compose_scaled(pointers, _lib.host_floats(scales), len(raws), ptr(z), ptr(rd), n,
                                                      s, ptr(rgb), ptr(disp), ptr(acc), ptr(w), ptr(depth),
                                                      ptr(acc_objects), stream_of(z)),
                  "cn_volume_render_compose_scaled")
        del keep
    if w is not None and s == 1:
        w = w[:, :0]          # as volume_render: the reference's S == 1 weights are (R, 0)
    return rgb, disp, acc, w, depth, acc_objects


def _pose_rows(poses) -> Tuple[list, int]:
    """K poses as host floats and their width: each a (rotation (3, 3), translation (3,)) pair or a row of 12 (R
    row-major, then t) -- width 12 -- or a (rotation, translation, scale) triple or a row of 13 -- width 13, a
    similarity pose; with any of these every pose becomes 13 floats (a rigid one gets scale 1)."""
    poses = list(poses)
    assert 1 <= len(poses) <= _lib.CN_MAX_SCENE_OBJECTS, \
        f"a scene holds 1..{_lib.CN_MAX_SCENE_OBJECTS} objects, got {len(poses)}"
    all_rows = []
    for pose in poses:
        pose = list(pose)
        if len(pose) in (2, 3):
            rot, t = pose[:2]
            rows = [float(v) for row in rot for v in row] + [float(v) for v in t]
            assert len(rows) == 12, "a pose is a (3, 3) rotation and a (3,) translation"
            rows += [float(pose[2])] if len(pose) == 3 else []
        else:
            rows = [float(v) for v in pose]
        assert len(rows) in (12, 13), "a pose is a (3, 3) rotation, a (3,) translation and an optional scale"
        all_rows.append(rows)
    width = max(len(rows) for rows in all_rows)
    flat = [v for rows in all_rows for v in rows + [1.0] * (width - len(rows))]
    if width == 13:
        _scale_values(flat[12::13], len(poses))
    return flat, width


def object_rays(ro: Tensor, rd: Tensor, poses) -> Tuple[Tensor, Tensor]:
    """World rays (R, 3) in the frames of K posed objects (cn_object_rays) -> ro (K, R, 3), rd (K, R, 3).
    ``poses``: K host (rotation (3, 3) row-major object-to-world, translation (3,)) pairs of floats, or K rows of
    12 (the rotation row-major, then the translation); the ray parameter is unchanged, so ro[k] + z rd[k] is the
    world point ro + z rd in object k's frame.  (rotation, translation, scale) triples or rows of 13 are similarity
    poses (cn_object_rays_scaled): the object-frame rays are divided by the scale, the ray parameter still
    unchanged; scale 1 gives the rigid pose's bits."""
    lib = _lib_ready()
    ro, rd = _cuda(ro, "ro"), _cuda(rd, "rd")
    n = ro.shape[0]
    assert ro.shape == (n, 3) and rd.shape == (n, 3), "ro / rd must be (num_rays, 3)"
    flat, width = _pose_rows(poses)
    k = len(flat) // width
    ro_out = torch.empty(k, n, 3, device=ro.device, dtype=torch.float32)
    rd_out = torch.empty(k, n, 3, device=ro.device, dtype=torch.float32)
    if n:
        entry, name = ((lib.cn_object_rays, "cn_object_rays") if width == 12 else
                       (lib.cn_object_rays_scaled, "cn_object_rays_scaled"))
        check(entry(ptr(ro), ptr(rd), n, _lib.host_floats(flat), k, ptr(ro_out), ptr(rd_out), stream_of(ro)), name)
    return ro_out, rd_out


# ------------------------------------------------------------------ MLP


def _fmt(precision: str) -> int:
    if precision not in _lib.FORMATS:
        raise ValueError(f"precision must be one of {sorted(_lib.FORMATS)}, got {precision!r}")
    return _lib.FORMATS[precision]


def mlp_packed_floats(precision: str = "f32") -> int:
    return int(_lib_ready().cn_mlp_packed_floats(_fmt(precision)))


def mlp_pack(params: Sequence[Tensor], precision: str = "f32") -> Tensor:
    """Pack a CodeNeRFModel state_dict (model.py:145-156, state_dict order) for the field kernel.

    precision "f32": fp32 fragments for v_mfma_f32_32x32x2_f32; "bf16x3": bf16 hi/lo
    fragments for the 3-product split on v_mfma_f32_32x32x16_bf16 (include/codenerf.h);
    "bf16x3_t": the transposed 3xbf16 pack of the fused backward; "f32_w16_fold": the "f32_w16"
    pack with fc_out's feature rows folded into layer_dir1 (frozen-weight inference; read by
    mlp_forward / radiance_field together with fold_bias rows); "f16": fp16 fragments (weights rounded
    to nearest even) for the one-product inference kernel on v_mfma_f32_32x32x16_f16.
    """
    lib = _lib_ready()
    assert len(params) == _lib.CN_NUM_PARAMS, "expected the 18 CodeNeRFModel weight/bias tensors"
    params = [_cuda(p.detach(), f"param{i}") for i, p in enumerate(params)]
    out = torch.empty(mlp_packed_floats(precision), device=params[0].device, dtype=torch.float32)
    arr, keep = _lib.pointer_array(params)
    check(lib.cn_mlp_pack(arr, _fmt(precision), ptr(out), stream_of(out)), "cn_mlp_pack")
    del keep
    return out


def code_bias(params: Sequence[Tensor], z_s: Tensor, z_t: Tensor) -> Tensor:
    """Per-code folded terms of CodeNeRFModel.forward (model.py:174-192) -> (n_codes, 520)."""
    lib = _lib_ready()
    params = [_cuda(p.detach(), f"param{i}") for i, p in enumerate(params)]
    z_s, z_t = _cuda(z_s.detach(), "z_s"), _cuda(z_t.detach(), "z_t")
    assert z_s.shape == z_t.shape and z_s.dim() == 2 and z_s.shape[1] == 256, "codes must be (n, 256)"
    out = torch.empty(z_s.shape[0], _lib.CN_CODE_BIAS_STRIDE, device=z_s.device, dtype=torch.float32)
    arr, keep = _lib.pointer_array(params)
    check(lib.cn_code_bias(arr, ptr(z_s), ptr(z_t), z_s.shape[0], ptr(out), stream_of(out)), "cn_code_bias")
    del keep
    return out


def fold_bias(params: Sequence[Tensor], cb: Tensor) -> Tensor:
    """The folded layer's per-code bias (cn_fold_bias): W_dir1[:, :256] c_feat + b_dir1 for every row of
    ``cb`` = code_bias(params, z_s, z_t), accumulated in double and rounded once -> (n_codes, 256)."""
    lib = _lib_ready()
    params = [_cuda(p.detach(), f"param{i}") for i, p in enumerate(params)]
    cb = _cuda(cb, "cb")
    assert cb.dim() == 2 and cb.shape[1] == _lib.CN_CODE_BIAS_STRIDE, "cb must be code_bias rows (n, 520)"
    out = torch.empty(cb.shape[0], 256, device=cb.device, dtype=torch.float32)
    arr, keep = _lib.pointer_array(params)
    check(lib.cn_fold_bias(arr, ptr(cb), cb.shape[0], ptr(out), stream_of(out)), "cn_fold_bias")
    del keep
    return out


def _fold_rows(precision: str, cb: Tensor, fold: Optional[Tensor]) -> Optional[Tensor]:
    """The checked ``fold_bias`` argument of a forward: required by "f32_w16_fold", refused by the rest."""
    if precision != "f32_w16_fold":
        assert fold is None, f"fold_bias goes with precision 'f32_w16_fold', not {precision!r}"
        return None
    assert fold is not None, "precision 'f32_w16_fold' needs fold_bias = ops.fold_bias(params, cb)"
    fold = _cuda(fold, "fold_bias")
    assert fold.shape == (cb.shape[0], 256), "fold_bias must be (n_codes, 256)"
    return fold


def field_prepare(params: Sequence[Tensor], z_s: Tensor, z_t: Tensor, pack: bool = True, pack_t: bool = True,
                  n_zero: int = 0):
    """cn_field_prepare: code_bias(params, z_s, z_t), the fp32 forward / backward packs ("f32_w16",
    "f32_w16_t"; each only if asked) and a zeroed (n_zero,) buffer in ONE launch -> (cb, packed or None,
    packed_t or None, zero or None); bitwise the separate calls' outputs."""
    lib = _lib_ready()
    params = [_cuda(p.detach(), f"param{i}") for i, p in enumerate(params)]
    z_s, z_t = _cuda(z_s.detach(), "z_s"), _cuda(z_t.detach(), "z_t")
    assert z_s.shape == z_t.shape and z_s.dim() == 2 and z_s.shape[1] == 256, "codes must be (n, 256)"
    dev = z_s.device
    cb = torch.empty(z_s.shape[0], _lib.CN_CODE_BIAS_STRIDE, device=dev, dtype=torch.float32)
    nf = mlp_packed_floats("f32_w16")
    packed = torch.empty(nf, device=dev, dtype=torch.float32) if pack else None
    packed_t = torch.empty(nf, device=dev, dtype=torch.float32) if pack_t else None
    zero = torch.empty(n_zero, device=dev, dtype=torch.float32) if n_zero else None
    arr, keep = _lib.pointer_array(params)
    check(lib.cn_field_prepare(arr, ptr(z_s), ptr(z_t), z_s.shape[0], ptr(cb), ptr(packed), ptr(packed_t), ptr(zero),
                               n_zero, stream_of(cb)), "cn_field_prepare")
    del keep
    return cb, packed, packed_t, zero


def field_prepare_models(models: Sequence[Tuple[Sequence[Tensor], bool, bool, int]], z_s: Tensor, z_t: Tensor,
                         want_act: bool = False):
    """cn_field_prepare_models: field_prepare for one or two models (params, pack, pack_t, n_zero) on the
    same codes in ONE launch -> [(cb, packed or None, packed_t or None, zero or None)] per model; bitwise
    each model's field_prepare.  ``want_act``: each tuple also carries the code-layer activations
    (n_codes, 768) (code_ds_outer's operand) as a fifth entry."""
    lib = _lib_ready()
    assert 1 <= len(models) <= 2, "one or two models"
    z_s, z_t = _cuda(z_s.detach(), "z_s"), _cuda(z_t.detach(), "z_t")
    assert z_s.shape == z_t.shape and z_s.dim() == 2 and z_s.shape[1] == 256, "codes must be (n, 256)"
    dev = z_s.device
    nf = mlp_packed_floats("f32_w16")
    outs, keep = [], []
    preps = (_lib.FieldPrep * len(models))()
    for k, (params, pack, pack_t, n_zero) in enumerate(models):
        params = [_cuda(p.detach(), f"param{i}") for i, p in enumerate(params)]
        cb = torch.empty(z_s.shape[0], _lib.CN_CODE_BIAS_STRIDE, device=dev, dtype=torch.float32)
        packed = torch.empty(nf, device=dev, dtype=torch.float32) if pack else None
        packed_t = torch.empty(nf, device=dev, dtype=torch.float32) if pack_t else None
        zero = torch.empty(n_zero, device=dev, dtype=torch.float32) if n_zero else None
        act = torch.empty(z_s.shape[0], 768, device=dev, dtype=torch.float32) if want_act else None
        arr, k_arr = _lib.pointer_array(params)
        keep += [params, arr, k_arr]
        preps[k] = _lib.FieldPrep(arr, ptr(cb), ptr(packed), ptr(packed_t), ptr(zero), n_zero, ptr(act))
        outs.append((cb, packed, packed_t, zero, act) if want_act else (cb, packed, packed_t, zero))
    check(lib.cn_field_prepare_models(preps, len(models), ptr(z_s), ptr(z_t), z_s.shape[0], stream_of(z_s)),
          "cn_field_prepare_models")
    del keep
    return outs


def xenc_columns():
    """The fp32 training forward's encoding plane (cn_field_train_saved_floats): column c' (0..63) ->
    PositionalEmbedder column (position_embed.py:44-53), -1 for the padding slot (mlp_common.h
    xenc_col: lane group g = c' // 16 holds layer_xyz1's k-steps t = c' % 16)."""
    out = []
    for cp in range(64):
        t, g = cp & 15, cp >> 4
        i, p = t & 7, 4 * (t & 7) + g
        if p < 30:
            out.append((3 if t < 8 else 6) + 6 * (p // 3) + p % 3)
        else:
            out.append((0 if g == 2 else 2) if t < 8 else (1 if g == 2 else -1))
    return out


def mlp_forward(packed: Tensor, cb: Tensor, x: Tensor, code_index: Optional[Tensor] = None,
                precision: str = "f32", fold_bias: Optional[Tensor] = None) -> Tensor:
    """CodeNeRFModel.forward on pre-encoded rows (model.py:160-194): (M, 90) -> (M, 4).
    precision "f32_w16_fold": ``packed`` that format's pack and ``fold_bias`` = ops.fold_bias(params, cb)."""
    lib = _lib_ready()
    fold = _fold_rows(precision, cb, fold_bias)
    x = _cuda(x, "x")
    assert x.dim() == 2 and x.shape[1] == 90, "x must be (M, 63 + 27)"
    m = x.shape[0]
    n_codes = cb.shape[0]
    if code_index is not None:
        code_index = _cuda(code_index, "code_index", torch.int64)
    else:
        assert n_codes in (1, m), "codes must be one row or one row per sample"
    raw = torch.empty(m, 4, device=x.device, dtype=torch.float32)
    if m and fold is not None:
        check(lib.cn_mlp_forward_fold(ptr(packed), _fmt(precision), ptr(cb), ptr(fold), ptr(code_index), n_codes,
                                      ptr(x), m, ptr(raw), stream_of(x)), "cn_mlp_forward_fold")
    elif m:
        check(lib.cn_mlp_forward(ptr(packed), _fmt(precision), ptr(cb), ptr(code_index), n_codes, ptr(x), m, ptr(raw),
                                 stream_of(x)),
              "cn_mlp_forward")
    return raw


# The fewest samples per ray at which the folded kernel reads its view-direction term from a per-ray
# table (cn_view_rows + cn_radiance_field_fold_rows) instead of computing it per sample.  A ray's row
# costs one 1 KiB store and S 1 KiB loads against S x (7 of 223 k-steps of matrix work + the direction's
# normalisation and encoding): at S = 1 (the culled renders' compact lists) the table is a pure loss.
# Measured on MI355X at 2^21 samples per launch, table build included, table / in-kernel time
# (profiles/viewrows/crossover.json): S = 1 1.082, 2 1.031, 4 1.000, 8 0.986, 16 0.977, 32 0.975, 64 0.975.
VIEW_ROWS_MIN_SAMPLES = 8


def view_rows(packed: Tensor, fold_bias: Tensor, rd: Tensor, freqs_dir: Sequence[float]) -> Tensor:
    """cn_view_rows: per ray, fold_bias row 0 + W_dir1[:, 256:] enc(rd / |rd|) -> (R, 256), bit for bit
    what the folded kernel's accumulators hold after its view-direction chunk.  ``packed``: the
    "f32_w16_fold" pack."""
    lib = _lib_ready()
    packed, fold_bias, rd = _cuda(packed, "packed"), _cuda(fold_bias, "fold_bias"), _cuda(rd, "rd")
    assert fold_bias.dim() == 2 and fold_bias.shape[1] == 256, "fold_bias must be (n_codes, 256)"
    assert rd.dim() == 2 and rd.shape[1] == 3, "rd must be (num_rays, 3)"
    assert len(freqs_dir) == 4, "the field kernel implements L_dir=4"
    n = rd.shape[0]
    nbytes = lib.cn_view_rows_bytes(n) if n else 0
    assert nbytes >= 0, "cn_view_rows_bytes refused the ray count"
    rows = torch.empty(nbytes // 4, device=rd.device, dtype=torch.float32).view(n, 256)
    if n:
        check(lib.cn_view_rows(ptr(packed), _fmt("f32_w16_fold"), ptr(fold_bias), ptr(rd), n,
                               _lib.host_floats(freqs_dir), ptr(rows), stream_of(rd)), "cn_view_rows")
    return rows


_view_rows_table = view_rows   # radiance_field's keyword of the same name shadows the function there


def radiance_field(packed: Tensor, cb: Tensor, rd: Tensor, n_samples: int, chunk_rows: int,
                   freqs_xyz: Sequence[float], freqs_dir: Sequence[float], pts: Optional[Tensor] = None,
                   ro: Optional[Tensor] = None, z: Optional[Tensor] = None,
                   code_index: Optional[Tensor] = None, precision: str = "f32",
                   fold_bias: Optional[Tensor] = None, view_rows: Optional[bool] = None,
                   count: Optional[Tensor] = None) -> Tensor:
    """forward_pass (nerf/__init__.py:94-134) fused with the MLP -> raw (R, S, 4).
    ``count`` (a (1,) int64 device tensor, e.g. occupancy_cull(sync=False)'s): the counted entries
    (cn_radiance_field_counted / _fold_counted) -- R is the capacity, only the first min(max(count, 0), R)
    rows are computed and written (the rest of ``raw`` stays uninitialised) and nothing is read back.
    Points form with n_samples = 1, precision "f32_w16" or "f32_w16_fold", one code row or ``code_index``,
    no view-rows table: ValueError otherwise.
    precision "f32_w16_fold": ``packed`` that format's pack and ``fold_bias`` = ops.fold_bias(params, cb).
    ``view_rows`` (that precision only): read layer_dir1's view-direction term from a per-ray table built
    here (ops.view_rows) instead of computing it per sample -- the same bits.  None: where it pays, i.e.
    geometry from rays, one code row, no code_index and n_samples >= VIEW_ROWS_MIN_SAMPLES; True forces it
    (one code row without code_index required), False forces the in-kernel path."""
    lib = _lib_ready()
    fold = _fold_rows(precision, cb, fold_bias)
    assert not view_rows or fold is not None, "view_rows goes with precision 'f32_w16_fold'"
    n_codes = cb.shape[0]
    rd, pts, ro, z, code_index, n, fx, fd = _ray_inputs(rd, n_samples, freqs_xyz, freqs_dir, pts, ro, z, code_index,
                                                        n_codes)
    raw = torch.empty(n, n_samples, 4, device=rd.device, dtype=torch.float32)
    one_code = n_codes == 1 and code_index is None
    if count is not None:
        count = _count_arg(count, "radiance_field", pts is not None and n_samples == 1 and not view_rows and
                           precision in ("f32_w16", "f32_w16_fold") and (one_code or code_index is not None),
                           "the points form with n_samples=1, precision 'f32_w16' or 'f32_w16_fold', one code row "
                           "or code_index, and no view_rows table")
        if n and fold is not None:
            check(lib.cn_radiance_field_fold_counted(ptr(packed), _fmt(precision), ptr(cb), ptr(fold), ptr(code_index),
                                                     n_codes, ptr(pts), None, ptr(rd), None, n, 1, ptr(count), fx, fd,
                                                     ptr(raw), stream_of(rd)), "cn_radiance_field_fold_counted")
        elif n:
            check(lib.cn_radiance_field_counted(ptr(packed), _fmt(precision), ptr(cb), ptr(code_index), n_codes,
                                                ptr(pts), None, ptr(rd), None, n, 1, ptr(count), fx, fd, ptr(raw),
                                                stream_of(rd)), "cn_radiance_field_counted")
        return raw
    if view_rows is None:
        view_rows = fold is not None and pts is None and one_code and n_samples >= VIEW_ROWS_MIN_SAMPLES
    elif view_rows:
        if not one_code:
            raise ValueError("view_rows=True needs one code row and no code_index: a table row holds code row 0's "
                             "c_v1")
    if n and fold is not None and view_rows:
        rows = _view_rows_table(packed, fold, rd, freqs_dir)
        check(lib.cn_radiance_field_fold_rows(ptr(packed), _fmt(precision), ptr(cb), ptr(fold), ptr(rows), None, 1,
                                              ptr(pts), ptr(ro), ptr(rd), ptr(z), n, n_samples, chunk_rows, fx, fd,
                                              ptr(raw), stream_of(rd)), "cn_radiance_field_fold_rows")
    elif n and fold is not None:
        check(lib.cn_radiance_field_fold(ptr(packed), _fmt(precision), ptr(cb), ptr(fold), ptr(code_index), n_codes,
                                         ptr(pts), ptr(ro), ptr(rd), ptr(z), n, n_samples, chunk_rows, fx, fd,
                                         ptr(raw), stream_of(rd)), "cn_radiance_field_fold")
    elif n:
        check(lib.cn_radiance_field(ptr(packed), _fmt(precision), ptr(cb), ptr(code_index), n_codes, ptr(pts), ptr(ro),
                                    ptr(rd), ptr(z), n, n_samples, chunk_rows, fx, fd, ptr(raw), stream_of(rd)),
              "cn_radiance_field")
    return raw


def density_field(packed: Tensor, cb: Tensor, freqs_xyz: Sequence[float], *, pts: Optional[Tensor] = None,
                  ro: Optional[Tensor] = None, rd: Optional[Tensor] = None, z: Optional[Tensor] = None,
                  x: Optional[Tensor] = None, code_index: Optional[Tensor] = None, want_sigma: bool = True,
                  want_raw: bool = False, count: Optional[Tensor] = None):
    """sigma_raw of CodeNeRFModel.forward alone (model.py:174-186; cn_density_field): the fp32 field
    kernel's first 10 weight chunks, bitwise the sigma_raw radiance_field gives for the same points.
    ``count`` (a (1,) int64 device tensor): cn_density_field_counted, as radiance_field's -- ``pts`` (M, 3)
    at capacity, one code row or ``code_index``, the first min(max(count, 0), M) rows written; ValueError
    for the ray form, encoded rows or (R, S, 3) points.

    Exactly one input: ``pts`` (R, S, 3) or (M, 3) [R = M, S = 1]; ``ro``, ``rd`` (R, 3) with ``z`` (R, S);
    ``x`` (M, 63) or (M, 90) encoded rows [R = M, S = 1].  ``packed``: the "f32_w16" pack; ``cb`` one code
    row, one per R, or rows picked by ``code_index`` (R,) (the texture half of ``cb`` is not read).
    -> sigma (R, S) / (M,), or raw (.., 4) rows [0, 0, 0, sigma_raw] (what volume_render and
    sample_pdf take), or (sigma, raw) when both are asked for."""
    lib = _lib_ready()
    assert want_sigma or want_raw, "ask for sigma, raw or both"
    n_codes = cb.shape[0]
    pts, ro, rd, z, x, code_index, lead, n, s, fx = _point_inputs(freqs_xyz, pts, ro, rd, z, x, code_index, n_codes)
    dev = (pts if pts is not None else x if x is not None else z).device
    sigma = torch.empty(lead, device=dev, dtype=torch.float32) if want_sigma else None
    raw = torch.empty(lead + (4,), device=dev, dtype=torch.float32) if want_raw else None
    if count is not None:
        count = _count_arg(count, "density_field", pts is not None and pts.dim() == 2 and
                           (n_codes == 1 or code_index is not None),
                           "pts (M, 3) with one code row or code_index")
        if n:
            check(lib.cn_density_field_counted(ptr(packed), _lib.CN_FMT_F32_W16, ptr(cb), ptr(code_index), n_codes,
                                               ptr(pts), None, None, None, n, 1, ptr(count), fx, ptr(sigma), ptr(raw),
                                               stream_of(cb)), "cn_density_field_counted")
    elif n * s:    # no samples: empty outputs without a launch (the C ABI refuses sizes of 0)
        check(lib.cn_density_field(ptr(packed), _lib.CN_FMT_F32_W16, ptr(cb), ptr(code_index), n_codes, ptr(pts),
                                   ptr(ro), ptr(rd), ptr(z), ptr(x), 0 if x is None else x.shape[1], n, s, fx,
                                   ptr(sigma), ptr(raw), stream_of(cb)), "cn_density_field")
    if want_sigma and want_raw:
        return sigma, raw
    return sigma if want_sigma else raw


def density_gradient(packed: Tensor, packed_t: Tensor, cb: Tensor, freqs_xyz: Sequence[float], *,
                     pts: Optional[Tensor] = None, ro: Optional[Tensor] = None, rd: Optional[Tensor] = None,
                     z: Optional[Tensor] = None, code_index: Optional[Tensor] = None) -> Tensor:
    """d sigma_raw / d point and sigma_raw in one launch (cn_density_gradient) -> (.., 4) rows
    [d/dx, d/dy, d/dz, sigma_raw]: column 3 is bitwise density_field's sigma, columns 0..2 equal the d_pts
    of radiance_field_masks + field_backward_x3(precision="f32") on d_raw = (0, 0, 0, 1).

    Exactly one input: ``pts`` (R, S, 3) or (M, 3) [R = M, S = 1]; ``ro``, ``rd`` (R, 3) with ``z`` (R, S):
    the gradient is taken at ro + rd z, with respect to that point.  ``packed``: the "f32_w16" pack,
    ``packed_t``: the "f32_w16_t" pack of the same parameters; ``cb`` one code row, one per R, or rows picked
    by ``code_index`` (R,)."""
    lib = _lib_ready()
    n_codes = cb.shape[0]
    pts, ro, rd, z, _, code_index, lead, n, s, fx = _point_inputs(freqs_xyz, pts, ro, rd, z, None, code_index, n_codes)
    out = torch.empty(lead + (4,), device=(pts if pts is not None else z).device, dtype=torch.float32)
    if n * s:      # no samples: an empty output without a launch (the C ABI refuses sizes of 0)
        check(lib.cn_density_gradient(ptr(packed), ptr(packed_t), _lib.CN_FMT_F32_W16, _lib.CN_FMT_F32_W16_T, ptr(cb),
                                      ptr(code_index), n_codes, ptr(pts), ptr(ro), ptr(rd), ptr(z), n, s, fx,
                                      ptr(out), stream_of(cb)), "cn_density_gradient")
    return out


# ------------------------------------------------------------------ occupancy-grid culling


def _grid_scale(resolution: int, bound: float) -> Tuple[float, float]:
    """(lo, inv_cell) of the point lookup (include/codenerf.h): -bound and G / (2 bound), which the
    ctypes call rounds to fp32."""
    return -float(bound), resolution / (2.0 * float(bound))


def occupancy_build(nodes: Tensor, threshold: float, dilate: int = 1) -> Tensor:
    """Occupancy bits from node densities (cn_occupancy_build): ``nodes`` (G+1, G+1, G+1), axis order
    [ix, iy, iz] -- what nerf.density_grid(resolution=G + 1) returns -> int32 words (G^3 / 32,).  A cell
    is occupied iff a node within ``dilate`` (0..2) cells of it is > ``threshold`` or NaN."""
    lib = _lib_ready()
    nodes = _cuda(nodes, "nodes")
    assert nodes.dim() == 3 and nodes.shape[0] == nodes.shape[1] == nodes.shape[2], "nodes must be (G+1, G+1, G+1)"
    g = nodes.shape[0] - 1
    assert g % 32 == 0 and 32 <= g <= 512, "the grid resolution G must be a multiple of 32 in [32, 512]"
    assert dilate in (0, 1, 2), "dilate must be 0, 1 or 2"
    bits = torch.empty(g * g * g // 32, device=nodes.device, dtype=torch.int32)
    check(lib.cn_occupancy_build(ptr(nodes), g, float(threshold), int(dilate), ptr(bits), stream_of(nodes)),
          "cn_occupancy_build")
    return bits


def occupancy_cull(ro: Tensor, rd: Tensor, z: Tensor, chunk_rows: int, bits: Tensor, resolution: int, bound: float,
                   code_index: Optional[Tensor] = None, want_code: bool = True, sync: bool = True):
    """Test every ray sample against an occupancy grid and compact the occupied ones
    (cn_occupancy_cull) -> (count, sample_index (M',) int32, pts (M', 3), vdir (M', 3), code_out (M',)
    int64 or None, state), M' = ``count`` samples in ascending sample order.  ``vdir`` holds the
    unnormalised rd row of each sample's Q1 view-direction ray and ``code_out`` its code row
    (``code_index[r]``, or r): with rd=vdir, n_samples=1, chunk_rows=M' the rows are a points-mode
    input of radiance_field / density_field.  ``state`` goes to occupancy_expand.

    This is the one place that reads ``count`` back (``.item()``): a HOST SYNCHRONISATION, since the
    field launch over the compact rows is sized by it.  A culled render is therefore not
    graph-capturable, although the C ABI entries themselves are stream-ordered and are -- unless
    ``sync=False``: nothing is read back, ``count`` is the (1,) int64 device tensor, the compact outputs
    come at full capacity (R S rows, the first ``count`` written) and go with ``count=`` to
    radiance_field / density_field / scatter_rgb; ``state`` is one occupancy_expand accepts for a
    compact result of that capacity."""
    lib = _lib_ready()
    ro, rd, z = _cuda(ro, "ro"), _cuda(rd, "rd"), _cuda(z, "z_vals")
    bits = _cuda(bits, "bits", torch.int32)
    assert z.dim() == 2, "z must be (num_rays, num_samples)"
    n, s = z.shape
    assert ro.shape == (n, 3) and rd.shape == (n, 3), "ro / rd must be (num_rays, 3)"
    g = int(resolution)
    assert g % 32 == 0 and 32 <= g <= 512 and bits.shape == (g * g * g // 32,), \
        "bits must be the (G^3 / 32,) words of a grid of resolution G, a multiple of 32 in [32, 512]"
    if code_index is not None:
        code_index = _cuda(code_index, "code_index", torch.int64)
        assert code_index.shape == (n,), "code_index must be (num_rays,)"
    dev = z.device
    m = n * s
    sample_index = torch.empty(m, device=dev, dtype=torch.int32)
    pts = torch.empty(m, 3, device=dev, dtype=torch.float32)
    vdir = torch.empty(m, 3, device=dev, dtype=torch.float32)
    code_out = torch.empty(m, device=dev, dtype=torch.int64) if want_code else None
    if m == 0:
        return (0 if sync else torch.zeros(1, device=dev, dtype=torch.int64)), sample_index, pts, vdir, code_out, \
            (None, n, s, 0)
    ws_bytes = lib.cn_occupancy_cull_workspace_bytes(n, s)
    if ws_bytes < 0:
        raise ValueError(f"occupancy_cull: {n} rays x {s} samples is outside 1..512 samples / 2^31 - 1 rows")
    workspace = torch.empty((ws_bytes + 7) // 8, device=dev, dtype=torch.int64)
    count = torch.empty(1, device=dev, dtype=torch.int64)
    lo, inv_cell = _grid_scale(g, bound)
    check(lib.cn_occupancy_cull(ptr(ro), ptr(rd), ptr(z), n, s, int(chunk_rows), ptr(code_index), ptr(bits), g, lo,
                                inv_cell, ptr(workspace), ptr(count), ptr(sample_index), ptr(pts), ptr(vdir),
                                ptr(code_out), stream_of(z)), "cn_occupancy_cull")
    if not sync:
        return count, sample_index, pts, vdir, code_out, (workspace, n, s, m)
    k = int(count.item())       # host synchronisation (see the docstring)
    return (k, sample_index[:k], pts[:k], vdir[:k], None if code_out is None else code_out[:k],
            (workspace, n, s, k))


def occupancy_expand(raw_compact: Optional[Tensor], state) -> Tensor:
    """The compact field result (M', 4) back at its samples (cn_occupancy_expand) -> raw (R, S, 4);
    culled slots hold [0, 0, 0, CN_EMPTY_SIGMA_RAW]: exactly zero density.  ``state``: occupancy_cull's;
    ``raw_compact`` may be None when that call kept nothing."""
    lib = _lib_ready()
    workspace, n, s, k = state
    if raw_compact is not None:
        raw_compact = _aligned16(_cuda(raw_compact, "raw_compact").reshape(-1, 4))
        assert raw_compact.shape[0] == k, f"raw_compact must hold the {k} kept rows"
    else:
        assert k == 0, f"raw_compact is required: {k} samples were kept"
    dev = workspace.device if workspace is not None else torch.device("cuda")
    raw = torch.empty(n, s, 4, device=dev, dtype=torch.float32)
    if n * s:
        check(lib.cn_occupancy_expand(ptr(raw_compact), ptr(workspace), n, s, ptr(raw), stream_of(raw)),
              "cn_occupancy_expand")
    return raw


def _grid_triples(grids) -> list:
    """``grids`` as a list of (bits, resolution, bound): one grid or a sequence of them, each a triple or an
    object with those attributes (nerf.OccupancyGrid)."""
    def one(g):
        if hasattr(g, "bits"):
            return g.bits, g.resolution, g.bound
        return tuple(g)
    if hasattr(grids, "bits") or (isinstance(grids, (tuple, list)) and len(grids) == 3
                                  and isinstance(grids[0], torch.Tensor)):
        return [one(grids)]
    return [one(g) for g in grids]


def sample_span(ro: Tensor, rd: Tensor, grids, near: float, far: float, n_probes: int, nc: int,
                t_rand: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Per-ray depth spans from occupancy grids and the coarse depths stratified inside them (cn_sample_span;
    the rule is in include/codenerf.h) -> z (R, Nc), span (R, 2) = (t_lo, t_hi), probe_range (R, 2) int32 =
    (first, last) occupied probe, (-1, -1) for a ray that meets no occupied cell (it keeps [near, far]).
    ``ro`` / ``rd``: (R, 3) for one grid, or (K, R, 3) for K grids, each object's rays in its own frame
    (object_rays).  ``grids``: one grid or K of them, each (bits, resolution, bound) or an object with those
    attributes.  ``n_probes``: a multiple of 64 in [64, 1024]; ``nc`` in [2, 512]; ``t_rand`` (R, Nc) as
    sample_uniform's (its last column is not read).  One launch, graph-capturable."""
    lib = _lib_ready()
    ro, rd = _cuda(ro, "ro"), _cuda(rd, "rd")
    triples = _grid_triples(grids)
    k = len(triples)
    assert 1 <= k <= _lib.CN_MAX_SCENE_OBJECTS, f"a scene holds 1..{_lib.CN_MAX_SCENE_OBJECTS} objects, got {k}"
    if ro.dim() == 2:
        assert k == 1, "ro / rd (num_rays, 3) go with one grid: K grids take (K, num_rays, 3)"
        ro, rd = ro.unsqueeze(0), rd.unsqueeze(0)
    n = ro.shape[1]
    assert ro.shape == (k, n, 3) and rd.shape == (k, n, 3), "ro / rd must be (num_grids, num_rays, 3)"
    n_probes, nc, near, far = int(n_probes), int(nc), float(near), float(far)
    assert n_probes % 64 == 0 and 64 <= n_probes <= 1024, "n_probes must be a multiple of 64 in [64, 1024]"
    assert 2 <= nc <= 512, "nc must be in [2, 512]"
    assert 0.0 <= near < far < float("inf"), "near / far must be finite with 0 <= near < far"
    bits_list, res, lo, inv = [], [], [], []
    for j, (bits, resolution, bound) in enumerate(triples):
        bits = _cuda(bits, f"grids[{j}].bits", torch.int32)
        g = int(resolution)
        assert g % 32 == 0 and 32 <= g <= 512 and bits.shape == (g * g * g // 32,), \
            "bits must be the (G^3 / 32,) words of a grid of resolution G, a multiple of 32 in [32, 512]"
        assert float(bound) > 0.0 and float(bound) < float("inf"), "a grid's bound must be positive and finite"
        l, i = _grid_scale(g, bound)
        bits_list.append(bits)
        res.append(g)
        lo.append(l)
        inv.append(i)
    if t_rand is not None:
        t_rand = _cuda(t_rand, "t_rand")
        assert t_rand.shape == (n, nc), "t_rand must be (num_rays, num_coarse)"
    dev = ro.device
    z = torch.empty(n, nc, device=dev, dtype=torch.float32)
    span = torch.empty(n, 2, device=dev, dtype=torch.float32)
    probe_range = torch.empty(n, 2, device=dev, dtype=torch.int32)
    if n:
        pointers, keep = _lib.pointer_array(bits_list)
        check(lib.cn_sample_span(ptr(ro), ptr(rd), n, pointers, (ctypes.c_int64 * k)(*res), _lib.host_floats(lo),
                                 _lib.host_floats(inv), k, near, far, n_probes, nc, ptr(t_rand), ptr(z), ptr(span),
                                 ptr(probe_range), stream_of(z)), "cn_sample_span")
        del keep
    return z, span, probe_range


# ------------------------------------------------------------------ iso-surface ray casting


def _strided_density(t: Tensor, name: str, shape) -> Tuple[Tensor, int]:
    """A density the surface entries read in place -> (the tensor, its element stride 1 or 4): ``t`` of ``shape``,
    contiguous, or column 3 of contiguous (.., 4) raw rows (``raw[..., 3]``); anything else is copied."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be on a HIP device (got {t.device}); the MI355X path has no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be {torch.float32} (got {t.dtype})")
    assert tuple(t.shape) == tuple(shape), f"{name} must be {tuple(shape)}"
    if not t.is_contiguous():
        rows = 4
        for k in reversed(range(t.dim())):
            if t.shape[k] != 1 and t.stride(k) != rows:
                return t.contiguous(), 1
            rows *= t.shape[k]
        return t, 4
    return t, 1


def _out(t: Optional[Tensor], name: str, shape, dtype, device) -> Tensor:
    """A caller's output buffer, checked, or a fresh one."""
    if t is None:
        return torch.empty(shape, device=device, dtype=dtype)
    assert isinstance(t, torch.Tensor) and t.device == device and t.dtype == dtype and \
        tuple(t.shape) == tuple(shape) and t.is_contiguous(), f"{name} must be a contiguous {dtype} {tuple(shape)}"
    return t


def surface_bracket(sigma: Tensor, z: Tensor, level: float, bracket: Optional[Tensor] = None,
                    hit: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Each ray's first crossing of ``sigma >= level`` among its search depths (cn_surface_bracket; the rule is in
    include/codenerf.h) -> bracket (R, 4) = [t_lo, t_hi, s_lo, s_hi], hit (R,) int32: 0 no crossing (both ends
    the last sample), 2 the first sample is at or above the level (both ends sample 0), 1 a crossing between
    samples j - 1 and j.  ``sigma`` (R, S): contiguous, or ``raw[..., 3]`` of contiguous (R, S, 4) rows, read in
    place; ``z`` (R, S) ascending; S in [2, 1024]; ``level`` finite, in sigma's unit.  ``bracket`` / ``hit``:
    buffers to write instead of fresh ones.  One launch, graph-capturable."""
    lib = _lib_ready()
    z = _cuda(z, "z")
    assert z.dim() == 2, "z must be (num_rays, num_samples)"
    n, s = z.shape
    sigma, stride = _strided_density(sigma, "sigma", (n, s))
    level = float(level)
    assert 2 <= s <= 1024, "num_samples must be in [2, 1024]"
    assert level == level and abs(level) != float("inf"), "level must be finite"
    bracket = _out(bracket, "bracket", (n, 4), torch.float32, z.device)
    hit = _out(hit, "hit", (n,), torch.int32, z.device)
    if n:
        check(lib.cn_surface_bracket(ptr(sigma), stride, ptr(z), n, s, level, ptr(bracket), ptr(hit), stream_of(z)),
              "cn_surface_bracket")
    return bracket, hit


def surface_step(ro: Tensor, rd: Tensor, hit: Tensor, bracket: Tensor, level: float, t: Optional[Tensor] = None,
                 probe: Optional[Tensor] = None, finish: bool = False,
                 pts: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """One round of the per-ray bisection (cn_surface_step) -> (t (R,), pts (R, 3) = ro + rd t).  ``bracket`` (R, 4)
    from surface_bracket is updated IN PLACE, and so is ``t`` when given.  ``probe`` (R,): the density at the
    previous call's ``t`` (contiguous, or ``raw[..., 3]`` of contiguous (R, .., 4) rows), which replaces the end
    of the bracket on its side of ``level`` where hit == 1; None on the first call, which only places ``t``.
    Then t = the bracket's midpoint, or with ``finish`` the linear interpolation of ``level`` between its ends
    (t_hi where the low end's density is unknown or the ends' densities do not rise).  One launch."""
    lib = _lib_ready()
    ro, rd, hit = _cuda(ro, "ro"), _cuda(rd, "rd"), _cuda(hit, "hit", torch.int32)
    n = hit.shape[0]
    assert hit.shape == (n,) and ro.shape == (n, 3) and rd.shape == (n, 3), \
        "hit must be (num_rays,) and ro / rd (num_rays, 3)"
    level = float(level)
    assert level == level and abs(level) != float("inf"), "level must be finite"
    bracket = _out(bracket, "bracket", (n, 4), torch.float32, ro.device)
    assert bracket.data_ptr() % 16 == 0, "bracket must be 16-byte aligned"
    stride = 1
    if probe is not None:
        assert t is not None, "probe is the density at the previous call's t: pass that t"
        probe, stride = _strided_density(probe, "probe", (n,))
    t = _out(t, "t", (n,), torch.float32, ro.device)
    pts = _out(pts, "pts", (n, 3), torch.float32, ro.device)
    if n:
        check(lib.cn_surface_step(ptr(ro), ptr(rd), ptr(hit), ptr(probe), stride, level, int(bool(finish)), n,
                                  ptr(bracket), ptr(t), ptr(pts), stream_of(ro)), "cn_surface_step")
    return t, pts


def surface_shade(raw: Tensor, hit: Tensor, t: Tensor, pts: Tensor, background=(1.0, 1.0, 1.0),
                  rgb: Optional[Tensor] = None, depth: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """The surface render's outputs from the field's rows at the final points (cn_surface_shade) -> (rgb (R, 3),
    depth (R,)).  A ray with hit != 0 shows sigmoid(raw[:3]) * 1.002 - 0.001, volume_render's colour of a raw row,
    at depth ``t``; a ray with hit == 0 shows ``background`` at depth +inf, and its row of ``pts`` (R, 3), written
    IN PLACE, becomes NaN.  ``raw`` (R, 4) or (R, 1, 4).  One launch."""
    lib = _lib_ready()
    raw, hit, t = _cuda(raw, "raw"), _cuda(hit, "hit", torch.int32), _cuda(t, "t")
    n = hit.shape[0]
    assert hit.shape == (n,) and t.shape == (n,) and raw.numel() == 4 * n and raw.shape[-1] == 4, \
        "hit and t must be (num_rays,) and raw (num_rays, 4)"
    raw = _aligned16(raw)
    bg = [float(v) for v in background]
    assert len(bg) == 3, "background must be three floats"
    pts = _out(pts, "pts", (n, 3), torch.float32, raw.device)
    rgb = _out(rgb, "rgb", (n, 3), torch.float32, raw.device)
    depth = _out(depth, "depth", (n,), torch.float32, raw.device)
    if n:
        check(lib.cn_surface_shade(ptr(raw), ptr(hit), ptr(t), _lib.host_floats(bg), n, ptr(rgb), ptr(depth),
                                   ptr(pts), stream_of(raw)), "cn_surface_shade")
    return rgb, depth


# ------------------------------------------------------------------ iso-surface extraction


def isosurface(nodes: Tensor, iso: float, axis: Tensor) -> Tuple[Tensor, Tensor]:
    """The ``iso`` level set of a node grid as a triangle mesh (cn_isosurface_count / cn_isosurface_emit;
    include/codenerf.h states the semantics): ``nodes`` (N, N, N), axis order [ix, iy, iz] -- what
    nerf.density_grid returns -- and ``axis`` (N,) node coordinates, used on all three axes ->
    (vertices (V, 3) float32, faces (T, 3) int32).  Marching tetrahedra on the Kuhn split of each cell:
    one vertex per sign-changing edge in ascending (node, direction) order, faces in ascending (cell,
    tetrahedron, triangle) order with normals towards the lower values; a node is inside iff its value
    is > ``iso``.  Deterministic, no atomics.

    The two totals are read back once (``.item()``) between the count and the emit: a HOST
    SYNCHRONISATION, since the outputs are allocated to exactly that size.  With V = 0 both results are
    empty and nothing is emitted."""
    lib = _lib_ready()
    nodes, axis = _cuda(nodes, "nodes"), _cuda(axis, "axis")
    assert nodes.dim() == 3 and nodes.shape[0] == nodes.shape[1] == nodes.shape[2], "nodes must be (N, N, N)"
    n = nodes.shape[0]
    assert axis.shape == (n,), "axis must be (N,)"
    iso = float(iso)
    if iso != iso or iso in (float("inf"), float("-inf")):
        raise ValueError(f"isosurface: iso must be finite (got {iso})")
    ws_bytes = lib.cn_isosurface_workspace_bytes(n)
    if ws_bytes < 0:
        raise ValueError(f"isosurface: N = {n} is outside 2..513")
    dev = nodes.device
    workspace = torch.empty((ws_bytes + 7) // 8, device=dev, dtype=torch.int64)
    counts = torch.empty(2, device=dev, dtype=torch.int64)
    st = stream_of(nodes)
    check(lib.cn_isosurface_count(ptr(nodes), n, iso, ptr(workspace), ptr(counts), st), "cn_isosurface_count")
    n_vertices, n_faces = (int(k) for k in counts.tolist())       # host synchronisation (see the docstring)
    vertices = torch.empty(n_vertices, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(n_faces, 3, device=dev, dtype=torch.int32)
    if n_vertices:
        check(lib.cn_isosurface_emit(ptr(nodes), ptr(axis), n, iso, ptr(workspace), n_vertices, n_faces,
                                     ptr(vertices), ptr(faces) if n_faces else None, st), "cn_isosurface_emit")
    return vertices, faces


# ------------------------------------------------------------------ weight-bounded colour culling


def float32_floor(x: float) -> float:
    """The largest float32 <= ``x`` (x finite, >= 0), as a Python float."""
    f = struct.unpack("<f", struct.pack("<f", x))[0]          # round to nearest
    if f > x:
        f = struct.unpack("<f", struct.pack("<I", struct.unpack("<I", struct.pack("<f", f))[0] - 1))[0]
    return f


def weight_cull_thresholds(tolerance: float, n_samples: int) -> Tuple[float, float]:
    """(eps_weight, eps_tail) of a colour tolerance on a ray of ``n_samples`` samples (include/codenerf.h):
    the largest float32 <= tol / (2 S), and tol / 2; the culled weights of a ray then sum to <= tol."""
    return float32_floor(tolerance / (2.0 * n_samples)), tolerance / 2.0


def weight_cull(weights: Tensor, ro: Tensor, rd: Tensor, z: Tensor, chunk_rows: int, eps_weight: float,
                eps_tail: float, code_index: Optional[Tensor] = None, want_code: bool = True, sync: bool = True):
    """Compact the samples whose volume-render weight can matter (cn_weight_cull): sample i of a ray is
    kept iff w_i > 0, w_i >= eps_weight (fp32) and the double sum of w_i.. >= eps_tail; NaN fails.
    ``weights`` (R, S) as volume_render returns them -> occupancy_cull's tuple (count, sample_index,
    pts, vdir, code_out or None, state), the kept samples in ascending order; ``state`` is valid for
    occupancy_expand.

    Like occupancy_cull, this reads ``count`` back once (``.item()``): a HOST SYNCHRONISATION, since
    the field launch over the kept rows is sized by it -- unless ``sync=False``, which returns the device
    ``count`` and full-capacity outputs as occupancy_cull's does."""
    lib = _lib_ready()
    weights = _cuda(weights, "weights")
    ro, rd, z = _cuda(ro, "ro"), _cuda(rd, "rd"), _cuda(z, "z_vals")
    assert z.dim() == 2, "z must be (num_rays, num_samples)"
    n, s = z.shape
    assert weights.shape == (n, s), "weights must be (num_rays, num_samples)"
    assert ro.shape == (n, 3) and rd.shape == (n, 3), "ro / rd must be (num_rays, 3)"
    eps_weight, eps_tail = float(eps_weight), float(eps_tail)
    if not (eps_weight >= 0.0 and eps_tail >= 0.0):
        raise ValueError(f"weight_cull: thresholds must be >= 0 and not NaN (got {eps_weight}, {eps_tail})")
    if code_index is not None:
        code_index = _cuda(code_index, "code_index", torch.int64)
        assert code_index.shape == (n,), "code_index must be (num_rays,)"
    dev = z.device
    m = n * s
    sample_index = torch.empty(m, device=dev, dtype=torch.int32)
    pts = torch.empty(m, 3, device=dev, dtype=torch.float32)
    vdir = torch.empty(m, 3, device=dev, dtype=torch.float32)
    code_out = torch.empty(m, device=dev, dtype=torch.int64) if want_code else None
    if m == 0:
        return (0 if sync else torch.zeros(1, device=dev, dtype=torch.int64)), sample_index, pts, vdir, code_out, \
            (None, n, s, 0)
    ws_bytes = lib.cn_occupancy_cull_workspace_bytes(n, s)
    if ws_bytes < 0:
        raise ValueError(f"weight_cull: {n} rays x {s} samples is outside 1..512 samples / 2^31 - 1 rows")
    workspace = torch.empty((ws_bytes + 7) // 8, device=dev, dtype=torch.int64)
    count = torch.empty(1, device=dev, dtype=torch.int64)
    check(lib.cn_weight_cull(ptr(weights), ptr(ro), ptr(rd), ptr(z), n, s, int(chunk_rows), ptr(code_index),
                             eps_weight, eps_tail, ptr(workspace), ptr(count), ptr(sample_index), ptr(pts), ptr(vdir),
                             ptr(code_out), stream_of(z)), "cn_weight_cull")
    if not sync:
        return count, sample_index, pts, vdir, code_out, (workspace, n, s, m)
    k = int(count.item())       # host synchronisation (see the docstring)
    return (k, sample_index[:k], pts[:k], vdir[:k], None if code_out is None else code_out[:k],
            (workspace, n, s, k))


def scatter_rgb(raw_compact: Tensor, sample_index: Tensor, raw: Tensor, count: Optional[Tensor] = None) -> Tensor:
    """The colours of the compact field rows (M', 4) into ``raw`` (.., 4) IN PLACE (cn_scatter_rgb):
    components 0..2 of row ``sample_index[j]`` from compact row j; component 3 (sigma_raw) and every
    other row stay as they are -> ``raw``.  Nothing is launched when no row was kept.
    ``count`` (a (1,) int64 device tensor): cn_scatter_rgb_counted -- ``raw_compact`` and ``sample_index``
    at capacity, the first min(max(count, 0), capacity) rows scattered, the others' indices not read."""
    lib = _lib_ready()
    sample_index = _cuda(sample_index, "sample_index", torch.int32)
    k = sample_index.shape[0]
    assert raw.is_cuda and raw.dtype == torch.float32 and raw.is_contiguous() and raw.shape[-1] == 4 and \
        raw.data_ptr() % 16 == 0, "raw must be a contiguous, 16-B aligned (.., 4) float32 device tensor"
    n_slots = raw.numel() // 4
    assert sample_index.dim() == 1 and k <= n_slots, "sample_index must be (M',) with M' <= raw's rows"
    if k == 0:
        return raw
    raw_compact = _aligned16(_cuda(raw_compact, "raw_compact").reshape(-1, 4))
    assert raw_compact.shape[0] == k, f"raw_compact must hold the {k} kept rows"
    if count is not None:
        count = _count_arg(count, "scatter_rgb", True, "")
        check(lib.cn_scatter_rgb_counted(ptr(raw_compact), ptr(sample_index), ptr(count), k, ptr(raw), n_slots,
                                         stream_of(raw)), "cn_scatter_rgb_counted")
        return raw
    check(lib.cn_scatter_rgb(ptr(raw_compact), ptr(sample_index), k, ptr(raw), n_slots, stream_of(raw)),
          "cn_scatter_rgb")
    return raw


# ------------------------------------------------------------------ backward (A14)


def volume_render_backward(raw: Tensor, z: Tensor, rd: Tensor, g_rgb=None, g_disp=None, g_acc=None,
                           g_weights=None, g_depth=None, want_rd: bool = True,
                           d_rd_into: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """Gradient of volume_render (volumetric_render.py:36-66) -> d_raw (R,S,4), d_rd (R,3) or None.
    ``d_rd_into`` (a contiguous (R, 3) device tensor): d rd ADDED into it (accumulate_rd) and returned."""
    lib = _lib_ready()
    raw, z, rd = _cuda(raw, "radiance_field"), _cuda(z, "depth_values"), _cuda(rd, "ray_directions")
    raw, z = _aligned16(raw), _aligned16(z)
    n, s = z.shape
    assert raw.shape == (n, s, 4) and rd.shape == (n, 3)
    g_rgb, g_disp, g_acc, g_depth = (_opt(g_rgb, "g_rgb"), _opt(g_disp, "g_disp"), _opt(g_acc, "g_acc"),
                                     _opt(g_depth, "g_depth"))
    if g_weights is not None and g_weights.shape[-1] != s:   # S == 1: the reference's weights are (R, 0)
        g_weights = None
    g_weights = _opt(g_weights, "g_weights")
    d_raw = torch.empty_like(raw)
    if d_rd_into is not None:
        assert d_rd_into.is_cuda and d_rd_into.is_contiguous() and d_rd_into.shape == (n, 3)
        d_rd = d_rd_into
    else:
        d_rd = torch.empty_like(rd) if want_rd else None
    if n == 0:      # no rays: empty gradients (the C ABI refuses n_rays == 0), as the forward
        return d_raw, d_rd
    check(lib.cn_volume_render_backward(ptr(raw), ptr(z), ptr(rd), n, s, ptr(g_rgb), ptr(g_disp), ptr(g_acc),
                                        ptr(g_weights), ptr(g_depth), ptr(d_raw), ptr(d_rd),
                                        int(d_rd_into is not None), stream_of(raw)), "cn_volume_render_backward")
    return d_raw, d_rd


def volume_render_compose_backward(raws: Sequence[Tensor], z: Tensor, rd: Tensor, g_rgb=None, g_disp=None, g_acc=None,
                                   g_weights=None, g_depth=None, g_acc_objects=None, want_rd: bool = True,
                                   d_rd_into: Optional[Tensor] = None, scales=None, want_scales: bool = False):
    """Gradient of volume_render_compose (cn_volume_render_compose_backward; the rule is in include/codenerf.h)
    -> (d_raws: one (R, S, 4) tensor per object, d_rd (R, 3) or None).  The upstream gradients as
    volume_render_backward's, plus ``g_acc_objects`` (K, R); ``d_rd_into``: d rd ADDED into it and returned.
    ``scales``: the forward's K host scales (cn_volume_render_compose_scaled_backward); with ``want_scales`` a
    third result, d_scales (K,), the gradient w.r.t. the scales through the densities (a fixed reduction order:
    two runs give the same bits)."""
    lib = _lib_ready()
    raws = list(raws)
    assert 1 <= len(raws) <= _lib.CN_MAX_SCENE_OBJECTS, \
        f"a scene holds 1..{_lib.CN_MAX_SCENE_OBJECTS} objects, got {len(raws)}"
    assert scales is not None or not want_scales, "want_scales needs the forward's scales"
    if scales is not None:
        scales = _scale_values(scales, len(raws))
    z, rd = _aligned16(_cuda(z, "depth_values")), _cuda(rd, "ray_directions")
    n, s = z.shape
    raws = [_aligned16(_cuda(raw, f"raws[{k}]")) for k, raw in enumerate(raws)]
    for raw in raws:
        assert raw.shape == (n, s, 4), "every radiance field must be (num_rays, num_samples, 4)"
    assert rd.shape == (n, 3), "ray_directions must be (num_rays, 3)"
    g_rgb, g_disp, g_acc, g_depth = (_opt(g_rgb, "g_rgb"), _opt(g_disp, "g_disp"), _opt(g_acc, "g_acc"),
                                     _opt(g_depth, "g_depth"))
    if g_weights is not None and g_weights.shape[-1] != s:   # S == 1: the reference's weights are (R, 0)
        g_weights = None
    g_weights, g_acc_objects = _opt(g_weights, "g_weights"), _opt(g_acc_objects, "g_acc_objects")
    assert g_rgb is None or g_rgb.shape == (n, 3), "g_rgb must be (num_rays, 3)"
    assert all(g is None or g.shape == (n,) for g in (g_disp, g_acc, g_depth)), "g_disp / g_acc / g_depth must be (num_rays,)"
    assert g_weights is None or g_weights.shape == (n, s), "g_weights must be (num_rays, num_samples)"
    assert g_acc_objects is None or g_acc_objects.shape == (len(raws), n), "g_acc_objects must be (num_objects, num_rays)"
    d_raws = [torch.empty_like(raw) for raw in raws]
    if d_rd_into is not None:
        assert d_rd_into.is_cuda and d_rd_into.is_contiguous() and d_rd_into.shape == (n, 3)
        d_rd = d_rd_into
    else:
        d_rd = torch.empty_like(rd) if want_rd else None
    d_scales = torch.empty(len(raws), device=z.device, dtype=torch.float32) if want_scales else None
    if n == 0:      # no rays: empty gradients (the C ABI refuses n_rays == 0), as the forward
        return (d_raws, d_rd, d_scales.zero_()) if want_scales else (d_raws, d_rd)
    pointers, keep = _lib.pointer_array(raws)
    outs, keep_outs = _lib.pointer_array(d_raws)
    if scales is None:
        check(lib.cn_volume_render_compose_backward(pointers, len(raws), ptr(z), ptr(rd), n, s, ptr(g_rgb), ptr(g_disp),
                                                    ptr(g_acc), ptr(g_weights), ptr(g_depth), ptr(g_acc_objects), outs,
                                                    ptr(d_rd), int(d_rd_into is not None), stream_of(z)),
              "cn_volume_render_compose_backward")
    else:
        workspace = None
        if want_scales:
            workspace = torch.empty(lib.cn_volume_render_compose_scaled_backward_workspace_floats(n, s, len(raws)),
                                    device=z.device, dtype=torch.float32)
        check(lib.cn_volume_render_compose_scaled_backward(
            pointers, _lib.host_floats(scales), len(raws), ptr(z), ptr(rd), n, s, ptr(g_rgb), ptr(g_disp), ptr(g_acc),
            ptr(g_weights), ptr(g_depth), ptr(g_acc_objects), outs, ptr(d_rd), int(d_rd_into is not None),
            ptr(d_scales), ptr(workspace), stream_of(z)), "cn_volume_render_compose_scaled_backward")
    del keep, keep_outs
    return (d_raws, d_rd, d_scales) if want_scales else (d_raws, d_rd)


def object_rays_backward(g_ro_obj: Optional[Tensor], g_rd_obj: Optional[Tensor], ro: Tensor, rd: Tensor, poses,
                         want_ro: bool = True, want_rd: bool = True, want_poses: bool = True,
                         ray_into: Optional[Tuple[Tensor, Tensor]] = None):
    """Gradient of object_rays (cn_object_rays_backward) -> (d_ro (R, 3), d_rd (R, 3), d_poses (K, 12): dR
    row-major, then dt -- (K, 13) with the scale's gradient last for similarity poses,
    cn_object_rays_scaled_backward), each None when not wanted.  ``g_ro_obj`` / ``g_rd_obj`` (K, R, 3), either may
    be None (zero); ``poses`` as object_rays takes them.  ``ray_into``: (d_ro, d_rd) contiguous (R, 3) device
    tensors the rays' gradients are ADDED into, and returned.  Deterministic: a fixed reduction order."""
    lib = _lib_ready()
    ro, rd = _cuda(ro, "ro"), _cuda(rd, "rd")
    n = ro.shape[0]
    assert ro.shape == (n, 3) and rd.shape == (n, 3), "ro / rd must be (num_rays, 3)"
    flat, width = _pose_rows(poses)
    k = len(flat) // width
    g_ro_obj, g_rd_obj = _opt(g_ro_obj, "g_ro_obj"), _opt(g_rd_obj, "g_rd_obj")
    assert all(g is None or g.shape == (k, n, 3) for g in (g_ro_obj, g_rd_obj)), \
        "g_ro_obj / g_rd_obj must be (num_objects, num_rays, 3)"
    dev = ro.device
    if ray_into is not None:
        d_ro, d_rd = ray_into
        assert all(t.is_cuda and t.is_contiguous() and t.shape == (n, 3) and t.dtype == torch.float32 for t in ray_into)
    else:
        d_ro = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_ro else None
        d_rd = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_rd else None
    d_poses = torch.empty(k, width, device=dev, dtype=torch.float32) if want_poses else None
    assert d_ro is not None or d_rd is not None or d_poses is not None, "nothing wanted"
    if n == 0:
        return d_ro, d_rd, (None if d_poses is None else d_poses.zero_())
    entry, floats, name = ((lib.cn_object_rays_backward, lib.cn_object_rays_backward_workspace_floats,
                            "cn_object_rays_backward") if width == 12 else
                           (lib.cn_object_rays_scaled_backward, lib.cn_object_rays_scaled_backward_workspace_floats,
                            "cn_object_rays_scaled_backward"))
    workspace = None
    if want_poses:
        workspace = torch.empty(floats(n, k), device=dev, dtype=torch.float32)
    check(entry(ptr(g_ro_obj), ptr(g_rd_obj), ptr(ro), ptr(rd), n, _lib.host_floats(flat), k, ptr(d_ro), ptr(d_rd),
                int(ray_into is not None), ptr(d_poses), ptr(workspace), stream_of(ro)), name)
    return d_ro, d_rd, d_poses


def occupancy_gather(g_raw: Tensor, state) -> Tensor:
    """Gradient of occupancy_expand (cn_occupancy_gather): ``g_raw`` (R, S, 4) -> the kept rows' gradients
    (M', 4) in compact order; the culled slots' are dropped.  ``state``: occupancy_cull's."""
    lib = _lib_ready()
    workspace, n, s, k = state
    g_raw = _aligned16(_cuda(g_raw, "g_raw"))
    assert g_raw.shape == (n, s, 4), "g_raw must be (num_rays, num_samples, 4)"
    g_compact = torch.empty(k, 4, device=g_raw.device, dtype=torch.float32)
    if k:
        check(lib.cn_occupancy_gather(ptr(g_raw), ptr(workspace), n, s, ptr(g_compact), stream_of(g_raw)),
              "cn_occupancy_gather")
    return g_compact


def occupancy_cull_backward(g_pts: Optional[Tensor], g_vdir: Optional[Tensor], z: Tensor, chunk_rows: int, state,
                            want_ro: bool = True, want_rd: bool = True) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """Gradient of the rows occupancy_cull forms (cn_occupancy_cull_backward): ``g_pts`` / ``g_vdir`` (M', 3),
    either may be None (zero) -> d_ro, d_rd (R, 3), each None when not wanted.  ``z``, ``chunk_rows`` and
    ``state`` as in (and from) that occupancy_cull call.  Sequential fp32 sums in a fixed order: deterministic."""
    lib = _lib_ready()
    workspace, n, s, k = state
    z = _cuda(z, "z_vals")
    assert z.shape == (n, s), "z must be (num_rays, num_samples)"
    g_pts, g_vdir = _opt(g_pts, "g_pts"), _opt(g_vdir, "g_vdir")
    assert all(g is None or g.shape == (k, 3) for g in (g_pts, g_vdir)), f"g_pts / g_vdir must hold the {k} kept rows"
    assert want_ro or want_rd, "nothing wanted"
    d_ro = torch.empty(n, 3, device=z.device, dtype=torch.float32) if want_ro else None
    d_rd = torch.empty(n, 3, device=z.device, dtype=torch.float32) if want_rd else None
    if n * s:
        check(lib.cn_occupancy_cull_backward(ptr(g_pts), ptr(g_vdir), ptr(z), ptr(workspace), n, s, int(chunk_rows),
                                             ptr(d_ro), ptr(d_rd), stream_of(z)), "cn_occupancy_cull_backward")
    return d_ro, d_rd


def ray_bundle_backward(dirs: Tensor, batch: int, g_ro: Optional[Tensor], g_rd: Optional[Tensor]) -> Tensor:
    """Gradient of get_bundle (ray_sampler.py:95-98) w.r.t. tform_cam2world -> (B, 4, 4)."""
    lib = _lib_ready()
    dirs = _cuda(dirs, "directions")
    hw = dirs.numel() // 3
    g_ro, g_rd = _opt(g_ro, "g_ro"), _opt(g_rd, "g_rd")
    d = torch.zeros(batch, 4, 4, device=dirs.device, dtype=torch.float32)
    if g_ro is None and g_rd is None:
        return d
    check(lib.cn_ray_bundle_backward(ptr(dirs), hw, batch, ptr(g_ro), ptr(g_rd), ptr(d), stream_of(d)),
          "cn_ray_bundle_backward")
    return d


def gather_rays_backward(g_ro: Optional[Tensor], g_rd: Optional[Tensor], batch: int, hw: int,
                         select_inds: Tensor) -> Tuple[Tensor, Tensor]:
    """Gradient of the sample gather (ray_sampler.py:77-80) -> d ro, d rd (B, HW, 3)."""
    lib = _lib_ready()
    sel = _cuda(select_inds, "select_inds", torch.int64)
    g_ro, g_rd = _opt(g_ro, "g_ro"), _opt(g_rd, "g_rd")
    d_ro = torch.zeros(batch, hw, 3, device=sel.device, dtype=torch.float32)
    d_rd = torch.zeros_like(d_ro)
    check(lib.cn_gather_rays_backward(ptr(g_ro), ptr(g_rd), batch, hw, ptr(sel), sel.shape[1], ptr(d_ro), ptr(d_rd),
                                      stream_of(sel)), "cn_gather_rays_backward")
    return d_ro, d_rd


def radiance_field_train(packed: Tensor, cb: Tensor, rd: Tensor, n_samples: int, chunk_rows: int,
                         freqs_xyz: Sequence[float], freqs_dir: Sequence[float], pts: Optional[Tensor] = None,
                         ro: Optional[Tensor] = None, z: Optional[Tensor] = None,
                         code_index: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """fp32 radiance_field that also keeps the activations -> raw (R,S,4), saved (5, R*S, 256)."""
    lib = _lib_ready()
    rd, pts, ro, z, code_index, n, fx, fd = _ray_inputs(rd, n_samples, freqs_xyz, freqs_dir, pts, ro, z, code_index,
                                                        cb.shape[0])
    raw = torch.empty(n, n_samples, 4, device=rd.device, dtype=torch.float32)
    saved = torch.empty(5, n * n_samples, 256, device=rd.device, dtype=torch.float32)
    if n * n_samples == 0:
        return raw, saved
    check(lib.cn_radiance_field_train(ptr(packed), ptr(cb), ptr(code_index), cb.shape[0], ptr(pts), ptr(ro), ptr(rd),
                                      ptr(z), n, n_samples, chunk_rows, fx, fd, ptr(raw), ptr(saved), stream_of(rd)),
          "cn_radiance_field_train")
    return raw, saved


def radiance_field_train_w16(packed: Tensor, cb: Tensor, rd: Tensor, n_samples: int, chunk_rows: int,
                             freqs_xyz: Sequence[float], freqs_dir: Sequence[float], pts: Optional[Tensor] = None,
                             ro: Optional[Tensor] = None, z: Optional[Tensor] = None,
                             code_index: Optional[Tensor] = None, precision: str = "f32"):
    """Training forward -> raw (R,S,4), saved (5, R*S, 256), ReLU masks (the fused training backward's
    inputs): precision "f32" on the fp32 16x16x4 kernel (packed "f32_w16"), "bf16x3" on the 3xbf16
    kernel (packed "bf16x3")."""
    fmt = _lib.CN_FMT_BF16X3 if precision == "bf16x3" else _lib.CN_FMT_F32_W16
    lib = _lib_ready()
    rd, pts, ro, z, code_index, n, fx, fd = _ray_inputs(rd, n_samples, freqs_xyz, freqs_dir, pts, ro, z, code_index,
                                                        cb.shape[0])
    m = n * n_samples
    raw = torch.empty(n, n_samples, 4, device=rd.device, dtype=torch.float32)
    if m == 0:
        return (raw, torch.empty(5, 0, 256, device=rd.device, dtype=torch.float32),
                torch.empty(0, device=rd.device, dtype=torch.int32))
    # the planes (+ fp32: the encoding plane) + one scratch row (cn_radiance_field_train_fmt); ``saved`` is
    # the (5, m, 256) planes view, the backward finds the encoding plane after them in the same storage
    buf = torch.empty(int(lib.cn_field_train_saved_floats(fmt, m)), device=rd.device, dtype=torch.float32)
    saved = buf[:5 * m * 256].view(5, m, 256)
    masks = torch.empty(int(lib.cn_field_mask_words_fmt(fmt, m)), device=rd.device, dtype=torch.int32)
    check(lib.cn_radiance_field_train_fmt(fmt, ptr(packed), ptr(cb), ptr(code_index), cb.shape[0], ptr(pts), ptr(ro),
                                          ptr(rd), ptr(z), n, n_samples, chunk_rows, fx, fd, ptr(raw), ptr(saved),
                                          ptr(masks), stream_of(rd)), "cn_radiance_field_train_fmt")
    return raw, saved, masks


def field_backward_train(packed_t: Tensor, params: Sequence[Tensor], masks: Tensor, saved: Tensor,
                         x_enc: Optional[Tensor],
                         d_raw: Tensor, n_rays: int, n_samples: int, chunk_rows: int, n_codes: int,
                         freqs_xyz: Sequence[float], freqs_dir: Sequence[float], rd: Tensor,
                         pts: Optional[Tensor] = None, ro: Optional[Tensor] = None, z: Optional[Tensor] = None,
                         code_index: Optional[Tensor] = None, param_grads: Optional[Sequence[Tensor]] = None,
                         want_pts: bool = False, want_ro: bool = False, want_rd: bool = False,
                         precision: str = "f32", g_code: Optional[Tensor] = None):
    """Fused training backward (one dX launch + deterministic dW GEMMs) -> dict g_code / d_pts / d_ro / d_rd.
    precision "f32" (packed_t "f32_w16_t") or "bf16x3" (packed_t "bf16x3_t", 3xbf16 dW GEMMs).
    ``g_code``: a zeroed (n_codes, CN_CODE_BIAS_STRIDE) accumulator (field_prepare's), else allocated."""
    return field_backward_train_multi([dict(
        packed_t=packed_t, params=params, masks=masks, saved=saved, x_enc=x_enc, d_raw=d_raw, n_rays=n_rays,
        n_samples=n_samples, chunk_rows=chunk_rows, n_codes=n_codes, freqs_xyz=freqs_xyz, freqs_dir=freqs_dir, rd=rd,
        pts=pts, ro=ro, z=z, code_index=code_index, param_grads=param_grads, want_pts=want_pts, want_ro=want_ro,
        want_rd=want_rd, g_code=g_code)], precision)[0]


def field_backward_train_multi(fields: Sequence[dict], precision: str = "f32"):
    """The training backwards of a render's fields (field_backward_train's keyword arguments, one dict
    per field, 1 or 2) through ONE cn_field_backward_train_multi call: with two fp32 fields on rays +
    depths, one dX launch, one batched dW launch (layer_xyz1's dW among its jobs), one DIRS-pass launch
    and one reduction launch for both, every gradient bitwise that of the per-field calls -> one result
    dict per field."""
    assert len(fields) in (1, 2)
    fmt_t = _lib.CN_FMT_BF16X3_T if precision == "bf16x3" else _lib.CN_FMT_F32_W16_T
    lib = _lib_ready()
    outs, structs, keep = [], [], []
    stream = None
    for f in fields:
        n_rays, n_samples, n_codes = f["n_rays"], f["n_samples"], f["n_codes"]
        m = n_rays * n_samples
        params = [_cuda(p.detach(), f"param{i}") for i, p in enumerate(f["params"])]
        d_raw = _aligned16(_cuda(f["d_raw"], "d_raw"))
        saved, x_enc = f["saved"], f.get("x_enc")
        assert d_raw.numel() == 4 * m and saved.shape == (5, m, 256) and (x_enc is None or x_enc.shape == (m, 90))
        if m and precision != "bf16x3" and x_enc is None:
            # the fp32 backward reads the forward's encoding plane at saved + 5 M 256 (cn_field_backward_train_fmt):
            # ``saved`` must be radiance_field_train_w16's view of its whole save buffer, not a copy of the planes
            need = 4 * int(lib.cn_field_train_saved_floats(_lib.CN_FMT_F32_W16, m))
            assert saved.is_contiguous() and saved.storage_offset() == 0 and \
                saved.untyped_storage().nbytes() >= need, \
                "field_backward_train: saved must be the training forward's own buffer (planes + encoding plane)"
        dev = d_raw.device
        rd, pts, ro, z, code_index, _, fx, fd = _ray_inputs(
            f["rd"], n_samples, f["freqs_xyz"], f["freqs_dir"], f.get("pts"), f.get("ro"), f.get("z"),
            f.get("code_index"), n_codes, n_rays)
        ws = torch.empty(max(0, int(lib.cn_field_backward_train_workspace_floats(m))), device=dev, dtype=torch.float32)
        g_code = f.get("g_code")
        if g_code is None:
            g_code = torch.zeros(n_codes, _lib.CN_CODE_BIAS_STRIDE, device=dev, dtype=torch.float32)
        else:
            assert g_code.shape == (n_codes, _lib.CN_CODE_BIAS_STRIDE) and g_code.is_contiguous()
        d_pts = torch.empty(n_rays, n_samples, 3, device=dev, dtype=torch.float32) if f.get("want_pts") else None
        d_ro = torch.zeros(n_rays, 3, device=dev, dtype=torch.float32) if f.get("want_ro") else None
        d_rd = torch.zeros(n_rays, 3, device=dev, dtype=torch.float32) if f.get("want_rd") else None
        outs.append({"g_code": g_code, "d_pts": d_pts, "d_ro": d_ro, "d_rd": d_rd})
        if m == 0:      # no samples: nothing accumulates (the C ABI refuses n_rays == 0)
            continue
        arr, k1 = _lib.pointer_array(params)
        garr, k2 = (None, None)
        pg = f.get("param_grads")
        if pg is not None:
            assert len(pg) == _lib.CN_NUM_PARAMS and all(g.is_contiguous() for g in pg)
            garr, k2 = _lib.pointer_array(list(pg))
        keep += [params, d_raw, ws, arr, k1, garr, k2, fx, fd, rd, pts, ro, z, code_index]
        structs.append(_lib.FieldTrainBwd(
            ptr(f["packed_t"]), arr, ptr(f["masks"]), ptr(saved), ptr(x_enc), ptr(d_raw), ptr(pts), ptr(ro), ptr(rd),
            ptr(z), n_rays, n_samples, f["chunk_rows"], ptr(code_index), n_codes,
            ctypes.cast(fx, ctypes.POINTER(ctypes.c_float)), ctypes.cast(fd, ctypes.POINTER(ctypes.c_float)), ptr(ws),
            garr, ptr(g_code), ptr(d_pts), ptr(d_ro), ptr(d_rd)))
        stream = stream_of(d_raw)
    if structs:
        jobs = (_lib.FieldTrainBwd * len(structs))(*structs)
        check(lib.cn_field_backward_train_multi(fmt_t, jobs, len(structs), stream), "cn_field_backward_train_multi")
    del keep
    return outs


def mlp_forward_train(packed: Tensor, cb: Tensor, x: Tensor, code_index: Optional[Tensor] = None
                      ) -> Tuple[Tensor, Tensor]:
    """fp32 mlp_forward that also keeps the activations -> raw (M,4), saved (5, M, 256)."""
    lib = _lib_ready()
    x = _cuda(x, "x")
    assert x.dim() == 2 and x.shape[1] == 90
    m = x.shape[0]
    if code_index is not None:
        code_index = _cuda(code_index, "code_index", torch.int64)
    raw = torch.empty(m, 4, device=x.device, dtype=torch.float32)
    saved = torch.empty(5, m, 256, device=x.device, dtype=torch.float32)
    check(lib.cn_mlp_forward_train(ptr(packed), ptr(cb), ptr(code_index), cb.shape[0], ptr(x), m, ptr(raw),
                                   ptr(saved), stream_of(x)), "cn_mlp_forward_train")
    return raw, saved


def encode_inputs(rd: Tensor, n_samples: int, chunk_rows: int, freqs_xyz: Sequence[float],
                  freqs_dir: Sequence[float], pts: Optional[Tensor] = None, ro: Optional[Tensor] = None,
                  z: Optional[Tensor] = None) -> Tensor:
    """forward_pass's MLP input rows (nerf/__init__.py:116-132) -> (R*S, 90)."""
    lib = _lib_ready()
    rd, pts, ro, z, _, n, fx, fd = _ray_inputs(rd, n_samples, freqs_xyz, freqs_dir, pts, ro, z, None, None)
    x = torch.empty(n * n_samples, 90, device=rd.device, dtype=torch.float32)
    if n * n_samples == 0:
        return x
    check(lib.cn_encode_inputs(ptr(pts), ptr(ro), ptr(rd), ptr(z), n, n_samples, chunk_rows, fx, fd, ptr(x),
                               stream_of(rd)), "cn_encode_inputs")
    return x


def field_backward(params: Sequence[Tensor], saved: Tensor, x_enc: Tensor, d_raw: Tensor, n_rays: int,
                   n_samples: int, chunk_rows: int, n_codes: int, freqs_xyz=None, freqs_dir=None,
                   rd: Optional[Tensor] = None, pts: Optional[Tensor] = None, ro: Optional[Tensor] = None,
                   z: Optional[Tensor] = None, code_index: Optional[Tensor] = None,
                   param_grads: Optional[Sequence[Tensor]] = None, want_code: bool = False,
                   want_pts: bool = False, want_ro: bool = False, want_rd: bool = False, want_x: bool = False,
                   precision: str = "f32"):
    """Backward of forward_pass + CodeNeRFModel.forward -> dict of d_pts / d_ro / d_rd / g_code / d_x.

    ``param_grads``: 18 zero-or-running fp32 buffers the parameter gradients accumulate into.
    ``precision``: the GEMMs' arithmetic, "f32" (exact products) or "bf16x3" (split bf16 MFMA).
    """
    lib = _lib_ready()
    m = n_rays * n_samples
    params = [_cuda(p.detach(), f"param{i}") for i, p in enumerate(params)]
    d_raw = _aligned16(_cuda(d_raw, "d_raw"))
    assert d_raw.numel() == 4 * m and saved.shape == (5, m, 256) and (x_enc is None or x_enc.shape == (m, 90))
    dev = d_raw.device
    if rd is not None:
        rd, pts, ro, z, code_index, _, fx, fd = _ray_inputs(rd, n_samples, freqs_xyz, freqs_dir, pts, ro, z, code_index,
                                                            n_codes, n_rays)
    else:       # no ray gradient wanted (encoded rows, or points alone): the C side's own rules
        pts, ro, z = _opt(pts, "pts"), _opt(ro, "ro"), _opt(z, "z")
        code_index = None if code_index is None else _cuda(code_index, "code_index", torch.int64)
        fx = _lib.host_floats(freqs_xyz) if freqs_xyz is not None else None
        fd = _lib.host_floats(freqs_dir) if freqs_dir is not None else None
    ws =torch.empty(max(0, int(lib.cn_field_backward_workspace_floats(m))), device=dev, dtype=torch.float32)
    out = {}
    g_code = torch.zeros(n_codes, _lib.CN_CODE_BIAS_STRIDE, device=dev, dtype=torch.float32) if want_code else None
    d_pts = torch.empty(n_rays, n_samples, 3, device=dev, dtype=torch.float32) if want_pts else None
    d_ro = torch.zeros(n_rays, 3, device=dev, dtype=torch.float32) if want_ro else None
    d_rd = torch.zeros(n_rays, 3, device=dev, dtype=torch.float32) if want_rd else None
    if m == 0:      # no samples: zero sums (the C ABI refuses n_rays == 0)
        out.update(g_code=g_code, d_pts=d_pts, d_ro=d_ro, d_rd=d_rd)
        if want_x:
            out["d_x"] = torch.empty(0, 90, device=dev, dtype=torch.float32)
        return out
    arr, keep = _lib.pointer_array(params)
    garr, gkeep = (None, None)
    if param_grads is not None:
        assert len(param_grads) == _lib.CN_NUM_PARAMS and all(g.is_contiguous() for g in param_grads)
        garr, gkeep = _lib.pointer_array(list(param_grads))
    check(lib.cn_field_backward_fmt(_lib.FORMATS[precision], arr, ptr(saved), ptr(x_enc), ptr(d_raw), ptr(pts), ptr(ro), ptr(rd), ptr(z), n_rays,
                                n_samples, chunk_rows, ptr(code_index), n_codes, fx, fd, ptr(ws), garr, ptr(g_code),
                                ptr(d_pts), ptr(d_ro), ptr(d_rd), stream_of(d_raw)), "cn_field_backward_fmt")
    del keep, gkeep
    out.update(g_code=g_code, d_pts=d_pts, d_ro=d_ro, d_rd=d_rd)
    if want_x:
        off = int(lib.cn_field_backward_dx_offset(m))
        out["d_x"] = ws[off: off + 90 * m].view(m, 90)
    return out


def code_bias_backward(params: Sequence[Tensor], z_s: Tensor, z_t: Tensor, g_code: Tensor,
                       param_grads: Optional[Sequence[Tensor]] = None, want_z: bool = True,
                       single_launch: bool = False, dz_into: Optional[Tuple[Tensor, Tensor]] = None):
    """Backward of code_bias (model.py:174-177 + the code halves) -> dz_s, dz_t (n_codes, 256) or None.
    The two-launch form (cn_code_bias_backward_ws) unless single_launch (cn_code_bias_backward):
    bitwise the same results.  ``dz_into`` (two contiguous (n_codes, 256) device tensors, two-launch
    form): the code gradients are ADDED into them (accumulate_dz) and returned."""
    lib = _lib_ready()
    params = [_cuda(p.detach(), f"param{i}") for i, p in enumerate(params)]
    z_s, z_t, g_code = _cuda(z_s.detach(), "z_s"), _cuda(z_t.detach(), "z_t"), _cuda(g_code, "g_code")
    n = z_s.shape[0]
    if dz_into is not None:
        assert not single_launch, "dz_into: the two-launch form"
        for d in dz_into:
            assert d.is_cuda and d.dtype == torch.float32 and d.is_contiguous() and d.shape == z_s.shape, \
                "dz_into: contiguous (n_codes, 256) fp32 device tensors"
        dz_s, dz_t = dz_into
    else:
        dz_s = torch.empty_like(z_s) if want_z else None
        dz_t = torch.empty_like(z_t) if want_z else None
    arr, keep = _lib.pointer_array(params)
    garr, gkeep = (None, None)
    if param_grads is not None:
        garr, gkeep = _lib.pointer_array(list(param_grads))
    if single_launch:
        check(lib.cn_code_bias_backward(arr, ptr(z_s), ptr(z_t), n, ptr(g_code), ptr(dz_s), ptr(dz_t), garr,
                                        stream_of(g_code)), "cn_code_bias_backward")
    else:
        ws = torch.empty(lib.cn_code_bias_backward_workspace_floats(n), device=g_code.device, dtype=torch.float32)
        check(lib.cn_code_bias_backward_ws(arr, ptr(z_s), ptr(z_t), n, ptr(g_code), ptr(dz_s), ptr(dz_t), garr,
                                           ptr(ws), int(dz_into is not None), stream_of(g_code)),
              "cn_code_bias_backward_ws")
    del keep, gkeep
    return dz_s, dz_t


def code_ds_outer(params: Sequence[Tensor], z_s: Tensor, z_t: Tensor, code_act: Tensor, g_code: Tensor,
                  param_grads: Optional[Sequence[Tensor]] = None) -> Tensor:
    """cn_code_bias_backward_act: the code backward's first half on the forward's code-layer activations
    (field_prepare_models(..., want_act=True)) -> its workspace (the masked ds1 / ds2 / dt1, for code_dz);
    the code layers' and code halves' gradients are added into ``param_grads``."""
    lib = _lib_ready()
    params = [_cuda(p.detach(), f"param{i}") for i, p in enumerate(params)]
    z_s, z_t, g_code = _cuda(z_s.detach(), "z_s"), _cuda(z_t.detach(), "z_t"), _cuda(g_code, "g_code")
    code_act = _cuda(code_act, "code_act")
    n = z_s.shape[0]
    assert code_act.numel() == n * 768, "code_act: (n_codes, 768)"
    ws = torch.empty(lib.cn_code_bias_backward_workspace_floats(n), device=g_code.device, dtype=torch.float32)
    arr, keep = _lib.pointer_array(params)
    garr, gkeep = _lib.pointer_array(list(param_grads)) if param_grads is not None else (None, None)
    check(lib.cn_code_bias_backward_act(arr, ptr(z_s), ptr(z_t), n, ptr(code_act), ptr(g_code), garr, ptr(ws),
                                        stream_of(g_code)), "cn_code_bias_backward_act")
    del keep, gkeep
    return ws


def code_ds_outer_multi(jobs, z_s: Tensor, z_t: Tensor):
    """code_ds_outer of a render's 1 or 2 fields on the same codes in ONE launch
    (cn_code_bias_backward_act_multi); jobs: [(params, code_act, g_code, param_grads | None)] -> the
    workspaces, one per job (bitwise code_ds_outer's)."""
    lib = _lib_ready()
    assert 1 <= len(jobs) <= 2, "one or two jobs"
    z_s, z_t = _cuda(z_s.detach(), "z_s"), _cuda(z_t.detach(), "z_t")
    n = z_s.shape[0]
    structs, keep, outs = [], [], []
    for params, code_act, g_code, param_grads in jobs:
        params = [_cuda(p.detach(), f"param{i}") for i, p in enumerate(params)]
        g_code, code_act = _cuda(g_code, "g_code"), _cuda(code_act, "code_act")
        assert code_act.numel() == n * 768, "code_act: (n_codes, 768)"
        ws = torch.empty(lib.cn_code_bias_backward_workspace_floats(n), device=g_code.device, dtype=torch.float32)
        arr, k1 = _lib.pointer_array(params)
        garr, k2 = _lib.pointer_array(list(param_grads)) if param_grads is not None else (None, None)
        keep += [params, g_code, code_act, arr, k1, garr, k2]
        structs.append(_lib.CodeActJob(arr, ptr(code_act), ptr(g_code), garr, ptr(ws)))
        outs.append(ws)
    js = (_lib.CodeActJob * len(structs))(*structs)
    check(lib.cn_code_bias_backward_act_multi(js, len(structs), ptr(z_s), ptr(z_t), n, stream_of(z_s)),
          "cn_code_bias_backward_act_multi")
    del keep
    return outs


def code_dz(jobs: Sequence[Tuple[Sequence[Tensor], Tensor, Tensor]], n_codes: int,
            dz_into: Optional[Tuple[Tensor, Tensor]] = None):
    """cn_code_dz: dz_s, dz_t of one or two fields' code backwards [(params, g_code, code_ds_outer's
    workspace)] on the same codes, summed in job order -> fresh (n_codes, 256) tensors, or ADDED into
    ``dz_into`` (contiguous (n_codes, 256) device tensors) and those returned."""
    lib = _lib_ready()
    assert 1 <= len(jobs) <= 2, "one or two jobs"
    dev = jobs[0][1].device
    if dz_into is not None:
        for d in dz_into:
            assert d.is_cuda and d.dtype == torch.float32 and d.is_contiguous() and d.shape == (n_codes, 256), \
                "dz_into: contiguous (n_codes, 256) fp32 device tensors"
        dz_s, dz_t = dz_into
    else:
        dz_s = torch.empty(n_codes, 256, device=dev, dtype=torch.float32)
        dz_t = torch.empty(n_codes, 256, device=dev, dtype=torch.float32)
    arr = (_lib.CodeDzJob * len(jobs))()
    keep = []
    for k, (params, g_code, ws) in enumerate(jobs):
        params = [_cuda(p.detach(), f"param{i}") for i, p in enumerate(params)]
        pa, pk = _lib.pointer_array(params)
        keep += [params, pa, pk]
        arr[k] = _lib.CodeDzJob(pa, ptr(_cuda(g_code, "g_code")), ptr(ws))
    check(lib.cn_code_dz(arr, len(jobs), n_codes, ptr(dz_s), ptr(dz_t), int(dz_into is not None), stream_of(dz_s)),
          "cn_code_dz")
    del keep
    return dz_s, dz_t


def gemm_nn(a: Tensor, b: Tensor, mask: Optional[Tensor] = None, precision: str = "f32") -> Tensor:
    """C = A B (masked where mask <= 0) on the fp32 (or 3xbf16) MFMA tile kernel."""
    lib = _lib_ready()
    # A may be a row-strided view (lda > k, unit column stride), as the field backward's
    # (M, 257)-in-rows-of-260 gradient buffers are
    if not (a.is_cuda and a.dtype == torch.float32 and a.dim() == 2 and a.stride(1) == 1 and a.stride(0) >= a.shape[1]):
        a = _cuda(a, "A")
    b = _cuda(b, "B")
    (m, k), (k2, n) = a.shape, b.shape
    assert k == k2
    mask = _opt(mask, "mask")
    c = torch.empty(m, n, device=a.device, dtype=torch.float32)
    fn, name = (lib.cn_gemm_nn_x3, "cn_gemm_nn_x3") if precision == "bf16x3" else (lib.cn_gemm_nn, "cn_gemm_nn")
    check(fn(ptr(a), a.stride(0), ptr(b), n, ptr(c), n, ptr(mask), n, m, n, k, stream_of(a)), name)
    return c


def gemm_tn(a: Tensor, b: Tensor, c: Optional[Tensor] = None, precision: str = "f32",
            deterministic: bool = False) -> Tensor:
    """C += A^T B on the fp32 (or 3xbf16) MFMA tile kernel (C zero-initialised when not given).
    deterministic: partial tiles + a fixed-order reduction (cn_gemm_tn_ws) instead of float atomics."""
    lib = _lib_ready()
    a, b = _cuda(a, "A"), _cuda(b, "B")
    (m, n), (m2, k) = a.shape, b.shape
    assert m == m2
    if c is None:
        c = torch.zeros(n, k, device=a.device, dtype=torch.float32)
    if deterministic:
        ws = torch.empty(lib.cn_gemm_tn_workspace_floats(m, n, k), device=a.device, dtype=torch.float32)
        fmt = _lib.FORMATS["bf16x3" if precision == "bf16x3" else "f32"]
        check(lib.cn_gemm_tn_ws(fmt, ptr(a), n, ptr(b), k, ptr(c), k, m, n, k, ptr(ws), stream_of(a)), "cn_gemm_tn_ws")
        return c
    fn, name = (lib.cn_gemm_tn_x3, "cn_gemm_tn_x3") if precision == "bf16x3" else (lib.cn_gemm_tn, "cn_gemm_tn")
    check(fn(ptr(a), n, ptr(b), k, ptr(c), k, m, n, k, stream_of(a)), name)
    return c


def posenc_backward(x: Tensor, freqs: Sequence[float], include_input: bool, g_enc: Tensor) -> Tensor:
    """Gradient of PositionalEmbedder.embed (position_embed.py:35-53) w.r.t. its input."""
    lib = _lib_ready()
    x, g_enc = _cuda(x, "x"), _cuda(g_enc, "g_enc")
    d = x.shape[-1]
    m = x.numel() // d
    assert g_enc.numel() == m * d * (int(include_input) + 2 * len(freqs))
    dx = torch.empty_like(x)
    check(lib.cn_posenc_backward(ptr(x), m, d, _lib.host_floats(freqs), len(freqs), int(include_input), ptr(g_enc),
                                 ptr(dx), stream_of(x)), "cn_posenc_backward")
    return dx


def ray_points_backward(g_pts: Tensor, z: Tensor, want_ro: bool = True, want_rd: bool = True):
    """Gradient of pts = ro + rd z (point_sampler.py:70, :118; z detached) -> d_ro, d_rd (R, 3)."""
    lib = _lib_ready()
    g_pts, z = _cuda(g_pts, "g_pts"), _cuda(z, "z")
    n, s = z.shape
    assert g_pts.shape == (n, s, 3)
    d_ro = torch.zeros(n, 3, device=z.device, dtype=torch.float32) if want_ro else None
    d_rd = torch.zeros(n, 3, device=z.device, dtype=torch.float32) if want_rd else None
    if want_ro or want_rd:
        check(lib.cn_ray_points_backward(ptr(g_pts), ptr(z), n, s, ptr(d_ro), ptr(d_rd), stream_of(z)),
              "cn_ray_points_backward")
    return d_ro, d_rd


# ------------------------------------------------------------------ fused 3xbf16 backward (eval step)


def radiance_field_masks(packed: Tensor, cb: Tensor, rd: Tensor, n_samples: int, chunk_rows: int,
                         freqs_xyz: Sequence[float], freqs_dir: Sequence[float], pts: Optional[Tensor] = None,
                         ro: Optional[Tensor] = None, z: Optional[Tensor] = None,
                         code_index: Optional[Tensor] = None, precision: str = "bf16x3") -> Tuple[Tensor, Tensor]:
    """radiance_field that also writes the ReLU masks of the fused backward -> raw (R,S,4), masks (uint32
    words as int32).  precision "bf16x3" (packed "bf16x3") or "f32" (packed "f32_w16": the fp32
    16x16x4 kernel)."""
    fmt = _lib.CN_FMT_BF16X3 if precision == "bf16x3" else _lib.CN_FMT_F32_W16
    lib = _lib_ready()
    rd, pts, ro, z, code_index, n, fx, fd = _ray_inputs(rd, n_samples, freqs_xyz, freqs_dir, pts, ro, z, code_index,
                                                        cb.shape[0])
    m = n * n_samples
    raw = torch.empty(n, n_samples, 4, device=rd.device, dtype=torch.float32)
    if m == 0:
        return raw, torch.empty(0, device=rd.device, dtype=torch.int32)
    masks = torch.empty(int(lib.cn_field_mask_words_fmt(fmt, m)), device=rd.device, dtype=torch.int32)
    check(lib.cn_radiance_field_masks_fmt(fmt, ptr(packed), ptr(cb), ptr(code_index), cb.shape[0], ptr(pts), ptr(ro),
                                          ptr(rd), ptr(z), n, n_samples, chunk_rows, fx, fd, ptr(raw), ptr(masks),
                                          stream_of(rd)), "cn_radiance_field_masks_fmt")
    return raw, masks


def fused_backward_supported(n_codes: int, n_samples: int, code_index: Optional[Tensor] = None,
                             precision: str = "bf16x3") -> bool:
    """cn_field_backward_fused needs one code row per wave: 32 consecutive samples (bf16x3) or 16 (f32)."""
    return n_codes == 1 or n_samples % (32 if precision == "bf16x3" else 16) == 0


def field_backward_x3_acc_floats(n_codes: int, n_rays: int, want_ro: bool, want_rd: bool) -> int:
    """Floats of field_backward_x3's zeroed accumulator buffer: g_code, then d ro / d rd if wanted."""
    return n_codes * _lib.CN_CODE_BIAS_STRIDE + 3 * n_rays * (int(want_ro) + int(want_rd))


def field_backward_x3(packed_t: Tensor, masks: Tensor, d_raw: Tensor, n_rays: int, n_samples: int,
                      chunk_rows: int, n_codes: int, freqs_xyz: Sequence[float], freqs_dir: Sequence[float],
                      rd: Tensor, pts: Optional[Tensor] = None, ro: Optional[Tensor] = None,
                      z: Optional[Tensor] = None, code_index: Optional[Tensor] = None, want_pts: bool = False,
                      want_ro: bool = False, want_rd: bool = False, precision: str = "bf16x3",
                      acc: Optional[Tensor] = None, ray_into: Optional[Tuple[Tensor, Tensor]] = None,
                      deterministic: bool = True):
    """Fused backward of forward_pass + CodeNeRFModel.forward (frozen weights) -> g_code / d_pts / d_ro / d_rd.
    precision "bf16x3" (packed_t "bf16x3_t") or "f32" (packed_t "f32_w16_t", masks of the f32_w16 forward).
    ``acc``: a zeroed buffer of field_backward_x3_acc_floats(...) floats for the accumulated outputs
    (field_prepare's), else one is allocated and filled.  ``ray_into`` ((R, 3) d ro, d rd device tensors,
    with want_ro and want_rd): the ray gradients are ADDED into those instead.  ``deterministic`` (default):
    with one code row and, for bf16x3, S % 32 == 0, cn_field_backward_fused_ws's form without float atomics,
    so repeated backwards give the same bits (False: the float-atomic kernel).  fp32 takes it at every S:
    with S % 16 == 0 a wave's ray sums are one partial row, else each sample's are."""
    fmt_t = _lib.CN_FMT_BF16X3_T if precision == "bf16x3" else _lib.CN_FMT_F32_W16_T
    lib = _lib_ready()
    m = n_rays * n_samples
    d_raw = _aligned16(_cuda(d_raw, "d_raw"))
    assert d_raw.numel() == 4 * m
    dev = d_raw.device
    rd, pts, ro, z, code_index, _, fx, fd = _ray_inputs(rd, n_samples, freqs_xyz, freqs_dir, pts, ro, z, code_index,
                                                        n_codes, n_rays)
    # the accumulated outputs share one zero-filled buffer (one fill launch instead of three)
    nc = n_codes * _lib.CN_CODE_BIAS_STRIDE
    n_acc = field_backward_x3_acc_floats(n_codes, n_rays, want_ro, want_rd)
    if acc is None:
        acc = torch.zeros(n_acc, device=dev, dtype=torch.float32)
    else:
        assert acc.numel() == n_acc and acc.is_contiguous()
    g_code = acc[:nc].view(n_codes, _lib.CN_CODE_BIAS_STRIDE)
    d_ro = acc[nc:nc + 3 * n_rays].view(n_rays, 3) if want_ro else None
    d_rd = acc[acc.numel() - 3 * n_rays:].view(n_rays, 3) if want_rd else None
    if ray_into is not None:
        assert want_ro and want_rd and all(t.is_cuda and t.is_contiguous() and t.shape == (n_rays, 3) for t in ray_into)
        d_ro, d_rd = ray_into
    d_pts = torch.empty(n_rays, n_samples, 3, device=dev, dtype=torch.float32) if want_pts else None
    if m == 0:      # no samples: zero sums (the C ABI refuses n_rays == 0)
        return {"g_code": g_code, "d_pts": d_pts, "d_ro": d_ro, "d_rd": d_rd}
    # one code row (3xbf16: and every wave inside one ray): the deterministic form (no float atomics; its
    # partials in a workspace, summed in a fixed order by two short launches), else the float-atomic kernel
    ws = None
    if deterministic and n_codes == 1 and (precision != "bf16x3" or n_samples % 32 == 0):
        ws = torch.empty(int(lib.cn_field_backward_fused_workspace_floats(fmt_t, n_rays, n_samples)), device=dev,
                         dtype=torch.float32)
    check(lib.cn_field_backward_fused_ws(fmt_t, ptr(packed_t), ptr(masks), ptr(d_raw), ptr(pts), ptr(ro), ptr(rd),
                                         ptr(z), n_rays, n_samples, chunk_rows, ptr(code_index), n_codes, fx, fd,
                                         ptr(g_code), ptr(d_pts), ptr(d_ro), ptr(d_rd), ptr(ws), stream_of(d_raw)),
          "cn_field_backward_fused_ws")
    return {"g_code": g_code, "d_pts": d_pts, "d_ro": d_ro, "d_rd": d_rd}


def field_backward_x3_multi(fields: Sequence[dict], d_rd_between: Optional[Tensor] = None):
    """The eval step's two fields' fused backwards (field_backward_x3's keyword arguments, one dict per
    field, both adding into the same ``ray_into`` d ro / d rd) through ONE cn_field_backward_fused_multi
    call: fp32, one code row, whole waves per ray -> one dX launch, one ray / g_code-row launch and one
    g_code reduction for both.  d ro / d rd end bitwise as field 0's call, then d rd += ``d_rd_between``,
    then field 1's call.  -> one result dict per field."""
    assert len(fields) == 2
    lib = _lib_ready()
    fmt_t = _lib.CN_FMT_F32_W16_T
    structs, keep, outs = [], [], []
    stream = None
    for f in fields:
        assert f.get("precision", "f32") == "f32" and f.get("ray_into") is not None and f.get("acc") is not None
        n_rays, n_samples, n_codes = f["n_rays"], f["n_samples"], f["n_codes"]
        assert n_codes == 1 and n_samples % 16 == 0 and f.get("pts") is None and not f.get("want_pts")
        m = n_rays * n_samples
        d_raw = _aligned16(_cuda(f["d_raw"], "d_raw"))
        assert d_raw.numel() == 4 * m and m > 0
        dev = d_raw.device
        rd, _, ro, z, _, _, fx, fd = _ray_inputs(f["rd"], n_samples, f["freqs_xyz"], f["freqs_dir"], None, f.get("ro"),
                                                 f.get("z"), None, 1, n_rays)
        acc = f["acc"]
        assert acc.numel() == field_backward_x3_acc_floats(n_codes, n_rays, True, True) and acc.is_contiguous()
        g_code = acc[:_lib.CN_CODE_BIAS_STRIDE].view(1, _lib.CN_CODE_BIAS_STRIDE)
        d_ro, d_rd = f["ray_into"]
        assert all(t.is_cuda and t.is_contiguous() and t.shape == (n_rays, 3) for t in (d_ro, d_rd))
        ws = torch.empty(int(lib.cn_field_backward_fused_workspace_floats(fmt_t, n_rays, n_samples)), device=dev,
                         dtype=torch.float32)
        keep += [d_raw, rd, ro, z, ws, fx, fd]
        structs.append(_lib.FieldFusedBwd(
            ptr(f["packed_t"]), ptr(f["masks"]), ptr(d_raw), None, ptr(ro), ptr(rd), ptr(z), n_rays, n_samples,
            f["chunk_rows"], None, 1, ctypes.cast(fx, ctypes.POINTER(ctypes.c_float)),
            ctypes.cast(fd, ctypes.POINTER(ctypes.c_float)), ptr(g_code), None, ptr(d_ro), ptr(d_rd), ptr(ws)))
        outs.append({"g_code": g_code, "d_pts": None, "d_ro": d_ro, "d_rd": d_rd})
        stream = stream_of(d_raw)
    if d_rd_between is not None:
        d_rd_between = _cuda(d_rd_between, "d_rd_between").contiguous()
        assert d_rd_between.shape == outs[0]["d_rd"].shape
    js = (_lib.FieldFusedBwd * 2)(*structs)
    check(lib.cn_field_backward_fused_multi(fmt_t, js, 2, ptr(d_rd_between), stream), "cn_field_backward_fused_multi")
    del keep
    return outs


# ------------------------------------------------------------------ training step: optimiser


def adamw_step(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, segments,
               beta1: float, beta2: float, eps: float) -> None:
    """torch.optim.AdamW.step (train.py:113) on flat fp32 buffers, in place (cn_adamw_step).

    ``segments``: [(begin, end, lr, weight_decay, step)] float ranges (multiples of 4).
    """
    lib = _lib_ready()
    bufs = [_cuda(t, name) for t, name in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"),
                                          (exp_avg_sq, "exp_avg_sq"))]
    n = param.numel()
    assert all(b.data_ptr() == t.data_ptr() and b.numel() == n for b, t in zip(bufs, (param, grad, exp_avg, exp_avg_sq))), \
        "flat optimiser buffers must be contiguous and of one size"
    assert segments and all(b % 4 == 0 and e % 4 == 0 and 0 <= b < e <= n for b, e, *_ in segments)
    k = len(segments)

    def arr(ct, vals):
        return (ct * k)(*vals)
    check(lib.cn_adamw_step(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), k,
                            arr(ctypes.c_int64, [int(s[0]) for s in segments]),
                            arr(ctypes.c_int64, [int(s[1]) for s in segments]),
                            arr(ctypes.c_double, [float(s[2]) for s in segments]),
                            arr(ctypes.c_double, [float(s[3]) for s in segments]),
                            arr(ctypes.c_int64, [int(s[4]) for s in segments]),
                            float(beta1), float(beta2), float(eps), stream_of(param)), "cn_adamw_step")


def adamw_scalars(segments, beta1: float, beta2: float, out) -> None:
    """The per-segment scalars of adamw_step_dev, folded on the host exactly as cn_adamw_step folds
    them: ``out`` a float32 buffer of 3 * len(segments) (a pinned tensor's numpy view)."""
    lib = _lib_ready()
    k = len(segments)
    assert k >= 1 and out.size >= 3 * k

    def arr(ct, vals):
        return (ct * k)(*vals)
    check(lib.cn_adamw_scalars(k, arr(ctypes.c_double, [float(s[2]) for s in segments]),
                               arr(ctypes.c_double, [float(s[3]) for s in segments]),
                               arr(ctypes.c_int64, [int(s[4]) for s in segments]), float(beta1), float(beta2),
                               ctypes.c_void_p(out.ctypes.data)), "cn_adamw_scalars")


def adamw_step_dev(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, segments, scalars: Tensor,
                   beta1: float, beta2: float, eps: float) -> None:
    """adamw_step with the per-segment scalars in device memory (``scalars``: float32, 3 per
    segment): the graph-capturable form (cn_adamw_step_dev)."""
    lib = _lib_ready()
    bufs = [_cuda(t, name) for t, name in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"),
                                          (exp_avg_sq, "exp_avg_sq"))]
    n = param.numel()
    assert all(b.data_ptr() == t.data_ptr() and b.numel() == n for b, t in zip(bufs, (param, grad, exp_avg, exp_avg_sq)))
    k = len(segments)
    assert k >= 1 and scalars.numel() >= 3 * k and scalars.dtype == torch.float32 and scalars.is_cuda
    assert all(b % 4 == 0 and e % 4 == 0 and 0 <= b < e <= n for b, e, *_ in segments)

    def arr(ct, vals):
        return (ct * k)(*vals)
    check(lib.cn_adamw_step_dev(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), k,
                                arr(ctypes.c_int64, [int(s[0]) for s in segments]),
                                arr(ctypes.c_int64, [int(s[1]) for s in segments]), ptr(scalars),
                                float(beta1), float(beta2), float(eps), stream_of(param)), "cn_adamw_step_dev")


# ------------------------------------------------------------------ the step's loss


def render_loss(rgb_coarse: Optional[Tensor], rgb_fine: Optional[Tensor], target: Tensor,
                z_s: Optional[Tensor] = None, z_t: Optional[Tensor] = None, expand: int = 1,
                regularizer_lambda: float = 0.0, psnr: Optional[Tensor] = None) -> Tensor:
    """train.py:103-108 / eval.py:157-163 in one launch -> (6,) [loss_coarse, loss_fine, regulariser,
    total, ||z_s||, ||z_t||]; ``||z||`` over z's elements times ``expand`` (expanded rows).
    ``psnr`` (a float64 device scalar): also mse2psnr of the fine loss, written by the same launch."""
    lib = _lib_ready()
    rc, rf = _opt(rgb_coarse, "rgb_coarse"), _opt(rgb_fine, "rgb_fine")
    target = _cuda(target, "target")
    n = (rc if rc is not None else rf).shape[0]
    assert target.shape[0] == n and target.dim() == 2 and target.shape[1] >= 3, "target must be (R, >=3)"
    zs, zt = _opt(z_s, "z_s"), _opt(z_t, "z_t")
    n_code = 0 if zs is None else zs.numel()
    assert zt is None or zt.numel() == n_code, "z_s and z_t must have the same size"
    out = torch.empty(6, device=target.device, dtype=torch.float32)
    nws = int(lib.cn_render_loss_workspace_doubles(n_code))
    ws = torch.empty(nws, device=target.device, dtype=torch.float64) if nws > 0 else None
    if psnr is not None:
        assert psnr.is_cuda and psnr.dtype == torch.float64 and psnr.numel() == 1, "psnr: a float64 device scalar"
        check(lib.cn_render_loss_psnr(ptr(rc), ptr(rf), ptr(target), target.shape[1], n, ptr(zs), ptr(zt), n_code,
                                      expand, regularizer_lambda, ptr(ws), ptr(out), ptr(psnr), stream_of(out)),
              "cn_render_loss_psnr")
        return out
    check(lib.cn_render_loss(ptr(rc), ptr(rf), ptr(target), target.shape[1], n, ptr(zs), ptr(zt), n_code, expand,
                             regularizer_lambda, ptr(ws), ptr(out), stream_of(out)), "cn_render_loss")
    return out


def render_loss_backward(rgb_coarse, rgb_fine, target, z_s, z_t, expand, regularizer_lambda, stats, grad_total,
                         want=(True, True, True, True), dz_into: Optional[Tuple[Tensor, Tensor]] = None):
    """Backward of render_loss -> (d_rgb_coarse, d_rgb_fine, d_z_s, d_z_t), None where not wanted.
    ``dz_into`` (two contiguous device tensors of z_s's / z_t's size): d z ADDED into them and returned."""
    lib = _lib_ready()
    rc, rf = _opt(rgb_coarse, "rgb_coarse"), _opt(rgb_fine, "rgb_fine")
    target = _cuda(target, "target")
    n = (rc if rc is not None else rf).shape[0]
    zs, zt = _opt(z_s, "z_s"), _opt(z_t, "z_t")
    n_code = 0 if zs is None else zs.numel()
    outs = [torch.empty_like(t) if (w and t is not None) else None for w, t in zip(want, (rc, rf, zs, zt))]
    if dz_into is not None:
        for d in dz_into:
            assert d.is_cuda and d.dtype == torch.float32 and d.is_contiguous() and d.numel() == n_code
        outs[2], outs[3] = dz_into
    check(lib.cn_render_loss_backward(ptr(rc), ptr(rf), ptr(target), target.shape[1], n, ptr(zs), ptr(zt), n_code,
                                      expand, regularizer_lambda, ptr(stats), ptr(_cuda(grad_total, "grad")),
                                      *[ptr(o) for o in outs], int(dz_into is not None), stream_of(target)),
          "cn_render_loss_backward")
    return tuple(outs)


# ------------------------------------------------------------------ SRN data resident in HBM


def srn_unpack(images: Tensor, view_index: Tensor, want_color: bool = True, want_mask: bool = True):
    """dataset.py:77-80 for a batch of resident uint8 views (n, h, w, c) -> color (B, h, w, c) float,
    mask (B, h, w, 1) float (either None when not wanted)."""
    lib = _lib_ready()
    images = _cuda(images, "images", torch.uint8)
    idx = _cuda(view_index, "view_index", torch.int64).reshape(-1)
    n, h, w, c = images.shape
    b = idx.numel()
    color = torch.empty(b, h, w, c, device=images.device, dtype=torch.float32) if want_color else None
    mask = torch.empty(b, h, w, 1, device=images.device, dtype=torch.float32) if want_mask else None
    check(lib.cn_srn_unpack(ptr(images), n, h * w, c, ptr(idx), b, ptr(color), ptr(mask), stream_of(images)),
          "cn_srn_unpack")
    return color, mask
