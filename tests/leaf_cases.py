"""Input builders and float64 references for the edge / branch tests of the small kernels
(volume.hip, loss.hip, optim.hip, pose.hip, rays.hip, the element-wise pieces of grad.hip).

Shared by tests/test_leaf_cases_cpu.py (which proves on the CPU that every input set reaches the
branch it is built for and that the oracle's own fp32 run stays inside the stated bounds) and
tests/test_gpu_leaf_edges.py (which runs the kernels).  Everything here is CPU torch; every builder
is seeded, and every reference is computed once per case (lru_cache) and must not be modified.

The float64 reference of an operation is oracle/codenerf_oracle.py run on the same fp32 inputs cast
to double, gradients by torch.autograd over that run.
"""
import contextlib
import functools
import math
import zlib

import torch

from oracle import codenerf_oracle as O

F32, F64 = torch.float32, torch.float64


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@contextlib.contextmanager
def default_dtype(dtype):
    """The oracle's factory calls (torch.eye in pose_spherical) follow the default dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def rel_err(got, ref) -> float:
    """max|got - ref| relative to the reference's largest magnitude (0 for two all-zero tensors)."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    if scale == 0.0:
        return 0.0 if err == 0.0 else math.inf
    return err / scale


# ---------------------------------------------------------------------------------------------
# 1. volume render
# ---------------------------------------------------------------------------------------------

VOLUME_REGIMES = ("opaque", "transparent", "ties", "rdscale", "satcol", "zero_rd")
# S = 1 (sample-free), 2, 7 (16 lanes, run 1), 64 / 128 (FULL), 65 (16 lanes, run 8), 129 (64 lanes, run 4),
# 300 (64 lanes, run 8); 21 rays: a ragged last wave at 16 lanes per ray, six workgroups at 64 lanes per
# ray; 20 rays at S = 64: the grouped forward launch
VOLUME_SHAPES = tuple((21, s) for s in (1, 2, 7, 64, 65, 128, 129, 300)) + ((20, 64),)
VOLUME_VARIANT_S = (7, 129)
VOLUME_ZERO_RD_RAYS = (3, 11)
# (regime, term) of the one-upstream-gradient-alone backward runs.  acc = 1 - exp(-sum sigma delta) saturates at
# exactly 1 wherever the last interval (1e10 long) is not transparent, so d acc is identically zero in every
# regime but ``transparent`` (a comparison there would be of rounding noise against no scale): g_acc alone
# runs on that regime, the other four on ``opaque`` and ``ties``.
VOLUME_SINGLE_UPSTREAM = tuple((regime, t) for regime in ("opaque", "ties") for t in ("rgb", "disp", "weights", "depth")) \
    + (("transparent", "acc"),)
VOLUME_TERMS = ("rgb", "disp", "acc", "weights", "depth")
# the regimes whose reference has acc == 0 rays: d disp there is 0 * inf = NaN, so their loss has no disp term
VOLUME_NO_DISP = ("transparent", "zero_rd")


def volume_bound(s: int) -> float:
    """test_volume_render_sizes' forward bound (absolute)."""
    return 5e-6 * max(1.0, s / 256)


@functools.lru_cache(maxsize=None)
def volume_case(regime: str, r: int, s: int):
    """-> dict raw (r, s, 4), z (r, s), rd (r, 3) and the upstream gradients of test_volume_render_backward's
    loss: g_rgb (r, 3), g_disp, g_acc, g_depth (r,), g_weights (r, s) (g_disp already scaled by 1e-2)."""
    g = _gen("volume", regime, r, s)
    raw = torch.randn(r, s, 4, generator=g) * 2
    z = torch.sort(0.8 + torch.rand(r, s, generator=g), dim=-1).values
    rd = torch.randn(r, 3, generator=g)
    if regime == "opaque":
        raw[:, s // 3, 3] = 25.0
        raw[::2, 0, 3] = 40.0
    elif regime == "transparent":
        raw[..., 3] = -30.0
        raw[::3, :, 3] = -100.0
    elif regime == "ties":
        z[:, 1::2] = z[:, 0::2][:, :z[:, 1::2].shape[1]]
        z[::4, :] = z[::4, :1]
    elif regime == "rdscale":
        rd[::2] *= 1e3
        rd[1::2] *= 1e-3
    elif regime == "satcol":
        raw[..., :3] = torch.where(torch.rand(r, s, 3, generator=g) < 0.5, -40.0, 40.0)
    elif regime == "zero_rd":
        rd[list(VOLUME_ZERO_RD_RAYS)] = 0.0
    else:
        raise KeyError(regime)
    return {"raw": raw, "z": z, "rd": rd,
            "g_rgb": torch.randn(r, 3, generator=g), "g_disp": 1e-2 * torch.randn(r, generator=g),
            "g_acc": torch.randn(r, generator=g), "g_weights": torch.randn(r, s, generator=g),
            "g_depth": torch.randn(r, generator=g)}


@functools.lru_cache(maxsize=None)
def volume_forward(regime: str, r: int, s: int, dtype=F64):
    """The oracle's (rgb, disp, acc, weights, depth) on the case's inputs cast to ``dtype``."""
    c = volume_case(regime, r, s)
    with torch.no_grad():
        return tuple(O.volume_render(c["raw"].to(dtype), c["z"].to(dtype), c["rd"].to(dtype)))


def volume_zero_acc_rays(regime: str, r: int, s: int) -> torch.Tensor:
    """Rays whose float64 reference has acc == 0 exactly (disp NaN)."""
    return (volume_forward(regime, r, s)[2] == 0).nonzero().flatten()


def volume_loss_terms(regime: str):
    return tuple(t for t in VOLUME_TERMS if not (t == "disp" and regime in VOLUME_NO_DISP))


@functools.lru_cache(maxsize=None)
def volume_grads(regime: str, r: int, s: int, terms, dtype=F64):
    """d raw, d rd of sum over ``terms`` of <output, its upstream gradient> by autograd over the oracle."""
    c = volume_case(regime, r, s)
    raw = c["raw"].to(dtype).clone().requires_grad_(True)
    rd = c["rd"].to(dtype).clone().requires_grad_(True)
    outs = dict(zip(VOLUME_TERMS, O.volume_render(raw, c["z"].to(dtype), rd)))
    loss = sum((outs[t] * c["g_" + t].to(dtype)).sum() for t in terms if outs[t].numel())
    if not torch.is_tensor(loss) or not loss.requires_grad:      # S == 1: no sample contributes
        return torch.zeros_like(raw), torch.zeros_like(rd)
    loss.backward()
    return raw.grad, rd.grad


def volume_upstream(regime: str, r: int, s: int, terms):
    """The keyword arguments of ops.volume_render_backward for ``terms`` (CPU tensors)."""
    c = volume_case(regime, r, s)
    return {"g_" + t: c["g_" + t] for t in terms}


# ---------------------------------------------------------------------------------------------
# 2. loss
# ---------------------------------------------------------------------------------------------

LOSS_RAYS = (1, 1365, 1366)          # 3, 4095 and 4098 elements: one round, one full round, a ragged second
LOSS_CODES = ((0, 0), (1, 256), (8, 256), (9, 256))   # 0; 256; 2048 (last without partial blocks); 2304
LOSS_LAMBDA = 0.01
LOSS_GRAD_TOTAL = 0.37


@functools.lru_cache(maxsize=None)
def loss_case(n_rays: int, stride: int, codes=(1, 256)):
    g = _gen("loss", n_rays, stride, codes)
    c = {"rgb_c": torch.rand(n_rays, 3, generator=g), "rgb_f": torch.rand(n_rays, 3, generator=g),
         "target": torch.rand(n_rays, stride, generator=g), "z_s": None, "z_t": None}
    if codes[0]:
        c["z_s"], c["z_t"] = torch.randn(*codes, generator=g), 0.5 * torch.randn(*codes, generator=g)
    return c


def loss_reference(rgb_c, rgb_f, target, z_s, z_t, expand, lam=LOSS_LAMBDA, grad_total=LOSS_GRAD_TOTAL):
    """float64: out (6,) [loss_coarse, loss_fine, regulariser, total, ||z_s||, ||z_t||] with ||z|| =
    sqrt(expand * sum z^2), and the gradients of grad_total * total -> (out, d rgb_c, d rgb_f, d z_s, d z_t)."""
    leaf = [None if t is None else t.double().clone().requires_grad_(True) for t in (rgb_c, rgb_f, z_s, z_t)]
    rc, rf, zs, zt = leaf
    tgt = target.double()[:, :3]
    zero = torch.zeros((), dtype=F64)
    lc = torch.nn.functional.mse_loss(rc, tgt) if rc is not None else zero
    lf = torch.nn.functional.mse_loss(rf, tgt) if rf is not None else zero

    def norm(z):      # torch.norm's backward is 0 at a zero norm (sqrt's would be 0 * inf)
        if z is None:
            return zero
        return torch.sqrt(expand * (z * z).sum()) if bool(z.any()) else (z * 0).sum()
    ns, nt = norm(zs), norm(zt)
    reg = lam * (ns + nt)
    total = lc + lf + reg
    (grad_total * total).backward()
    grads = [None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t)) for t in leaf]
    return (torch.stack([lc, lf, reg, total, ns, nt]).detach(), *grads)


# ---------------------------------------------------------------------------------------------
# 3. AdamW
# ---------------------------------------------------------------------------------------------

ADAM_BETAS = (0.3, 0.95)             # 1 - beta1 = 0.7 >= 0.5: torch's second lerp form
ADAM_STEPS = 4
ADAM_EPS = 1e-8
ADAM_GROUP_LRS = (1e-3, 3e-4, 1e-3, 3e-4)
ADAM_GROUP_SIZES = ((4, 7, 12, 40, 9, 16), (40, 5, 8, 33, 20, 4), (13, 4, 28, 6, 36, 11), (24, 39, 4, 17, 10, 32))
# 4 x (error of torch's own fp32 CPU AdamW against its float64 run on the same inputs, relative to each
# tensor kind's largest magnitude, the largest over param / exp_avg / exp_avg_sq and both weight decays).
# Measured by test_leaf_cases_cpu.test_adam_float64_bound: 1.988e-07 (weight_decay 0.5, param; exp_avg
# 4.61e-08, exp_avg_sq 4.56e-08); the margin of 4 allows for the kernel's FMA contraction differing from torch's.
ADAM_F64_ERR_MEASURED = 1.99e-07
ADAM_F64_BOUND = 4 * ADAM_F64_ERR_MEASURED


def adam_layout():
    """The optimiser-level layout: four param groups (learning rates alternating) of six parameters of 4 to
    40 floats; every other parameter never gets a gradient.  Each parameter occupies its own 64-float
    slot of the flat buffers, so the 12 parameters with gradients are 12 non-adjacent segments: two launches
    of at most 8.  Segments k and k + 8 differ in learning rate for k = 1, 2 (groups of three)."""
    g = _gen("adam-layout")
    groups = [[torch.randn(n, generator=g) * 0.1 for n in sizes] for sizes in ADAM_GROUP_SIZES]
    has_grad = [[i % 2 == 0 for i in range(len(sizes))] for sizes in ADAM_GROUP_SIZES]
    return groups, has_grad


def adam_grads(step: int):
    """Per-parameter gradients of one step (every parameter; the caller drops those without a gradient)."""
    g = _gen("adam-grads", step)
    return [[torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-4, 1, (1,), generator=g)) for n in sizes]
            for sizes in ADAM_GROUP_SIZES]


@functools.lru_cache(maxsize=None)
def adam_torch_run(weight_decay: float, dtype):
    """torch.optim.AdamW(foreach=False) on the CPU over ADAM_STEPS steps of adam_layout() -> per parameter
    (param, exp_avg | None, exp_avg_sq | None) in group order."""
    groups, has_grad = adam_layout()
    ps = [[torch.nn.Parameter(t.to(dtype).clone()) for t in grp] for grp in groups]
    opt = torch.optim.AdamW([{"params": grp, "lr": lr} for grp, lr in zip(ps, ADAM_GROUP_LRS)], betas=ADAM_BETAS,
                            eps=ADAM_EPS, weight_decay=weight_decay, foreach=False)
    for it in range(ADAM_STEPS):
        grads = adam_grads(it)
        for grp, gg, hh in zip(ps, grads, has_grad):
            for p, gr, h in zip(grp, gg, hh):
                p.grad = gr.to(dtype).clone() if h else None
        opt.step()
    out = []
    for grp in ps:
        for p in grp:
            st = opt.state.get(p, {})
            out.append((p.detach().clone(), st.get("exp_avg"), st.get("exp_avg_sq")))
    return out


def adam_err(got, ref) -> dict:
    """Per tensor kind, max|got - ref| over every parameter relative to the kind's largest |ref|."""
    out = {}
    for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
        pairs = [(a[k], b[k]) for a, b in zip(got, ref) if b[k] is not None]
        scale = max(b.double().abs().max().item() for _, b in pairs)
        out[name] = max((a.double().cpu() - b.double()).abs().max().item() for a, b in pairs) / scale
    return out


def adam_flat_case():
    """The ops-level case: one flat buffer of 1024 floats and 11 segments with gaps before, between and
    after them, every segment with its own lr, weight decay and step count -> (n, segments)."""
    segs, lo = [], 8
    for k in range(11):
        n = 4 * (1 + (5 * k) % 7)
        segs.append((lo, lo + n, 1e-3 * (1 + 0.37 * k), 0.05 * (k % 3), 1 + k % 5))
        lo += n + 4 * (1 + k % 3)
    return 1024, segs


def adam_flat_reference(param, grad, m, v, segs, dtype):
    """torch's _single_tensor_adam (decoupled decay) on each segment's slice, through torch.optim.AdamW with
    the state preset to the segment's step count - 1 -> (param, exp_avg, exp_avg_sq) flat, untouched elsewhere."""
    p_out, m_out, v_out = param.to(dtype).clone(), m.to(dtype).clone(), v.to(dtype).clone()
    for b, e, lr, wd, step in segs:
        p = torch.nn.Parameter(param[b:e].to(dtype).clone())
        opt = torch.optim.AdamW([p], lr=lr, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=wd, foreach=False)
        opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m[b:e].to(dtype).clone(),
                        "exp_avg_sq": v[b:e].to(dtype).clone()}
        p.grad = grad[b:e].to(dtype).clone()
        opt.step()
        p_out[b:e], m_out[b:e], v_out[b:e] = p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    return p_out, m_out, v_out


# ---------------------------------------------------------------------------------------------
# 4. rays and pose
# ---------------------------------------------------------------------------------------------

RAY_H, RAY_W, RAY_B = 72, 64, 3
RAY_HW = RAY_H * RAY_W               # 4608: three rounds of the pose backward's 2 x 1024 rays
RAY_INTRINSICS = (60.0, 31.5, 36.25)   # focal, cx, cy
# sample sizes of cn_pose_rays_backward: 1; 2047 / 2049 around one round of 2 x 1024; None = the whole
# bundle (select_inds NULL); "repeat": indices drawn with replacement
POSE_SELECTIONS = (1, 2047, 2049, None, "repeat")
REPEAT_S = 2049
RAY_RTOL = 1e-5                      # the project's bound on d c2w / d angles, relative to the largest magnitude


def intrinsics(focal, cx, cy, dtype=F32):
    k = torch.eye(4, dtype=dtype)
    k[0, 0] = k[1, 1] = focal
    k[0, 2], k[1, 2] = cx, cy
    return k


@functools.lru_cache(maxsize=None)
def ray_dirs(h=RAY_H, w=RAY_W):
    """fp32 directions (h, w, 3) (the kernels' input; cn_ray_directions gives the same bits)."""
    return O.ray_directions(h, w, intrinsics(*RAY_INTRINSICS))


@functools.lru_cache(maxsize=None)
def selection(kind, batch=RAY_B, hw=RAY_HW):
    """(batch, S) int64 indices, or None for the whole bundle.  "repeat": with replacement, and the first
    two rays of every image select the same pixel (neighbouring lanes of one wave)."""
    g = _gen("selection", kind, batch, hw)
    if kind is None:
        return None
    if kind == "repeat":
        sel = torch.randint(0, hw, (batch, min(REPEAT_S, hw)), generator=g)
        sel[:, 1] = sel[:, 0]
        return sel
    return torch.stack([torch.randperm(hw, generator=g)[:kind] for _ in range(batch)])


def repeated_fraction(sel: torch.Tensor) -> float:
    """Fraction of a selection's entries that repeat an earlier entry of the same image."""
    rep = sum(row.numel() - row.unique().numel() for row in sel)
    return rep / sel.numel()


@functools.lru_cache(maxsize=None)
def pose_case(kind, batch=RAY_B, hw=RAY_HW):
    g = _gen("pose", kind, batch, hw)
    sel = selection(kind, batch, hw)
    s = hw if sel is None else sel.shape[1]
    ang = (torch.rand(batch, generator=g) * 2 - 1, torch.rand(batch, generator=g) * 6 - 3,
           torch.rand(batch, generator=g) + 1)
    c2w = torch.eye(4).repeat(batch, 1, 1) + 0.1 * torch.randn(batch, 4, 4, generator=g)
    return {"sel": sel, "angles": ang, "c2w": c2w, "g_ro": torch.randn(batch * s, 3, generator=g),
            "g_rd": torch.randn(batch * s, 3, generator=g)}


def _bundle_loss(dirs, c2w, sel, g_ro, g_rd):
    """<ro, g_ro> + <rd, g_rd> over the oracle's get_bundle + gather; rows with an out-of-range index
    contribute nothing (their rays are NaN in the forward and ignored by the backward)."""
    b, hw = c2w.shape[0], dirs.shape[0] * dirs.shape[1]
    ro, rd = O.ray_bundle(dirs, c2w)
    if sel is None:
        ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
        keep = None
    else:
        ok = (sel >= 0) & (sel < hw)
        ro, rd = O.gather_rays(ro, rd, torch.where(ok, sel, 0))
        keep = ok.reshape(-1, 1).to(ro.dtype)
    loss = 0.0
    for x, gx in ((ro, g_ro), (rd, g_rd)):
        if gx is not None:
            gx = gx.to(x.dtype)
            loss = loss + (x * (gx if keep is None else gx * keep)).sum()
    return loss


def pose_grads(dirs, sel, g_ro, g_rd, dtype, angles=None, c2w=None):
    """Autograd over the oracle in ``dtype`` -> (d theta, d phi, d rho | None, d c2w (B, 4, 4))."""
    with default_dtype(dtype):
        d = dirs.to(dtype)
        if angles is not None:
            a = [x.to(dtype).clone().requires_grad_(True) for x in angles]
            pose = torch.stack([O.pose_spherical(a[0][b:b + 1], a[1][b:b + 1], a[2][b:b + 1]) for b in range(a[0].numel())])
            assert pose.dtype == dtype
            pose.retain_grad()
        else:
            a = None
            pose = c2w.to(dtype).clone().requires_grad_(True)
        _bundle_loss(d, pose, sel, g_ro, g_rd).backward()
    return (None if a is None else tuple(x.grad for x in a)), pose.grad


def ray_bound(ref64, own32) -> float:
    """The larger of the project's 1e-5 and 4 x the fp32 oracle's own error, relative to max|ref64|."""
    return max(RAY_RTOL, 4 * rel_err(own32, ref64))


def scatter_reference(g, sel, hw, dtype):
    """index_add_ of the rows g (B*S, 3) onto zeros (B, hw, 3); out-of-range indices dropped."""
    b, s = sel.shape
    ok = ((sel >= 0) & (sel < hw)).reshape(-1)
    flat = (torch.arange(b)[:, None] * hw + sel).reshape(-1)
    out = torch.zeros(b * hw, 3, dtype=dtype)
    out.index_add_(0, flat[ok], g.to(dtype)[ok])
    return out.view(b, hw, 3)


def with_bad_indices(sel: torch.Tensor, hw: int):
    """A copy of sel with -1 and hw written at a few positions of every image -> (sel, bad mask (B, S))."""
    bad = torch.zeros_like(sel, dtype=torch.bool)
    s = sel.shape[1]
    out = sel.clone()
    for b in range(sel.shape[0]):
        for k, pos in enumerate(sorted({0, (5 + 7 * b) % s, s // 2, s - 1})):
            out[b, pos] = -1 if (k + b) % 2 == 0 else hw
            bad[b, pos] = True
    return out, bad


BUNDLE_SHAPES = ((1, 1), (12, 16), (RAY_H, RAY_W))        # hw = 1, 192, 4608
POINTS_SHAPES = ((1, 1), (257, 7), (300, 192))


@functools.lru_cache(maxsize=None)
def points_case(r: int, s: int):
    g = _gen("points", r, s)
    return {"g_pts": torch.randn(r, s, 3, generator=g),
            "z": torch.sort(0.8 + torch.rand(r, s, generator=g), dim=-1).values}


def points_reference(g_pts, z, dtype=F64):
    """d ro = sum_s g_pts, d rd = sum_s g_pts z by autograd over pts = ro + rd z (z detached)."""
    r = z.shape[0]
    ro = torch.zeros(r, 3, dtype=dtype, requires_grad=True)
    rd = torch.zeros(r, 3, dtype=dtype, requires_grad=True)
    pts = ro[:, None, :] + rd[:, None, :] * z.to(dtype)[..., None]
    (pts * g_pts.to(dtype)).sum().backward()
    return ro.grad, rd.grad


# ---------------------------------------------------------------------------------------------
# 5. positional encoding
# ---------------------------------------------------------------------------------------------

# (name, d, L, include_input, log_sampling, |x| scale)
POSENC_CONFIGS = (("xyz10", 3, 10, True, True, 1.5), ("dir4", 3, 4, True, True, 1.5), ("d1_L1_noinput", 1, 1, False, True, 1.5),
                  ("identity", 5, 0, True, True, 1.5), ("linear6", 2, 6, True, False, 1.5), ("xyz10_far", 3, 10, True, True, 100.0))
POSENC_ROWS = (1, 777)
POSENC_FWD_ATOL = 2e-6
POSENC_BWD_RTOL = 1e-5


@functools.lru_cache(maxsize=None)
def posenc_case(name: str, m: int):
    _, d, nf, inc, log, scale = next(c for c in POSENC_CONFIGS if c[0] == name)
    g = _gen("posenc", name, m)
    freqs = O.frequency_bands(nf, log) if nf else torch.zeros(0)
    x = torch.randn(m, d, generator=g) * scale
    return {"x": x, "freqs": freqs, "inc": inc, "g": torch.randn(m, d * (int(inc) + 2 * nf), generator=g)}


def posenc_reference(x, freqs, inc, g=None):
    """float64 sin / cos of the FP32 product fl(x * f) (the kernel and the reference library both round the
    product first); with ``g``: also d x of <enc, g> by autograd (d arg / d x = f).  -> enc, d x | None."""
    x64 = x.double().clone().requires_grad_(True)
    parts = [x64] if inc else []
    for f in freqs:
        arg = x64 * f.double()
        arg = arg + ((x * f).double() - arg).detach()
        parts += [torch.sin(arg), torch.cos(arg)]
    enc = torch.cat(parts, dim=-1)
    if g is None:
        return enc.detach(), None
    (enc * g.double()).sum().backward()
    return enc.detach(), x64.grad


# ---------------------------------------------------------------------------------------------
# 6. SE3 pose error
# ---------------------------------------------------------------------------------------------

SE3_ANGLES = (math.pi, math.pi - 1e-4, math.pi - 1e-3, 0.0, 1e-4, 5e-4, 2e-3)
SE3_AXES = 32
SE3_TWIST_RTOL = 1e-4                # the golden test's bounds
SE3_ERR_RTOL, SE3_ERR_ATOL = 2e-5, 2e-6


def _rotation(axis: torch.Tensor, angle: float) -> torch.Tensor:
    """Rodrigues in float64."""
    a = axis.double() / axis.double().norm()
    k = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=F64)
    return torch.eye(3, dtype=F64) + math.sin(angle) * k + (1 - math.cos(angle)) * (k @ k)


@functools.lru_cache(maxsize=None)
def se3_axes():
    g = _gen("se3-axes")
    ax = torch.randn(SE3_AXES, 3, generator=g)
    ax[0], ax[1], ax[2] = torch.tensor([1.0, 0, 0]), torch.tensor([0, -1.0, 0]), torch.tensor([0, 0, 1.0])
    ax[3], ax[4], ax[5] = torch.tensor([0, 0.6, -0.8]), torch.tensor([-0.6, 0, 0.8]), torch.tensor([0.8, -0.6, 0])
    ax[6] = -ax[6].abs()
    return ax


@functools.lru_cache(maxsize=None)
def se3_degenerate():
    """224 poses, angle-major (pose i: angle i // 32, axis i % 32): gt has an identity rotation and a non-zero
    translation, so the rotation block of inverse(gt) @ cam is cam's, exactly, in every implementation."""
    g = _gen("se3-degenerate")
    n = len(SE3_ANGLES) * SE3_AXES
    cam = torch.eye(4).repeat(n, 1, 1)
    for i in range(n):
        cam[i, :3, :3] = _rotation(se3_axes()[i % SE3_AXES], SE3_ANGLES[i // SE3_AXES]).float()
    cam[:, :3, 3] = torch.randn(n, 3, generator=g)
    gt = torch.eye(4).repeat(n, 1, 1)
    # quarters: torch.inverse's LU then leaves the rotation block of inverse(gt) the exact identity (with a
    # general translation it comes out an ulp off, and the branch decision would not be the kernel's)
    sign = torch.where(torch.rand(n, 3, generator=g) < 0.5, -1.0, 1.0)
    gt[:, :3, 3] = sign * torch.randint(1, 9, (n, 3), generator=g).float() / 4
    return gt, cam


@functools.lru_cache(maxsize=None)
def se3_general():
    """32 pose_spherical pairs whose relative rotation angle lies in [0.3, 2.5]."""
    g = _gen("se3-general")
    gts, cams = [], []
    while len(gts) < 32:
        a = [torch.rand(2, generator=g) * 2 - 1, torch.rand(2, generator=g) * 6 - 3, torch.rand(2, generator=g) + 1]
        p = [O.pose_spherical(a[0][k:k + 1], a[1][k:k + 1], a[2][k:k + 1]) for k in range(2)]
        if 0.3 <= se3_relative_angle(p[0], p[1]) <= 2.5:
            gts.append(p[0])
            cams.append(p[1])
    return torch.stack(gts), torch.stack(cams)


def se3_relative_angle(gt, cam) -> float:
    r = gt.double()[:3, :3].t() @ cam.double()[:3, :3]
    return math.acos(max(-1.0, min(1.0, (torch.trace(r).item() - 1) / 2)))


def se3_reference(gt, cam, dtype):
    """The oracle's twist (B, 6) and pose error (B,) in ``dtype`` on the CPU."""
    with default_dtype(dtype):
        g = torch.matmul(torch.inverse(gt.to(dtype)), cam.to(dtype))
        tw = O.se3_log(g)
    return tw, tw.norm(p=2, dim=1)


def se3_branches(gt, cam):
    """The fp32 oracle's branch quantities: (|sin t / t| <= 1e-7, |t| < 1e-3) per pose."""
    g = torch.matmul(torch.inverse(gt), cam)
    tr = torch.stack([torch.trace(m) for m in g[:, :3, :3]])
    t = torch.acos((tr - 1) / 2)
    return O._sin_by_t(t).abs() <= 1e-7, t.abs() < 1e-3
