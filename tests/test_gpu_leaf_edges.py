"""Edges and branches of the small kernels around the field: volume.hip, loss.hip, optim.hip, pose.hip,
rays.hip and the element-wise pieces of grad.hip, each against a float64 reference (the oracle on the same
fp32 inputs cast to double, gradients by autograd; tests/leaf_cases.py) at the smallest shapes that reach
the branch or loop round named in each test.  tests/test_leaf_cases_cpu.py proves on the CPU that the input
sets reach those branches and that a correct fp32 implementation fits the bounds.  Every comparison
against a bound is recorded through conftest.margin()."""
import math

import numpy as np
import pytest
import torch

import leaf_cases as L
from conftest import margin
from test_gpu_grad import GRAD_RTOL, dev  # noqa: F401
from test_gpu_train import ADAM_RTOL

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def rel_margin(test, quantity, got, ref, rtol, atol=0.0):
    """margin() of max|got - ref| against rtol * max|ref| + atol (test_gpu_grad.close's measure)."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (test, quantity, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (test, quantity, "non-finite result")
    scale = ref.abs().max().item() if ref.numel() else 0.0
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    return margin(test, quantity, err, rtol * scale + atol)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def to_dev(dev, t):
    return None if t is None else t.to(dev)


# ---------------------------------------------------------------- 1. volume render


@pytest.mark.parametrize("r,s", L.VOLUME_SHAPES)
@pytest.mark.parametrize("regime", L.VOLUME_REGIMES)
def test_volume_forward_regimes(dev, regime, r, s):
    """All five outputs vs float64 at test_volume_render_sizes' bound, non-finite positions identical."""
    from codenerf import ops
    c = L.volume_case(regime, r, s)
    got = ops.volume_render(c["raw"].to(dev), c["z"].to(dev), c["rd"].to(dev))
    ref = L.volume_forward(regime, r, s)
    name = f"leaf_volume_forward[{regime},{r}x{s}]"
    for what, a, b in zip(L.VOLUME_TERMS, got, ref):
        a = a.cpu()
        assert a.shape == b.shape, what
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b)), what
        fin = torch.isfinite(b)
        err = (a.double()[fin] - b[fin]).abs().max().item() if bool(fin.any()) else 0.0
        margin(name, what, err, L.volume_bound(s))


@pytest.mark.parametrize("r,s", L.VOLUME_SHAPES)
@pytest.mark.parametrize("regime", L.VOLUME_REGIMES)
def test_volume_backward_regimes(dev, regime, r, s):
    """test_volume_render_backward's loss with every upstream gradient (no disp term where the reference has
    acc == 0 rays): d raw, d rd vs float64 autograd; with g_disp given, the acc == 0 rays' gradients stay
    finite and equal the run without it (the q > 1e-10 guard); S = 1: zero gradients."""
    from codenerf import ops
    c = L.volume_case(regime, r, s)
    raw, z, rd = c["raw"].to(dev), c["z"].to(dev), c["rd"].to(dev)
    terms = L.volume_loss_terms(regime)
    up = {k: v.to(dev) for k, v in L.volume_upstream(regime, r, s, terms).items()}
    d_raw, d_rd = ops.volume_render_backward(raw, z, rd, **up)
    name = f"leaf_volume_backward[{regime},{r}x{s}]"
    if s == 1:
        full = {k: v.to(dev) for k, v in L.volume_upstream(regime, r, s, L.VOLUME_TERMS).items()}
        d_raw, d_rd = ops.volume_render_backward(raw, z, rd, **full)
        assert not bool(d_raw.any()) and not bool(d_rd.any())
        return
    ref_raw, ref_rd = L.volume_grads(regime, r, s, terms)
    rel_margin(name, "d raw", d_raw, ref_raw, GRAD_RTOL, 1e-7)
    rel_margin(name, "d rd", d_rd, ref_rd, GRAD_RTOL, 1e-7)
    if regime in L.VOLUME_NO_DISP:
        dead = L.volume_zero_acc_rays(regime, r, s).to(dev)
        assert dead.numel() >= 2
        w_raw, w_rd = ops.volume_render_backward(raw, z, rd, g_disp=c["g_disp"].to(dev), **up)
        assert bool(torch.isfinite(w_raw[dead]).all()) and bool(torch.isfinite(w_rd[dead]).all())
        assert bits_equal(w_raw[dead], d_raw[dead]) and bits_equal(w_rd[dead], d_rd[dead])


VARIANT_REGIMES = ("opaque", "ties")


@pytest.mark.parametrize("s", L.VOLUME_VARIANT_S)
@pytest.mark.parametrize("regime,term", L.VOLUME_SINGLE_UPSTREAM)
def test_volume_backward_single_upstream(dev, regime, term, s):
    """Each upstream gradient alone, the other four NULL (g_acc on the transparent regime, the only one whose
    d acc is not identically zero: leaf_cases.VOLUME_SINGLE_UPSTREAM)."""
    from codenerf import ops
    r = 21
    c = L.volume_case(regime, r, s)
    up = {k: v.to(dev) for k, v in L.volume_upstream(regime, r, s, (term,)).items()}
    d_raw, d_rd = ops.volume_render_backward(c["raw"].to(dev), c["z"].to(dev), c["rd"].to(dev), **up)
    ref_raw, ref_rd = L.volume_grads(regime, r, s, (term,))
    name = f"leaf_volume_backward_only_{term}[{regime},{r}x{s}]"
    rel_margin(name, "d raw", d_raw, ref_raw, GRAD_RTOL, 1e-7)
    rel_margin(name, "d rd", d_rd, ref_rd, GRAD_RTOL, 1e-7)


@pytest.mark.parametrize("s", L.VOLUME_VARIANT_S)
@pytest.mark.parametrize("regime", VARIANT_REGIMES)
def test_volume_backward_rd_variants(dev, regime, s):
    """want_rd=False leaves d raw unchanged; d_rd_into pre-filled ends as pre-fill + the plain d rd, bit for bit."""
    from codenerf import ops
    r = 21
    c = L.volume_case(regime, r, s)
    raw, z, rd = c["raw"].to(dev), c["z"].to(dev), c["rd"].to(dev)
    up = {k: v.to(dev) for k, v in L.volume_upstream(regime, r, s, L.VOLUME_TERMS).items()}
    d_raw, d_rd = ops.volume_render_backward(raw, z, rd, **up)
    n_raw, n_rd = ops.volume_render_backward(raw, z, rd, want_rd=False, **up)
    assert n_rd is None and bits_equal(n_raw, d_raw)
    fill = torch.randn(r, 3, generator=torch.Generator().manual_seed(s)).to(dev)
    into = fill.clone()
    a_raw, a_rd = ops.volume_render_backward(raw, z, rd, d_rd_into=into, **up)
    assert a_rd.data_ptr() == into.data_ptr() and bits_equal(a_raw, d_raw)
    assert bits_equal(a_rd, fill + d_rd)


# ---------------------------------------------------------------- 2. loss


def _run_loss(dev, rc, rf, target, zs, zt, expand, psnr=False, dz_into=None):
    from codenerf import ops
    rc, rf, target, zs, zt = (to_dev(dev, t) for t in (rc, rf, target, zs, zt))
    ps = torch.full((1,), float("nan"), dtype=F64, device=dev) if psnr else None
    out = ops.render_loss(rc, rf, target, zs, zt, expand, L.LOSS_LAMBDA, psnr=ps)
    grad = torch.tensor(L.LOSS_GRAD_TOTAL, device=dev)
    grads = ops.render_loss_backward(rc, rf, target, zs, zt, expand, L.LOSS_LAMBDA, out, grad, dz_into=dz_into)
    return out, grads, ps


def _check_loss(name, out, grads, ps, ref, which_psnr):
    ref_out, *ref_grads = ref
    out = out.double().cpu()
    for k, what in enumerate(("loss_coarse", "loss_fine", "regulariser", "total")):
        margin(name, what, abs(out[k].item() - ref_out[k].item()), 1e-5 * abs(ref_out[k].item()))
    for k, what in ((4, "norm z_s"), (5, "norm z_t")):
        margin(name, what, abs(out[k].item() - ref_out[k].item()), 1e-6 * abs(ref_out[k].item()))
    for got, want, what in zip(grads, ref_grads, ("d rgb_coarse", "d rgb_fine", "d z_s", "d z_t")):
        assert (got is None) == (want is None), what
        if got is not None:
            rel_margin(name, what, got, want, 1e-5)
    if ps is not None:
        mse = out[which_psnr].item()                 # float64 of the fp32 loss the kernel wrote
        want = -10.0 * math.log10(mse if mse != 0.0 else 1e-5)
        margin(name, "psnr", abs(ps.item() - want), 1e-12 * abs(want))


@pytest.mark.parametrize("mode", ["coarse", "fine", "both"])
@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("n_rays", L.LOSS_RAYS)
def test_loss_rounds_strides_and_null_inputs(dev, n_rays, stride, mode):
    """3, 4095 and 4098 elements (the second, ragged round), target stride 3 and 4, rgb_coarse / rgb_fine
    NULL, psnr of the fine loss (of the coarse one when there is no fine), upstream gradient 0.37."""
    c = L.loss_case(n_rays, stride)
    rc = c["rgb_c"] if mode != "fine" else None
    rf = c["rgb_f"] if mode != "coarse" else None
    out, grads, ps = _run_loss(dev, rc, rf, c["target"], c["z_s"], c["z_t"], 300, psnr=True)
    ref = L.loss_reference(rc, rf, c["target"], c["z_s"], c["z_t"], 300)
    _check_loss(f"leaf_loss[{n_rays},stride{stride},{mode}]", out, grads, ps, ref, 0 if mode == "coarse" else 1)
    if mode == "coarse":
        assert out[1].item() == 0.0
    if mode == "fine":
        assert out[0].item() == 0.0


@pytest.mark.parametrize("expand", [1, 300])
@pytest.mark.parametrize("codes", L.LOSS_CODES)
def test_loss_code_sizes(dev, codes, expand):
    """No codes, 256, 2048 (the last size summed by the loss kernel itself) and 2304 (partial blocks, the last
    one ragged) code values, as a table (expand 1) and as one row expanded over 300 rays."""
    from codenerf import _lib
    n_code = codes[0] * codes[1]
    assert int(_lib.load().cn_render_loss_workspace_doubles(n_code)) == (0 if n_code <= 2048 else 2 * 3)
    c = L.loss_case(1366, 4, codes)
    out, grads, ps = _run_loss(dev, c["rgb_c"], c["rgb_f"], c["target"], c["z_s"], c["z_t"], expand, psnr=True)
    ref = L.loss_reference(c["rgb_c"], c["rgb_f"], c["target"], c["z_s"], c["z_t"], expand)
    _check_loss(f"leaf_loss_codes[{n_code},expand{expand}]", out, grads, ps, ref, 1)
    if n_code == 0:
        assert out[2].item() == 0.0 and out[4].item() == 0.0 and out[5].item() == 0.0


def test_loss_workspace_boundary(dev):
    from codenerf import _lib
    ws = _lib.load().cn_render_loss_workspace_doubles
    assert [int(ws(n)) for n in (0, 1, 2048, 2049, 3072, 3073)] == [0, 0, 0, 6, 6, 8] and int(ws(-1)) == -1


def test_loss_zero_norm_guard(dev):
    """z_s all zero: d z_s == 0 exactly (torch's norm backward at 0), d z_t as with a non-zero z_s."""
    c = L.loss_case(1366, 4, (9, 256))
    zero = torch.zeros_like(c["z_s"])
    out, grads, _ = _run_loss(dev, c["rgb_c"], c["rgb_f"], c["target"], zero, c["z_t"], 300)
    assert out[4].item() == 0.0 and not bool(grads[2].any())
    ref = L.loss_reference(c["rgb_c"], c["rgb_f"], c["target"], zero, c["z_t"], 300)
    _check_loss("leaf_loss_zero_norm", out, grads, None, ref, 1)
    _, plain, _ = _run_loss(dev, c["rgb_c"], c["rgb_f"], c["target"], c["z_s"], c["z_t"], 300)
    assert bits_equal(grads[3], plain[3])


def test_loss_zero_mse_psnr(dev):
    """rgb_fine == target: out[1] == 0 and psnr is mse2psnr's 1e-5 branch, exactly."""
    c = L.loss_case(1366, 4)
    rf = c["target"][:, :3].contiguous()
    out, grads, ps = _run_loss(dev, c["rgb_c"], rf, c["target"], c["z_s"], c["z_t"], 300, psnr=True)
    assert out[1].item() == 0.0 and not bool(grads[1].any())
    assert ps.item() == -10.0 * math.log10(1e-5), ps.item()
    ref = L.loss_reference(c["rgb_c"], rf, c["target"], c["z_s"], c["z_t"], 300)
    _check_loss("leaf_loss_zero_mse", out, grads, None, ref, 1)


@pytest.mark.parametrize("codes", [(1, 256), (9, 256)])
def test_loss_backward_accumulates_dz(dev, codes):
    """dz_into pre-filled: pre-fill + the plain gradients, bit for bit."""
    c = L.loss_case(1365, 3, codes)
    _, plain, _ = _run_loss(dev, c["rgb_c"], c["rgb_f"], c["target"], c["z_s"], c["z_t"], 300)
    g = torch.Generator().manual_seed(codes[0])
    fill = [torch.randn(*codes, generator=g).to(dev) * 1e-3 for _ in range(2)]
    into = tuple(f.clone() for f in fill)
    _, acc, _ = _run_loss(dev, c["rgb_c"], c["rgb_f"], c["target"], c["z_s"], c["z_t"], 300, dz_into=into)
    assert acc[2].data_ptr() == into[0].data_ptr() and acc[3].data_ptr() == into[1].data_ptr()
    assert bits_equal(acc[2], fill[0] + plain[2]) and bits_equal(acc[3], fill[1] + plain[3])
    assert bits_equal(acc[0], plain[0]) and bits_equal(acc[1], plain[1])


# ---------------------------------------------------------------- 3. AdamW


@pytest.mark.parametrize("device_scalars", [False, True])
def test_adamw_flat_segments_two_launches(dev, device_scalars):
    """ops.adamw_step / adamw_step_dev on 11 segments (two launches of at most 8; the second launch's scalars
    start at 3 * 8), each with its own lr, weight decay and step, betas (0.3, 0.95): vs torch's fp32 CPU
    AdamW per segment at ADAM_RTOL and its float64 run at ADAM_F64_BOUND, exp_avg also bit for bit (the lerp
    form); every element outside the segments (before, between and after them) keeps param, exp_avg and
    exp_avg_sq bit for bit."""
    from codenerf import ops
    n, segs = L.adam_flat_case()
    assert len(segs) == 11 > 8
    g = torch.Generator().manual_seed(7)
    p0, gr = torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g) * 1e-2
    m0, v0 = torch.randn(n, generator=g) * 1e-2, torch.rand(n, generator=g) * 1e-4
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    b1, b2 = L.ADAM_BETAS
    if device_scalars:
        host = np.zeros(3 * len(segs), dtype=np.float32)
        ops.adamw_scalars(segs, b1, b2, host)
        ops.adamw_step_dev(p, gr.to(dev), m, v, segs, torch.from_numpy(host).to(dev), b1, b2, L.ADAM_EPS)
    else:
        ops.adamw_step(p, gr.to(dev), m, v, segs, b1, b2, L.ADAM_EPS)
    inside = torch.zeros(n, dtype=torch.bool)
    for b, e, *_ in segs:
        inside[b:e] = True
    assert int((~inside[segs[0][0]:segs[-1][1]]).sum()) > 0
    for got, was in ((p, p0), (m, m0), (v, v0)):
        assert bits_equal(got.cpu()[~inside], was[~inside])
    name = f"leaf_adamw_flat[{'dev' if device_scalars else 'host'}]"
    for dtype, bound in ((F32, ADAM_RTOL), (F64, L.ADAM_F64_BOUND)):
        ref = L.adam_flat_reference(p0, gr, m0, v0, segs, dtype)
        for got, want, what in zip((p, m, v), ref, ("param", "exp_avg", "exp_avg_sq")):
            rel_margin(name, f"{what} vs torch {str(dtype)[6:]}", got.cpu()[inside], want[inside], bound)
        if dtype == F32:
            # the two lerp forms are the same number up to rounding (an ulp or more of exp_avg, far below
            # ADAM_RTOL): the kernel takes torch's form for this beta1 with torch's fused multiply-add, so
            # one step's exp_avg is torch's fp32 CPU lerp bit for bit
            assert bits_equal(m.cpu()[inside], ref[1][inside]), "exp_avg is not torch's lerp form"


@pytest.mark.parametrize("weight_decay", [0.0, 0.5])
def test_adamw_optimizer_two_launches(dev, weight_decay):
    """codenerf.optim.AdamW on 24 small parameters, every other one without a gradient: 12 non-adjacent
    segments, betas (0.3, 0.95), 4 steps, vs torch.optim.AdamW(foreach=False) in fp32 (ADAM_RTOL) and float64
    (ADAM_F64_BOUND); graph_scalars + graph_step is bit-identical to step(); a parameter without a gradient
    keeps its bits."""
    from codenerf.optim import AdamW
    groups, has_grad = L.adam_layout()

    def make():
        ps = [[torch.nn.Parameter(t.clone().to(dev)) for t in grp] for grp in groups]
        opt = AdamW([{"params": grp, "lr": lr} for grp, lr in zip(ps, L.ADAM_GROUP_LRS)], betas=L.ADAM_BETAS,
                    eps=L.ADAM_EPS, weight_decay=weight_decay)
        return ps, opt
    (pa, oa), (pb, ob) = make(), make()
    ob.zero_grad(set_to_none=False)
    for grp, hh in zip(pb, has_grad):
        for p, h in zip(grp, hh):
            if not h:
                p.grad = None
    n_seg = 12
    scal = torch.zeros(3 * n_seg, dtype=F32, device=dev)
    host = np.zeros(3 * n_seg, dtype=np.float32)
    for it in range(L.ADAM_STEPS):
        grads = L.adam_grads(it)
        oa.zero_grad()
        for ps in (pa, pb):
            for grp, gg, hh in zip(ps, grads, has_grad):
                for p, gr, h in zip(grp, gg, hh):
                    if h and ps is pa:
                        p.grad = gr.to(dev)
                    elif h:
                        p.grad.copy_(gr.to(dev))
        if it == 0:
            segs = oa._plan(advance=False)
            assert len(segs) == n_seg >= 11 and all(a[1] < b[0] for a, b in zip(segs, segs[1:]))
            assert any(segs[k][2] != segs[k + 8][2] for k in range(n_seg - 8))
        oa.step()
        ob.graph_scalars(host)
        scal.copy_(torch.from_numpy(host))
        assert ob.graph_step(scal) == n_seg
    torch.cuda.synchronize()

    def state(ps, opt):
        return [(p.detach(), opt.state[p].get("exp_avg"), opt.state[p].get("exp_avg_sq")) for grp in ps for p in grp]
    got, graph = state(pa, oa), state(pb, ob)
    flat_grad = [h for hh in has_grad for h in hh]
    flat_init = [t for grp in groups for t in grp]
    for a, b, h, t0 in zip(got, graph, flat_grad, flat_init):
        assert bits_equal(a[0], b[0])
        if h:
            assert bits_equal(a[1], b[1]) and bits_equal(a[2], b[2])
        else:
            assert a[1] is None and bits_equal(a[0].cpu(), t0)
    name = f"leaf_adamw_optimizer[wd{weight_decay}]"
    for dtype, bound in ((F32, ADAM_RTOL), (F64, L.ADAM_F64_BOUND)):
        for what, err in L.adam_err(got, L.adam_torch_run(weight_decay, dtype)).items():
            margin(name, f"{what} vs torch {str(dtype)[6:]}", err, bound)


# ---------------------------------------------------------------- 4. rays and pose


def _dirs(dev, h=L.RAY_H, w=L.RAY_W):
    """The kernel's own directions; the references use the oracle's, the same bits."""
    from codenerf import ops
    d = ops.ray_directions(h, w, *L.RAY_INTRINSICS, dev)
    assert torch.equal(d.cpu(), L.ray_dirs(h, w))
    return d


def _pose_backward(dev, name, kind, path, which):
    from codenerf import ops
    c = L.pose_case(kind)
    g_ro = c["g_ro"] if which != "rd" else None
    g_rd = c["g_rd"] if which != "ro" else None
    sel = c["sel"]
    dirs = _dirs(dev)
    kw = {"angles": c["angles"]} if path == "angles" else {"c2w": c["c2w"]}
    ref_ang, ref_c2w = L.pose_grads(L.ray_dirs(), sel, g_ro, g_rd, F64, **kw)
    own_ang, own_c2w = L.pose_grads(L.ray_dirs(), sel, g_ro, g_rd, F32, **kw)
    th, ph, rh = (a.to(dev) for a in c["angles"]) if path == "angles" else (None, None, None)
    (d_th, d_ph, d_rh), d_c2w = ops.pose_rays_backward(dirs, L.RAY_B, to_dev(dev, g_ro), to_dev(dev, g_rd), th, ph, rh,
                                                       to_dev(dev, sel), want_c2w=True)
    assert not bool(d_c2w[:, 3].any()), "row 3 of d c2w"
    bound = L.ray_bound(ref_c2w, own_c2w)
    rel_margin(name, "d c2w", d_c2w, ref_c2w, bound, 0.0)
    if path == "angles":
        for got, want, own, what in zip((d_th, d_ph, d_rh), ref_ang, own_ang, ("d theta", "d phi", "d rho")):
            rel_margin(name, what, got, want, L.ray_bound(want, own))
    else:
        assert d_th is None


@pytest.mark.parametrize("kind", L.POSE_SELECTIONS, ids=lambda k: f"sel_{k}")
@pytest.mark.parametrize("path", ["angles", "c2w"])
def test_pose_rays_backward_rounds(dev, path, kind):
    """sample sizes 1, 2047, 2049, the whole 4608-ray bundle (select_inds NULL: three rounds of 2 x 1024) and an
    index list with repeats; the angle path also asks for d c2w (row 3 zero)."""
    _pose_backward(dev, f"leaf_pose_rays_backward[{path},{kind}]", kind, path, "both")


@pytest.mark.parametrize("which", ["ro", "rd"])
@pytest.mark.parametrize("path", ["angles", "c2w"])
def test_pose_rays_backward_single_upstream(dev, path, which):
    _pose_backward(dev, f"leaf_pose_rays_backward[{path},2049,g_{which} only]", 2049, path, which)


def _scatter_case(kind, seed):
    sel = L.selection(kind)
    g = torch.Generator().manual_seed(seed)
    n = sel.numel()
    return sel, torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)


def test_gather_rays_backward_unique_is_index_add_bitwise(dev):
    """Unique indices: every destination gets a single add, so the result is index_add_ on zeros, bit for bit."""
    from codenerf import ops
    sel, g_ro, g_rd = _scatter_case(2049, 1)
    d_ro, d_rd = ops.gather_rays_backward(g_ro.to(dev), g_rd.to(dev), L.RAY_B, L.RAY_HW, sel.to(dev))
    assert bits_equal(d_ro.cpu(), L.scatter_reference(g_ro, sel, L.RAY_HW, F32))
    assert bits_equal(d_rd.cpu(), L.scatter_reference(g_rd, sel, L.RAY_HW, F32))
    only_ro, zero_rd = ops.gather_rays_backward(g_ro.to(dev), None, L.RAY_B, L.RAY_HW, sel.to(dev))
    assert bits_equal(only_ro, d_ro) and not bool(zero_rd.any())


def test_gather_rays_backward_repeated_indices(dev):
    """Indices drawn with replacement (>= 10 % repeats, two of them in neighbouring lanes): a scatter-ADD,
    vs float64 index_add_ at 1e-6 relative."""
    from codenerf import ops
    sel, g_ro, g_rd = _scatter_case("repeat", 2)
    assert L.repeated_fraction(sel) >= 0.10
    d_ro, d_rd = ops.gather_rays_backward(g_ro.to(dev), g_rd.to(dev), L.RAY_B, L.RAY_HW, sel.to(dev))
    rel_margin("leaf_gather_rays_backward[repeat]", "d ro", d_ro, L.scatter_reference(g_ro, sel, L.RAY_HW, F64), 1e-6)
    rel_margin("leaf_gather_rays_backward[repeat]", "d rd", d_rd, L.scatter_reference(g_rd, sel, L.RAY_HW, F64), 1e-6)


def test_out_of_range_indices(dev):
    """Indices -1 and hw: exactly those rays (and their target rows) are NaN in cn_gather_rays and cn_pose_rays,
    every other row is unchanged; both backwards ignore those rows."""
    from codenerf import ops
    good = L.selection(2049)
    bad, mask = L.with_bad_indices(good, L.RAY_HW)
    rows = mask.reshape(-1)
    c = L.pose_case(2049)
    dirs = _dirs(dev)
    ro_b, rd_b = ops.ray_bundle(dirs, c["c2w"].to(dev))
    ro_b, rd_b = ro_b.reshape(L.RAY_B, -1, 3), rd_b.reshape(L.RAY_B, -1, 3)
    target = torch.rand(L.RAY_B, L.RAY_HW, 4, generator=torch.Generator().manual_seed(3)).to(dev)
    th, ph, rh = (a.to(dev) for a in c["angles"])
    for fwd in ("gather", "pose"):
        if fwd == "gather":
            want = ops.gather_rays(ro_b, rd_b, good.to(dev))
            got = ops.gather_rays(ro_b, rd_b, bad.to(dev))
        else:
            ro, rd, pose, tp = ops.pose_rays(dirs, th, ph, rh, select_inds=good.to(dev), target=target)
            want = (ro, rd, tp)
            ro, rd, pose2, tp = ops.pose_rays(dirs, th, ph, rh, select_inds=bad.to(dev), target=target)
            got = (ro, rd, tp)
            assert bits_equal(pose, pose2)
        for a, b in zip(got, want):
            a, b = a.cpu(), b.cpu()
            assert torch.equal(torch.isnan(a), rows[:, None].expand_as(a)), fwd
            assert bits_equal(a[~rows], b[~rows]) and bool(torch.isfinite(b).all()), fwd
    d_ro, d_rd = ops.gather_rays_backward(c["g_ro"].to(dev), c["g_rd"].to(dev), L.RAY_B, L.RAY_HW, bad.to(dev))
    assert bits_equal(d_ro.cpu(), L.scatter_reference(c["g_ro"], bad, L.RAY_HW, F32))
    assert bits_equal(d_rd.cpu(), L.scatter_reference(c["g_rd"], bad, L.RAY_HW, F32))
    ref_ang, ref_c2w = L.pose_grads(L.ray_dirs(), bad, c["g_ro"], c["g_rd"], F64, angles=c["angles"])
    own_ang, own_c2w = L.pose_grads(L.ray_dirs(), bad, c["g_ro"], c["g_rd"], F32, angles=c["angles"])
    d_ang, d_c2w = ops.pose_rays_backward(dirs, L.RAY_B, c["g_ro"].to(dev), c["g_rd"].to(dev), th, ph, rh, bad.to(dev),
                                          want_c2w=True)
    rel_margin("leaf_pose_rays_backward[out of range]", "d c2w", d_c2w, ref_c2w, L.ray_bound(ref_c2w, own_c2w))
    for got, want, own, what in zip(d_ang, ref_ang, own_ang, ("d theta", "d phi", "d rho")):
        rel_margin("leaf_pose_rays_backward[out of range]", what, got, want, L.ray_bound(want, own))


@pytest.mark.parametrize("which", ["both", "ro", "rd"])
@pytest.mark.parametrize("h,w", L.BUNDLE_SHAPES)
def test_ray_bundle_backward_sizes(dev, h, w, which):
    """hw = 1, 192, 4608 with batch 3, g_ro / g_rd alone; through the C ABI, a pre-filled d c2w has rows 0..2
    accumulated into and row 3 untouched."""
    from codenerf import _lib, ops
    hw = h * w
    dirs = _dirs(dev, h, w)
    c = L.pose_case(None, L.RAY_B, hw)
    g_ro = c["g_ro"] if which != "rd" else None
    g_rd = c["g_rd"] if which != "ro" else None
    d = ops.ray_bundle_backward(dirs, L.RAY_B, to_dev(dev, g_ro), to_dev(dev, g_rd))
    _, ref = L.pose_grads(L.ray_dirs(h, w), None, g_ro, g_rd, F64, c2w=c["c2w"])
    _, own = L.pose_grads(L.ray_dirs(h, w), None, g_ro, g_rd, F32, c2w=c["c2w"])
    rel_margin(f"leaf_ray_bundle_backward[hw{hw},{which}]", "d c2w", d, ref, L.ray_bound(ref, own))
    fill = torch.randn(L.RAY_B, 4, 4, generator=torch.Generator().manual_seed(hw)).to(dev)
    into = fill.clone()
    gro, grd = to_dev(dev, g_ro), to_dev(dev, g_rd)
    _lib.check(_lib.load().cn_ray_bundle_backward(_lib.ptr(dirs), hw, L.RAY_B, _lib.ptr(gro), _lib.ptr(grd), _lib.ptr(into),
                                                  _lib.stream_of(into)), "cn_ray_bundle_backward")
    assert bits_equal(into[:, :3], fill[:, :3] + d[:, :3]) and bits_equal(into[:, 3], fill[:, 3])
    assert not bool(d[:, 3].any())


@pytest.mark.parametrize("want", ["both", "ro", "rd"])
@pytest.mark.parametrize("r,s", L.POINTS_SHAPES)
def test_ray_points_backward_sizes(dev, r, s, want):
    """(R, S) = (1, 1), (257, 7), (300, 192): d ro, d rd vs float64, each alone, and accumulated into pre-filled
    outputs through the C ABI (pre-fill + the plain result, bit for bit)."""
    from codenerf import _lib, ops
    c = L.points_case(r, s)
    g_pts, z = c["g_pts"].to(dev), c["z"].to(dev)
    d_ro, d_rd = ops.ray_points_backward(g_pts, z, want_ro=want != "rd", want_rd=want != "ro")
    ref_ro, ref_rd = L.points_reference(c["g_pts"], c["z"])
    name = f"leaf_ray_points_backward[{r}x{s},{want}]"
    assert (d_ro is None) == (want == "rd") and (d_rd is None) == (want == "ro")
    g = torch.Generator().manual_seed(r + s)
    for got, ref, what in ((d_ro, ref_ro, "d ro"), (d_rd, ref_rd, "d rd")):
        if got is not None:
            rel_margin(name, what, got, ref, 1e-5)
    fill = [torch.randn(r, 3, generator=g).to(dev) for _ in range(2)]
    into = [f.clone() if got is not None else None for f, got in zip(fill, (d_ro, d_rd))]
    _lib.check(_lib.load().cn_ray_points_backward(_lib.ptr(g_pts), _lib.ptr(z), r, s, _lib.ptr(into[0]), _lib.ptr(into[1]),
                                                  _lib.stream_of(z)), "cn_ray_points_backward")
    for acc, f, got in zip(into, fill, (d_ro, d_rd)):
        if got is not None:
            assert bits_equal(acc, f + got)


# ---------------------------------------------------------------- 5. positional encoding


@pytest.mark.parametrize("m", L.POSENC_ROWS)
@pytest.mark.parametrize("config", [c[0] for c in L.POSENC_CONFIGS])
def test_posenc_configurations(dev, config, m):
    """cn_posenc / cn_posenc_backward over (d, L, include_input, log_sampling) incl. L = 0 (identity), no
    input block, linear bands and |x| ~ 100, vs float64 sin / cos of the fp32 product."""
    from codenerf import ops
    c = L.posenc_case(config, m)
    freqs = [float(f) for f in c["freqs"]]
    x = c["x"].to(dev)
    enc = ops.posenc(x, freqs, c["inc"])
    dx = ops.posenc_backward(x, freqs, c["inc"], c["g"].to(dev))
    ref_enc, ref_dx = L.posenc_reference(c["x"], c["freqs"], c["inc"], c["g"])
    name = f"leaf_posenc[{config},{m}]"
    assert enc.shape == ref_enc.shape and bool(torch.isfinite(enc).all())
    margin(name, "forward", (enc.double().cpu() - ref_enc).abs().max().item(), L.POSENC_FWD_ATOL)
    rel_margin(name, "backward", dx, ref_dx, L.POSENC_BWD_RTOL)
    if config == "identity":
        assert bits_equal(enc, x) and bits_equal(dx.cpu(), c["g"])


# ---------------------------------------------------------------- 6. SE3 pose error


def _check_pose_error(name, twist, err, ref_twist, ref_err, rows=slice(None)):
    twist, err = twist.cpu()[rows], err.cpu()[rows]
    ref_twist, ref_err = ref_twist[rows], ref_err[rows]
    rel_margin(name, "twist", twist, ref_twist, L.SE3_TWIST_RTOL, 1e-7)
    excess = ((err.double() - ref_err.double()).abs() / (L.SE3_ERR_RTOL * ref_err.double().abs() + L.SE3_ERR_ATOL)).max()
    margin(name, "err / (2e-5 |err| + 2e-6)", excess.item(), 1.0)


def test_pose_error_degenerate_angles(dev):
    """224 poses (four workgroups, the last ragged): 32 axes x rotation angles pi, pi - 1e-4 (the
    |sin t / t| <= 1e-7 branch), pi - 1e-3, 0, 1e-4, 5e-4 (the Taylor branch), 2e-3, vs the oracle's se3_log in
    FP32 on the CPU (the branch taken is a fact of fp32 rounding)."""
    from codenerf import ops
    gt, cam = L.se3_degenerate()
    twist, err = ops.pose_error(gt.to(dev), cam.to(dev))
    ref_twist, ref_err = L.se3_reference(gt, cam, F32)
    for k, angle in enumerate(L.SE3_ANGLES):
        rows = slice(k * L.SE3_AXES, (k + 1) * L.SE3_AXES)
        _check_pose_error(f"leaf_pose_error[angle {angle:.6f}]", twist, err, ref_twist, ref_err, rows)


def test_pose_error_general_poses(dev):
    """32 pose_spherical pairs, relative rotation 0.3 .. 2.5 rad, general gt: vs float64."""
    from codenerf import ops
    gt, cam = L.se3_general()
    twist, err = ops.pose_error(gt.to(dev), cam.to(dev))
    _check_pose_error("leaf_pose_error[general]", twist, err, *L.se3_reference(gt, cam, F64))
