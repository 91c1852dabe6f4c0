"""Inputs and CPU references of the paired field backward's off-path cases (tests/test_gpu_pair_paths.py).

The eval step of eval.py:145-163 at the smallest size that reaches every branch of autograd.FieldPair:
a 16x16 view, 100 selected rays, near 0.8 / far 1.8, the synthetic models 0 / 1 and codes 5 / 6, injected
uniforms; three sample counts (a field pairs only when its samples are a multiple of 16) times three
losses (coarse + fine, fine only, coarse only).  ``eval_reference`` is the oracle's op sequence
(oracle/codenerf_oracle.py) under torch.autograd in a chosen dtype, on given fine depths; its pose matrix
is built with torch.stack, since oracle.pose_spherical fills a float32 matrix.
"""
import torch

SIZE, N_RAYS, NEAR, FAR, LAM = 16, 100, 0.8, 1.8, 1e-5
SAMPLES = [(16, 16), (32, 24), (24, 40)]
LOSSES = ["both", "fine", "coarse"]
LEAVES = ("theta", "phi", "rho", "z_s", "z_t")
# test_eval_c5's bound (tests/test_gpu_pose_data.py): 2e-3 of the reference's largest magnitude, the three
# pose scalars with a floor of 1e-2 on that magnitude
RTOL, ANGLE_FLOOR = 2e-3, 1e-2

# (samples, loss) -> calls of (ops.field_backward_x3_multi, ops.field_backward_x3, autograd._pair_flush with
# a field waiting).  autograd runs the fine field's backward first.  16 + 16: both fields pair; one alone
# waits and is run by whatever reads its sums.  32 + 24: the fine field (56 samples) cannot pair and runs
# alone, the coarse one waits alone.  24 + 40: the fine field (64) waits, the coarse one (24) cannot pair
# and flushes it before running itself.
EXPECTED_CALLS = {
    ((16, 16), "both"): (1, 0, 0), ((16, 16), "fine"): (0, 1, 1), ((16, 16), "coarse"): (0, 1, 1),
    ((32, 24), "both"): (0, 2, 1), ((32, 24), "fine"): (0, 1, 0), ((32, 24), "coarse"): (0, 1, 1),
    ((24, 40), "both"): (0, 2, 1), ((24, 40), "fine"): (0, 1, 1), ((24, 40), "coarse"): (0, 1, 0),
}


def intrinsics():
    from codenerf import synthetic
    return synthetic.srn_intrinsics(SIZE, focal=131.25 * SIZE / 128)


def eval_inputs(nc: int, nf: int):
    """CPU float32 inputs of one eval case."""
    from codenerf import synthetic
    return {
        "theta": torch.tensor([0.6]), "phi": torch.tensor([0.4]), "rho": torch.tensor([1.3]),
        "z_s": synthetic.latent_codes(5, 1), "z_t": synthetic.latent_codes(6, 1),
        "sel": torch.randperm(SIZE * SIZE, generator=torch.Generator().manual_seed(3))[:N_RAYS].reshape(1, -1),
        "t_rand": synthetic.uniforms01(21, 1, (N_RAYS, nc)), "u": synthetic.uniforms01(21, 2, (N_RAYS, nf)),
        "target": synthetic.uniforms01(21, 3, (SIZE * SIZE, 4)),
    }


def eval_reference(inp, nc: int, nf: int, loss: str, dtype, z_fine=None):
    """The oracle's eval step in ``dtype`` -> (loss, {leaf: gradient}, fine depths).  ``z_fine``: fine
    depths to use (a kernel's, or another run's) instead of this run's own sample_pdf."""
    import oracle.codenerf_oracle as o
    from codenerf import synthetic
    lv = {k: inp[k].to(dtype).clone().requires_grad_(True) for k in LEAVES}
    th, ph, rh = (lv[k][0] for k in ("theta", "phi", "rho"))
    st, ct, sp, cp = torch.sin(th), torch.cos(th), torch.sin(ph), torch.cos(ph)
    zero, one = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    c2w = torch.stack([torch.stack([-sp, -st * cp, ct * cp, rh * ct * cp]),
                       torch.stack([cp, -st * sp, ct * sp, rh * ct * sp]),
                       torch.stack([zero, ct, st, rh * st]),
                       torch.stack([zero, zero, zero, one])])
    ro, rd = o.ray_bundle(o.ray_directions(SIZE, SIZE, intrinsics().to(dtype)), c2w[None])
    ro, rd = o.gather_rays(ro, rd, inp["sel"])
    pc = {k: v.to(dtype) for k, v in synthetic.codenerf_params(0).items()}
    pf = {k: v.to(dtype) for k, v in synthetic.codenerf_params(1).items()}
    smp, ecfg = o.Sampling(nc, nf, NEAR, FAR), o.EmbedCfg()
    zs, zt = lv["z_s"].expand(N_RAYS, -1), lv["z_t"].expand(N_RAYS, -1)
    t_rand, u, tgt = inp["t_rand"].to(dtype), inp["u"].to(dtype), inp["target"][inp["sel"][0]].to(dtype)
    pts_c, z_c = o.sample_uniform(ro, rd, smp.bins, t_rand)
    z_c = z_c.to(dtype)
    rgb_c, _, _, w_c, _ = o.volume_render(o.forward_pass(pc, ecfg, rd, pts_c, zs, zt), z_c, rd)
    if z_fine is None:
        z_fine = o.sample_pdf(ro.detach(), rd.detach(), w_c.detach()[..., 1:-1], z_c, nf, u)[1]
    z_f = z_fine.detach().to(dtype)
    pts_f = ro[..., None, :] + rd[..., None, :] * z_f[..., :, None]
    rgb_f = o.volume_render(o.forward_pass(pf, ecfg, rd, pts_f, zs, zt), z_f, rd)[0]
    mse = torch.nn.functional.mse_loss
    total = LAM * (torch.norm(zs, p=2) + torch.norm(zt, p=2))
    if loss in ("both", "coarse"):
        total = total + mse(rgb_c[..., :3], tgt[..., :3])
    if loss in ("both", "fine"):
        total = total + mse(rgb_f[..., :3], tgt[..., :3])
    total.backward()
    return total.item(), {k: v.grad.detach().clone() for k, v in lv.items()}, z_f.detach()


def relative_errors(got, ref):
    """{leaf: max |got - ref| / scale}; scale: the reference's largest magnitude (pose scalars: at least
    ANGLE_FLOOR)."""
    out = {}
    for k in LEAVES:
        r = ref[k].double().cpu()
        scale = r.abs().max().item()
        if k in ("theta", "phi", "rho"):
            scale = max(ANGLE_FLOOR, scale)
        out[k] = (got[k].double().cpu().reshape(r.shape) - r).abs().max().item() / scale
    return out
