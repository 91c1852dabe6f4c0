"""Buffer contracts of the kernels (tests/buffers.py): no result depends on what an allocation held, and
no kernel stores past the end of a buffer.

Every case is an existing runner of the suite -- the integer-exact probes of test_gpu_field_exact.py /
test_gpu_field_fold.py, the leaf cases of test_gpu_leaf_edges.py / test_gpu_parity.py and the backward and
step tests of test_gpu_grad.py / test_gpu_train.py -- called through its module (an alias is not collected
twice) at sizes its own case module states, once under ``contracts("zero")`` and once under
``contracts("poison")``.  The runner builds its inputs with the real ``torch``; every buffer the package
allocates for the library comes from the stand-in.  Per case:

  * both runs satisfy the runner's own reference assertions, unchanged (they run inside the context);
  * on leaving each context every trailing guard holds its canary;
  * ``n_allocations > 0`` in both runs;
  * what every ``codenerf.ops`` call returned, and every caller-owned buffer it accumulated into, is bitwise
    equal between the two runs (NaNs included: a NaN the zero run lacks is a difference), except for the
    entries of EXCEPTIONS below.

No numeric bound is introduced here: each entry of EXCEPTIONS cites the test it borrows its bound from."""
import numpy as np
import pytest
import torch

import buffers as B
import exact_cases as X
import leaf_cases as L
import test_gpu_field_exact as E
import test_gpu_field_fold as FF
import test_gpu_grad as G
import test_gpu_isosurface as ISO
import test_gpu_leaf_edges as LE
import test_gpu_occupancy as OCC
import test_gpu_parity as P
import test_gpu_pose_data as PD
import test_gpu_train as T
import test_gpu_weight_cull as WC
from test_gpu_grad import GEMM_TOL, close, dev  # noqa: F401

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- the only non-bitwise comparisons
#
# The float-atomic paths: two runs add in no fixed order, so "equal between the fills" is the bound the
# existing test of that path states for two orders of the same sum (relative to the largest magnitude,
# test_gpu_grad.close's measure).  key -> (bound, the test it is borrowed from).  A bound of None: the two
# fills' results are not compared with each other; both runs are held to the named test's own reference.
EXCEPTIONS = {
    # ops.field_backward_x3(deterministic=False): every output of the float-atomic eval backward
    "x3_atomic": (1e-5, "test_gpu_grad.py::test_fused_backward_deterministic"),
    # g_code and the three code biases (b_xyz2, b_out, b_rgb) of the training backward with n_codes > 1
    "train_codes_f32": (1e-5, "test_gpu_grad.py::test_field_backward_train_nogeo_bitwise"),
    "train_codes_bf16x3": (2.6e-5, "test_gpu_grad.py::test_field_backward_train_nogeo_bitwise"),
    # d ro / d rd of the training backward: "the fused dX chain of cn_field_backward_fused" (codenerf.h), whose
    # ray sums are float atomics; that test compares this chain's atomic form with the form without atomics
    "train_rays_atomic": (1e-5, "test_gpu_grad.py::test_fused_backward_deterministic"),
    # ops.gemm_tn(deterministic=False): the float-atomic flush; each run against the float64 product at GEMM_TOL
    "gemm_tn_atomic": (None, "test_gpu_grad.py::test_gemm_tn_accumulates"),
    # the eval step: its float-atomic ray gradients feed every later stage, so the golden bounds hold under
    # both fills and nothing is compared between them
    "eval_step": (None, "test_gpu_grad.py::test_eval_step_gradients_golden"),
    # the scatter-add of gather_rays_backward with repeated indices
    "gather_repeated": (1e-6, "test_gpu_leaf_edges.py::test_gather_rays_backward_repeated_indices"),
}
BOUNDS = {key: bound for key, (bound, _) in EXCEPTIONS.items()}
CODE_BIAS_GRADS = ("3", "5", "17")    # b_xyz2, b_out, b_rgb in param_list order (test_field_backward_train_nogeo_bitwise)


def exception_for(name, label, kwargs, allowed):
    """The EXCEPTIONS key that covers the output ``label`` (buffers._tensors: the path of dict keys and positions,
    "0.d_ro", "0.param_grads.3") of the logged call ``name``, if the case allows it."""
    leaf = label.split(".")
    if "gemm_tn_atomic" in allowed and name == "gemm_tn" and not kwargs.get("deterministic", False):
        return "gemm_tn_atomic"
    if "train_rays_atomic" in allowed and name in ("field_backward_train", "field_backward_train_multi") and \
            leaf[-1] in ("d_ro", "d_rd"):
        return "train_rays_atomic"
    if "x3_atomic" in allowed and name == "field_backward_x3" and kwargs.get("deterministic") is False:
        return "x3_atomic"
    for key in ("train_codes_f32", "train_codes_bf16x3"):
        if key in allowed and name.startswith("field_backward_train"):
            if leaf[-1] == "g_code" or (len(leaf) >= 2 and leaf[-2] == "param_grads" and leaf[-1] in CODE_BIAS_GRADS):
                return key
    if "gather_repeated" in allowed and name == "gather_rays_backward":
        return "gather_repeated"
    return None


# ---------------------------------------------------------------- what of a logged return is an output
#
# Returned tensors whose contents the header leaves partly open: only the documented part is compared.
#
# What this cannot see.  The scratch row behind the save buffer is compared nowhere (unspecified by the
# header).  The mask words are compared decoded, rows < M only (the bits past M are open).  The integer
# poison is the value 1, as the harness's rule asks, so a poisoned mask word differs from a zeroed one in
# bit 0 alone: a backward that read a mask word nobody wrote would mostly go unseen here; the masks are
# covered by the forwards' own comparison of every decoded decision with the reference.


def outputs_of(name, pairs, kwargs):
    if name in ("radiance_field_train_w16", "radiance_field_masks") and len(pairs) >= 2:
        raw, masks = pairs[0][1], pairs[-1][1]
        m = raw.numel() // 4
        if m == 0:
            return pairs[:-1]
        x3 = kwargs.get("precision", "f32") == "bf16x3"
        decoded = (G.decode_relu_masks if x3 else G.decode_relu_masks_w16)(masks, m)
        out = list(pairs[:-1]) + [("masks." + k, decoded[k]) for k in sorted(decoded)]
        if name == "radiance_field_train_w16" and not x3:
            # the fp32 forward's (M, 64) encoding plane, behind the five planes in saved's own storage
            # (ops.radiance_field_train_w16; codenerf.h), padding slot included
            saved = pairs[1][1]
            plane = torch.empty(0, dtype=torch.float32, device=saved.device).set_(
                saved.untyped_storage(), 5 * m * 256, (m, 64), (64, 1))
            out.append(("encoding_plane", plane))
        return out
    if name in ("occupancy_cull", "weight_cull"):
        # sample_index, pts, vdir (, code_out); then the state's workspace, which goes to occupancy_expand
        return pairs[:4 if kwargs.get("want_code", True) else 3]
    if name in ("code_ds_outer", "code_ds_outer_multi"):
        return []                     # they return their workspace (rows 3..5 of each code written, the rest open)
    return pairs


def compare_fills(zero, poison, allowed):
    return B.compare_fills(zero, poison, outputs_of, lambda name, label, kw: exception_for(name, label, kw, allowed),
                           BOUNDS, close)


def fresh_caches():
    """Nothing made under one context is handed to the next: the packs cached by test_gpu_field_exact."""
    for k in [k for k in E._DEV if k[0] == "pack"]:
        del E._DEV[k]


def both_fills(run, allowed=()):
    logs = {}
    for fill in B.FILLS:
        fresh_caches()
        with B.contracts(fill) as arena:
            run(arena)
        assert arena.n_allocations > 0, f"{fill}: no allocation went through the stand-in"
        logs[fill] = arena.returns
    fresh_caches()
    assert logs["zero"], "no codenerf.ops call was logged"
    if "eval_step" not in allowed:
        compare_fills(logs["zero"], logs["poison"], set(allowed))


# ---------------------------------------------------------------- the cases


def case_list():
    """(id, runner(dev, arena), allowed exceptions)"""
    out = []

    def add(name, fn, *args, allowed=()):
        out.append(pytest.param(lambda dev, arena: fn(dev, *args), tuple(allowed), id=name))

    # -- field kernels, from exact_cases
    enc = [c for c in X.encoded_forward_cases() if c["m"] in (1, 127, 129, 257)]
    for c in enc:
        for fmt in E.FORWARD_FORMATS:
            add(f"encoded-{E.ident(c)}-{fmt}", run_encoded, c, fmt)
        add(f"encoded-{E.ident(c)}-{FF.FOLD}", FF.run_exact, c)
    for c in X.geometry_forward_cases():
        if (c["r"], c["s"], c["chunk"]) in ((1, 1, 1), (7, 5, 3), (37, 8, 10), (3, 64, 2)):
            for fmt in E.FORWARD_FORMATS + ("density",):
                add(f"geometry-{E.ident(c)}-{fmt}", E.test_geometry_forward, c, fmt)
            add(f"geometry-{E.ident(c)}-{FF.FOLD}", FF.run_exact, c)
    add("train-forward-encoded", E.test_encoded_forward_train)
    for c in X.train_forward_cases()[1:]:
        for precision in ("f32", "bf16x3", "f32_v1"):
            add(f"train-forward-{E.ident(c)}-{precision}", E.test_geometry_forward_train, c, precision)
    for c in X.fused_backward_cases():
        for precision in ("f32", "bf16x3"):
            for det in (True, False):
                add(f"fused-eval-{E.ident(c)}-{precision}-{'det' if det else 'atomic'}", E.test_fused_backward_eval,
                    c, precision, det, allowed=("x3_atomic",))
            add(f"fused-train-{E.ident(c)}-{precision}", E.test_fused_backward_train, c, precision)
    for c in X.unfused_backward_cases():
        for precision in ("f32", "bf16x3"):
            add(f"unfused-{E.ident(c)}-{precision}", E.test_unfused_backward_encoded, c, precision)
        for single in (False, True):
            add(f"code-backward-{E.ident(c)}-{'single' if single else 'ws'}", E.test_code_backward, c, single)
    for m, layout in ((1, "one"), (129, "per_row")):
        add(f"density-encoded-{m}", E.test_density_encoded_rows, m, layout)
    for fmt in E.FORWARD_FORMATS:
        add(f"persistent-{fmt}", E.test_encoded_forward_second_tile_of_every_workgroup, fmt)
    add(f"persistent-{FF.FOLD}", FF.test_fold_exact_second_tile_of_every_workgroup)

    # -- the deterministic eval backward's idle waves and partial tiles (test_fused_backward_deterministic's
    #    inputs: two deterministic runs bitwise, deterministic vs atomic at its 1e-5, ray_into = base + result)
    for precision, mode, r, s in (("f32", "rayz", 5, 16), ("bf16x3", "rayz", 5, 32), ("f32", "pts", 37, 32),
                                  ("bf16x3", "pts", 37, 32)):
        add(f"eval-det-{precision}-{mode}-{r}x{s}", G.test_fused_backward_deterministic, precision, mode, r, s, r,
            allowed=("x3_atomic",))

    # -- the training backward's dW plans
    for precision, r, s, n_codes in (("f32", 5, 16, 1), ("f32", 300, 24, 1), ("f32", 1024, 64, 3),
                                     ("bf16x3", 1024, 64, 3)):
        add(f"train-dw-{precision}-{r}x{s}-codes{n_codes}", G.test_field_backward_train_nogeo_bitwise, precision,
            "rayz", r, s, n_codes,
            allowed=("train_rays_atomic",) + (("train_codes_" + precision,) if n_codes > 1 else ()))
    add("train-dw-batched-dirs-1056x64", G.test_field_backward_train_dir1_fold, "rayz", 1056, 64, 256)

    # -- paired entries: pair vs single bitwise (the runners' own assertion) under both fills
    add("pair-eval-300x16+32", G.test_fused_backward_pair_bitwise, 300, 16, 32)
    add("pair-train-512x64+128", T.test_field_backward_train_pair_bitwise, 512, 64, 128)

    # -- GEMMs through ops
    for m, n, k in ((129, 3, 27), (300, 63, 3), (1000, 257, 283)):
        for precision in ("f32", "bf16x3"):
            add(f"gemm-nn-{m}x{n}x{k}-{precision}", G.test_gemm_nn_masked, m, n, k, precision)
            for det in (False, True):
                add(f"gemm-tn-{m}x{n}x{k}-{precision}-{'det' if det else 'atomic'}", run_gemm_tn, m, n, k, precision,
                    det, allowed=() if det else ("gemm_tn_atomic",))

    # -- leaf kernels, one case per dispatch form
    for s in (1, 7, 65, 129):
        add(f"volume-forward-{s}", LE.test_volume_forward_regimes, "opaque", 21, s)
        add(f"volume-backward-{s}", LE.test_volume_backward_regimes, "opaque", 21, s)
    for s in (1, 7, 65, 129):
        out.append(pytest.param(lambda dev, arena, s=s: run_volume_rd_variants(dev, arena, s), (),
                                id=f"volume-backward-accumulate-rd-{s}"))
    for nc in (6, 8):
        add(f"sample-uniform-{nc}", run_sample_uniform, nc)
    for n, nc, nf in ((37, 3, 5), (130, 13, 7), (33, 256, 256)):
        add(f"sample-pdf-{n}x{nc}x{nf}", P.test_sample_pdf_scan_and_sort_bitwise, n, nc, nf)
    for config in [c[0] for c in L.POSENC_CONFIGS]:
        for m in L.POSENC_ROWS:
            add(f"posenc-{config}-{m}", LE.test_posenc_configurations, config, m)
    for h, w in L.BUNDLE_SHAPES[:2]:
        add(f"ray-bundle-backward-{h}x{w}", LE.test_ray_bundle_backward_sizes, h, w, "both")
    for r, s in L.POINTS_SHAPES[:2]:
        add(f"ray-points-backward-{r}x{s}", LE.test_ray_points_backward_sizes, r, s, "both")
    add("pose-rays-forward", PD.test_pose_rays_spherical_forward_and_grads)
    for kind in (1, 2049):
        for path in ("angles", "c2w"):
            add(f"pose-rays-forward-{path}-{kind}", run_pose_rays_forward, path, kind)
            add(f"pose-rays-backward-{path}-{kind}", LE.test_pose_rays_backward_rounds, path, kind)
    add("gather-rays-backward-unique", LE.test_gather_rays_backward_unique_is_index_add_bitwise)
    add("gather-rays-backward-repeated", LE.test_gather_rays_backward_repeated_indices, allowed=("gather_repeated",))
    add("random-select", PD.test_random_select_device)
    for n_rays in L.LOSS_RAYS:
        add(f"render-loss-rays-{n_rays}", LE.test_loss_rounds_strides_and_null_inputs, n_rays, 3, "both")
    for codes in L.LOSS_CODES:
        add(f"render-loss-codes-{codes[0]}", LE.test_loss_code_sizes, codes, 1)
    for codes in ((1, 256), (9, 256)):
        add(f"render-loss-backward-dz-{codes[0]}", LE.test_loss_backward_accumulates_dz, codes)
    add("occupancy-build", OCC.test_build_matches_oracle, 32, 1)
    for r, s in ((1, 1), (37, 64)):
        add(f"occupancy-cull-{r}x{s}", OCC.test_cull_matches_oracle, r, s, "sphere")
        add(f"occupancy-expand-{r}x{s}", OCC.test_expand, r, s, "sphere")
        add(f"weight-cull-{r}x{s}", WC.test_weight_cull_matches_model, r, s)
    for n_slots, n_rows in ((1, 1), (7, 3)):
        out.append(pytest.param(lambda dev, arena, a=(n_slots, n_rows): run_scatter_rgb(dev, arena, *a), (),
                                id=f"scatter-rgb-{n_slots}x{n_rows}"))
    add("isosurface-33", ISO.test_crosses_workgroups)

    # -- two whole steps through the public API
    for precision in ("f32", "bf16x3"):
        add(f"train-step-{precision}", T.test_train_minibatch_deterministic, precision)
    add("eval-step", G.test_eval_step_gradients_golden, allowed=("eval_step",))
    return out


def run_encoded(dev, case, fmt):
    """test_encoded_forward_sizes_and_code_layouts' body on any encoded case (the model set's too)."""
    from codenerf import ops
    d, ref = E.on_dev(dev, case), X.reference(case)
    cb = E.code_bias(dev, case)
    E.same(cb, ref["code_bias"], "code_bias")
    raw = ops.mlp_forward(E.packed(dev, case, fmt), cb, d["x"], d["code_index"], precision=fmt)
    E.same(raw, ref["raw"], "raw")


def run_gemm_tn(dev, m, n, k, precision, det):
    """test_gemm_tn_accumulates (C given: a random base), and C left to ops."""
    from codenerf import ops
    G.test_gemm_tn_accumulates(dev, m, n, k, precision, det)
    # C not given: ops allocates it (zeroed, guarded)
    g = torch.Generator().manual_seed(m + n + k)
    a, b = torch.randn(m, n, generator=g), torch.randn(m, k, generator=g)
    c = ops.gemm_tn(a.to(dev), b.to(dev), None, precision=precision, deterministic=det)
    close(c, a.double().t() @ b.double(), GEMM_TOL[precision], "gemm_tn into zeros " + precision)


def run_scatter_rgb(dev, arena, n_slots, n_rows):
    """test_gpu_weight_cull.test_scatter_rgb with ``raw`` in an arena buffer of exactly n_slots rows."""
    from codenerf import ops
    g = torch.Generator().manual_seed(n_slots)
    idx = torch.randperm(n_slots, generator=g)[:n_rows].sort().values.to(torch.int32)
    compact = torch.randn(n_rows, 4, generator=g)
    compact[::5, 1] = float("nan")
    raw = arena.empty((n_slots, 4), torch.float32, dev)
    raw.view(torch.int32).fill_(WC.SENTINEL)
    expect = raw.view(torch.int32).clone()
    expect[idx.long().to(dev), :3] = compact.to(dev).view(torch.int32)[:, :3]
    out = ops.scatter_rgb(compact.to(dev), idx.to(dev), raw)
    assert out is raw
    assert torch.equal(raw.view(torch.int32), expect)


def run_volume_rd_variants(dev, arena, s):
    """test_volume_backward_rd_variants' body at any s, with d_rd_into in an arena buffer of exactly (R, 3):
    want_rd=False leaves d raw unchanged; accumulate_rd = 1 ends as pre-fill + the plain d rd, bit for bit."""
    from codenerf import ops
    r, regime = 21, "opaque"
    c = L.volume_case(regime, r, s)
    raw, z, rd = c["raw"].to(dev), c["z"].to(dev), c["rd"].to(dev)
    up = {k: v.to(dev) for k, v in L.volume_upstream(regime, r, s, L.VOLUME_TERMS).items()}
    d_raw, d_rd = ops.volume_render_backward(raw, z, rd, **up)
    n_raw, n_rd = ops.volume_render_backward(raw, z, rd, want_rd=False, **up)
    assert n_rd is None and LE.bits_equal(n_raw, d_raw)
    fill = torch.randn(r, 3, generator=torch.Generator().manual_seed(s)).to(dev)
    into = arena.empty((r, 3), torch.float32, dev).copy_(fill)
    a_raw, a_rd = ops.volume_render_backward(raw, z, rd, d_rd_into=into, **up)
    assert a_rd.data_ptr() == into.data_ptr() and LE.bits_equal(a_raw, d_raw)
    assert LE.bits_equal(a_rd, fill + d_rd)


def run_pose_rays_forward(dev, path, kind):
    """cn_pose_rays at leaf_cases.pose_case(kind) (one ray per image; 2049: a ragged second round), from the
    angles or from c2w, with target rows: ro / rd bit for bit the rays of ray_bundle + gather_rays on the pose
    (the one it returns, or the c2w given) (test_sample_c2w_equals_bundle_then_gather's identity), the target rows exact, and from the
    angles the pose and the rays against the oracle at test_pose_rays_spherical_forward_and_grads' 1e-6."""
    from codenerf import ops
    from oracle import codenerf_oracle as O
    c = L.pose_case(kind)
    sel = c["sel"]
    dirs = LE._dirs(dev)
    target = torch.rand(L.RAY_B, L.RAY_HW, 4, generator=torch.Generator().manual_seed(3))
    if path == "angles":
        th, ph, rh = (a.to(dev) for a in c["angles"])
        ro, rd, pose, tp = ops.pose_rays(dirs, th, ph, rh, select_inds=sel.to(dev), target=target.to(dev))
        want_pose = torch.stack([O.pose_spherical(*(a[b:b + 1] for a in c["angles"])) for b in range(L.RAY_B)])
        assert (pose.cpu() - want_pose).abs().max().item() <= 1e-6
        ro_o, rd_o = O.gather_rays(*O.ray_bundle(L.ray_dirs(), want_pose), sel.numpy())
        assert (ro.cpu() - ro_o).abs().max().item() <= 1e-6 and (rd.cpu() - rd_o).abs().max().item() <= 1e-6
    else:
        pose = c["c2w"].to(dev)
        ro, rd, _, tp = ops.pose_rays(dirs, c2w=pose, select_inds=sel.to(dev), target=target.to(dev))
    ro_b, rd_b = ops.ray_bundle(dirs, pose)
    o, d = ops.gather_rays(ro_b.reshape(L.RAY_B, -1, 3), rd_b.reshape(L.RAY_B, -1, 3), sel.to(dev))
    assert ro.shape == (L.RAY_B * kind, 3) and torch.equal(ro, o) and torch.equal(rd, d)
    assert torch.equal(tp.cpu(), torch.cat([target[b, sel[b]] for b in range(L.RAY_B)]))


def run_sample_uniform(dev, nc):
    """test_sample_uniform_shapes_vs_oracle's comparison at R = 37: both forms (nc % 4 == 0 and not), with and
    without the perturbed draw, bit for bit against the oracle."""
    from codenerf import ops
    from codenerf.nerf import PointSampler
    from oracle import codenerf_oracle as O
    g = torch.Generator().manual_seed(nc)
    R = 37
    ro, rd = torch.randn(R, 3, generator=g), torch.randn(R, 3, generator=g)
    for perturb in (False, True):
        ps = PointSampler(nc, 8, 0.8, 1.8, spacing_mode="lindepth", perturb=perturb, dtype=torch.float32, device=dev)
        t_rand = torch.rand(R, nc, generator=g) if perturb else None
        pts, z = ops.sample_uniform(ro.to(dev), rd.to(dev), ps.z_vals, ps.lower, ps.upper,
                                    None if t_rand is None else t_rand.to(dev))
        pts_o, z_o = O.sample_uniform(ro, rd, O.Sampling(nc, 8, 0.8, 1.8).bins, t_rand)
        assert torch.equal(z.cpu(), z_o) and torch.equal(pts.cpu(), pts_o)


@pytest.mark.parametrize("run,allowed", case_list())
def test_fills_agree_and_guards_hold(dev, run, allowed):
    both_fills(lambda arena: run(dev, arena), allowed)


def test_exceptions_cite_existing_tests():
    """Every entry of EXCEPTIONS names a test function that exists in the file it names."""
    import importlib
    for key, (bound, where) in EXCEPTIONS.items():
        module, name = where.split("::")
        assert callable(getattr(importlib.import_module(module[:-3]), name)), key
        assert bound is None or 0 < bound <= 2.6e-5


def test_harness_on_the_device(dev):
    """The stand-in is what ``codenerf.ops`` allocates from, on the device: poisoned interiors (NaN, the value
    1), offset 0, 256-byte aligned, and a store one element past a view (a torch copy inside the flat
    allocation, so nothing faults) trips the guard with the allocation's call site inside the package."""
    from codenerf import ops
    nodes = torch.zeros(33, 33, 33, device=dev)
    for fill in B.FILLS:
        with B.contracts(fill) as arena:
            assert ops.torch is not torch and torch.empty is not ops.torch.empty
            own = [arena.empty((5, 3), dt, dev) for dt in (torch.float32, torch.int32, torch.int64)]
            bits_ = ops.occupancy_build(nodes, 0.5, 0)           # (32^3 / 32,) words, all written: nothing occupied
        assert ops.torch is torch
        assert arena.n_allocations == 4 and not bool(bits_.any())
        for t in own + [bits_]:
            assert t.is_cuda and t.storage_offset() == 0 and t.data_ptr() % 256 == 0
        if fill == "poison":
            assert bool(torch.isnan(own[0]).all()) and bool((own[1] == 1).all()) and bool((own[2] == 1).all())
        else:
            assert not any(bool(t.any()) for t in own)
    with pytest.raises(B.GuardError) as info:
        with B.contracts("poison"):
            bits_ = ops.occupancy_build(nodes, 0.5, 0)
            bits_.as_strided((bits_.numel() + 1,), (1,))[-1] = 7
    assert "ops.py:" in str(info.value) and f"first at byte {4 * bits_.numel()} " in str(info.value)


@pytest.mark.parametrize("stage", ["train", "val"])
def test_srn_unpack(dev, tmp_path, stage):
    def run(arena):
        tree = tmp_path / arena.fill
        tree.mkdir()
        PD.test_srn_resident_batches(dev, tree, stage)
    both_fills(run)


# ---------------------------------------------------------------- caller-owned buffers from the arena


@pytest.mark.parametrize("device_scalars", [False, True])
def test_adamw_state_from_the_arena(dev, device_scalars):
    """ops.adamw_step / adamw_step_dev on leaf_cases.adam_flat_case() with param, grad, exp_avg and exp_avg_sq
    in arena buffers of exactly n floats: a store past the last segment lands in a guard.  Values as
    test_adamw_flat_segments_two_launches asserts them (torch's fp32 AdamW at ADAM_RTOL, elements outside the
    segments kept bit for bit); the two fills agree bit for bit."""
    from codenerf import ops
    n, segs = L.adam_flat_case()
    g = torch.Generator().manual_seed(7)
    p0, gr = torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g) * 1e-2
    m0, v0 = torch.randn(n, generator=g) * 1e-2, torch.rand(n, generator=g) * 1e-4
    b1, b2 = L.ADAM_BETAS
    inside = torch.zeros(n, dtype=torch.bool)
    for b, e, *_ in segs:
        inside[b:e] = True
    ref = L.adam_flat_reference(p0, gr, m0, v0, segs, torch.float32)
    got = {}
    for fill in B.FILLS:
        with B.contracts(fill) as arena:
            p, gd, m, v = (arena.empty((n,), torch.float32, dev).copy_(t) for t in (p0, gr, m0, v0))
            if device_scalars:
                host = np.zeros(3 * len(segs), dtype=np.float32)
                ops.adamw_scalars(segs, b1, b2, host)
                scalars = arena.empty((host.size,), torch.float32, dev).copy_(torch.from_numpy(host))
                ops.adamw_step_dev(p, gd, m, v, segs, scalars, b1, b2, L.ADAM_EPS)
            else:
                ops.adamw_step(p, gd, m, v, segs, b1, b2, L.ADAM_EPS)
        assert arena.n_allocations > 0
        got[fill] = [t.cpu() for t in (p, m, v)]
        for t, was, want, what in zip(got[fill], (p0, m0, v0), ref, ("param", "exp_avg", "exp_avg_sq")):
            assert LE.bits_equal(t[~inside], was[~inside]), what
            LE.rel_margin(f"buffers_adamw[{fill}]", what, t[inside], want[inside], LE.ADAM_RTOL)
        assert torch.equal(gd.cpu(), gr)
    for a, b in zip(got["zero"], got["poison"]):
        assert LE.bits_equal(a, b)


def _based(arena, dev, shape, seed):
    """(an arena buffer holding a finite random base, the base)."""
    base = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)
    return arena.empty(shape, torch.float32, dev).copy_(base), base


def _train_backward_inputs(dev, r, s, chunk, precision):
    """test_field_backward_train_nogeo_bitwise's inputs (rays + depths, one code row)."""
    from codenerf import ops, synthetic
    params = [p.detach() for p in G.model(dev, 0).param_list()]
    g = torch.Generator().manual_seed(r + s + 1)
    ro = (torch.randn(r, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 1.3])).to(dev)
    rd = torch.randn(r, 3, generator=g).to(dev)
    z = torch.sort(0.8 + torch.rand(r, s, generator=g), dim=-1).values.to(dev)
    gout = torch.randn(r, s, 4, generator=g).to(dev)
    zs, zt = synthetic.latent_codes(5, 1).to(dev), synthetic.latent_codes(6, 1).to(dev)
    x3 = precision == "bf16x3"
    cb = ops.code_bias(params, zs, zt)
    _, saved, masks = ops.radiance_field_train_w16(ops.mlp_pack(params, "bf16x3" if x3 else "f32_w16"), cb, rd, s,
                                                   chunk, E.FX, E.FD, precision=precision, ro=ro, z=z)
    return dict(packed_t=ops.mlp_pack(params, "bf16x3_t" if x3 else "f32_w16_t"), params=params, masks=masks,
                saved=saved, x_enc=None, d_raw=gout, n_rays=r, n_samples=s, chunk_rows=chunk, n_codes=1,
                freqs_xyz=E.FX, freqs_dir=E.FD, rd=rd, ro=ro, z=z, precision=precision)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_accumulated_buffers_from_the_arena(dev, precision):
    """Caller-owned ACCUMULATED buffers in arena buffers of their exact size, pre-filled with a finite random
    base, on the deterministic paths: they come back as base + the zero-base result, bit for bit, under both
    fills -- C of the deterministic gemm_tn, ray_into of the eval backward without atomics (M = 80 / 160: a
    last tile with idle waves), dz_into of the two-launch code backward, d_rd_into of the volume render's
    backward, and param_grads of the training backward at (300, 32) (M = 9600: 75 tiles; g_code zeroed, as the header asks)."""
    from codenerf import ops, synthetic
    x3 = precision == "bf16x3"
    g = torch.Generator().manual_seed(11)
    m, n, k = 300, 63, 3
    a, b = torch.randn(m, n, generator=g).to(dev), torch.randn(m, k, generator=g).to(dev)
    r, s = 5, 32 if x3 else 16
    params = [p.detach() for p in G.model(dev, 0).param_list()]
    ro = (torch.randn(r, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 1.3])).to(dev)
    rd = torch.randn(r, 3, generator=g).to(dev)
    z = torch.sort(0.8 + torch.rand(r, s, generator=g), dim=-1).values.to(dev)
    gout = torch.randn(r, s, 4, generator=g).to(dev)
    zs, zt = synthetic.latent_codes(5, 1).to(dev), synthetic.latent_codes(6, 1).to(dev)
    gc = (torch.randn(3, ops.code_bias(params, zs, zt).shape[1], generator=g) * 1e-2).to(dev)
    zs3, zt3 = synthetic.latent_codes(5, 3).to(dev), synthetic.latent_codes(6, 3).to(dev)
    vc = L.volume_case("opaque", 21, 7)
    vup = {kk: v.to(dev) for kk, v in L.volume_upstream("opaque", 21, 7, L.VOLUME_TERMS).items()}
    train = _train_backward_inputs(dev, 300, 32, 256, precision)
    got = {}
    for fill in B.FILLS:
        with B.contracts(fill) as arena:
            out = {}
            # gemm_tn, deterministic
            c, base = _based(arena, dev, (n, k), 1)
            plain = ops.gemm_tn(a, b, None, precision=precision, deterministic=True)
            ops.gemm_tn(a, b, c, precision=precision, deterministic=True)
            out["gemm_tn"] = (c, base, plain)
            # the eval backward without atomics
            cb = ops.code_bias(params, zs, zt)
            _, masks = ops.radiance_field_masks(ops.mlp_pack(params, "bf16x3" if x3 else "f32_w16"), cb, rd, s, r,
                                                E.FX, E.FD, precision=precision, ro=ro, z=z)
            kw = dict(packed_t=ops.mlp_pack(params, "bf16x3_t" if x3 else "f32_w16_t"), masks=masks, d_raw=gout,
                      n_rays=r, n_samples=s, chunk_rows=r, n_codes=1, freqs_xyz=E.FX, freqs_dir=E.FD, rd=rd, ro=ro, z=z,
                      want_ro=True, want_rd=True, precision=precision, deterministic=True)
            plain = ops.field_backward_x3(**kw)
            (d_ro, base_ro), (d_rd, base_rd) = _based(arena, dev, (r, 3), 2), _based(arena, dev, (r, 3), 3)
            ops.field_backward_x3(ray_into=(d_ro, d_rd), **kw)
            out["d_ro"], out["d_rd"] = (d_ro, base_ro, plain["d_ro"]), (d_rd, base_rd, plain["d_rd"])
            # the two-launch code backward
            dz = ops.code_bias_backward(params, zs3, zt3, gc, None)
            (dzs, base_s), (dzt, base_t) = _based(arena, dev, (3, 256), 4), _based(arena, dev, (3, 256), 5)
            ops.code_bias_backward(params, zs3, zt3, gc, None, dz_into=(dzs, dzt))
            out["dz_s"], out["dz_t"] = (dzs, base_s, dz[0]), (dzt, base_t, dz[1])
            # the volume render's backward
            _, v_rd = ops.volume_render_backward(vc["raw"].to(dev), vc["z"].to(dev), vc["rd"].to(dev), **vup)
            into, base = _based(arena, dev, (21, 3), 6)
            ops.volume_render_backward(vc["raw"].to(dev), vc["z"].to(dev), vc["rd"].to(dev), d_rd_into=into, **vup)
            out["volume d_rd"] = (into, base, v_rd)
            # the training backward: every parameter gradient and g_code
            zero_pg = [arena.empty(tuple(p.shape), torch.float32, dev).zero_() for p in params]
            zero_gc = arena.empty((1, gc.shape[1]), torch.float32, dev).zero_()
            ops.field_backward_train_multi([dict(train, param_grads=zero_pg, g_code=zero_gc)], precision)
            based = [_based(arena, dev, tuple(p.shape), 20 + i) for i, p in enumerate(params)]
            # g_code is an accumulator the caller zeroes (codenerf.h): the code biases are its column sums
            gcb, gc_base = arena.empty((1, gc.shape[1]), torch.float32, dev).zero_(), torch.zeros_like(zero_gc)
            ops.field_backward_train_multi([dict(train, param_grads=[t for t, _ in based], g_code=gcb)], precision)
            for i, ((t, base), zpg) in enumerate(zip(based, zero_pg)):
                out[f"param grad {i}"] = (t, base, zpg)
            out["train g_code"] = (gcb, gc_base, zero_gc)
        assert arena.n_allocations > 0
        for what, (t, base, plain) in out.items():
            assert bool(torch.isfinite(t).all()), (fill, what)
            assert torch.equal(t, base + plain), f"{fill}: {what} is not base + the zero-base result"
        got[fill] = {what: t for what, (t, _, _) in out.items()}
    for what in got["zero"]:
        assert torch.equal(got["zero"][what], got["poison"][what]), f"{what} differs between the fills"


# ---------------------------------------------------------------- strided outputs through the C ABI

GAP = -12345.0                         # what the gap columns of C (and of the mask) hold


def _strided(arena, dev, rows, cols, ld, payload):
    buf = arena.empty((rows, ld), torch.float32, dev)
    buf.fill_(GAP)
    buf[:, :cols] = payload.to(dev)
    return buf


def _gaps_untouched(buf, cols, what):
    gap = buf[:, cols:]
    assert torch.equal(gap, torch.full_like(gap, GAP)), f"{what}: a gap column of the strided output was written"


@pytest.mark.parametrize("m,n,k", [(129, 63, 27), (300, 257, 283)])
def test_strided_outputs_leave_the_gaps_alone(dev, m, n, k):
    """cn_gemm_nn / cn_gemm_nn_x3 with ldc = N + 3 and ldm = N + 5, cn_gemm_tn / cn_gemm_tn_x3 / cn_gemm_tn_ws
    with ldc = K + 3 (the layer-wise backward's rows of 260 are this form): the gap columns and the trailing
    guard stay as they were, the payload is the float64 product at GEMM_TOL."""
    from codenerf import _lib, ops
    lib = ops._lib_ready()
    g = torch.Generator().manual_seed(m + n + k)
    a, b = torch.randn(m, k, generator=g), torch.randn(k, n, generator=g)
    mask = torch.randn(m, n, generator=g)
    at, bt, c0 = torch.randn(m, n, generator=g), torch.randn(m, k, generator=g), torch.randn(n, k, generator=g)
    ref_nn = (a.double() @ b.double()) * (mask > 0)
    ref_tn = c0.double() + at.double().t() @ bt.double()
    ad, bd, atd, btd = a.to(dev), b.to(dev), at.to(dev), bt.to(dev)
    st = ops.stream_of(ad)
    for fill in B.FILLS:
        with B.contracts(fill) as arena:
            maskd = _strided(arena, dev, m, n, n + 5, mask)
            for precision, fn in (("f32", lib.cn_gemm_nn), ("bf16x3", lib.cn_gemm_nn_x3)):
                c = arena.empty((m, n + 3), torch.float32, dev)
                c[:, n:] = GAP
                ops.check(fn(ops.ptr(ad), k, ops.ptr(bd), n, ops.ptr(c), n + 3, ops.ptr(maskd), n + 5, m, n, k, st),
                          "cn_gemm_nn " + precision)
                close(c[:, :n], ref_nn, GEMM_TOL[precision], "strided gemm_nn " + precision)
                _gaps_untouched(c, n, "gemm_nn " + precision)
            _gaps_untouched(maskd, n, "mask")
            for precision, fn in (("f32", lib.cn_gemm_tn), ("bf16x3", lib.cn_gemm_tn_x3)):
                c = _strided(arena, dev, n, k, k + 3, c0)
                ops.check(fn(ops.ptr(atd), n, ops.ptr(btd), k, ops.ptr(c), k + 3, m, n, k, st), "cn_gemm_tn " + precision)
                close(c[:, :k], ref_tn, GEMM_TOL[precision], "strided gemm_tn " + precision)
                _gaps_untouched(c, k, "gemm_tn " + precision)
            det = {}
            for precision in ("f32", "bf16x3"):
                c = _strided(arena, dev, n, k, k + 3, c0)
                ws = arena.empty((int(lib.cn_gemm_tn_workspace_floats(m, n, k)),), torch.float32, dev)
                ops.check(lib.cn_gemm_tn_ws(_lib.FORMATS[precision], ops.ptr(atd), n, ops.ptr(btd), k, ops.ptr(c), k + 3,
                                            m, n, k, ops.ptr(ws), st), "cn_gemm_tn_ws " + precision)
                close(c[:, :k], ref_tn, GEMM_TOL[precision], "strided gemm_tn_ws " + precision)
                _gaps_untouched(c, k, "gemm_tn_ws " + precision)
                det[precision] = c.clone()
        assert arena.n_allocations > 0
        if fill == "zero":
            first = det
        else:
            for precision in det:      # the deterministic form: the same bits whatever the workspace held
                assert torch.equal(first[precision], det[precision]), precision
