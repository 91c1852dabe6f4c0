"""Integer-exact probes of the field kernels: every comparison is torch.equal against the float64
reference of tests/exact_cases.py cast to fp32.

With the small-integer probe models and inputs every product and partial sum of the network is an
integer fp32 holds exactly in any summation order, and every 3xbf16 product is exact
(exact_cases.check_exact, proven on the reference alone by tests/test_exact_cases_cpu.py).  So the
fp32 MFMA kernels (mlp.hip, mlp_f32.hip), the 3xbf16 kernels (mlp_x3.hip, mlp_x3w.hip), the fused code
bias and the backwards (grad.hip) must all return the reference's bits: a wrong row, column, pad slot,
ray, code row or mask bit shows as an integer difference.  Code indices stay in range everywhere.

Geometry cases compare the gradients of layer_xyz1 / layer_dir1 on the raw-input columns only
(exact_cases.exact_columns): the sin / cos columns' gradients are sums of non-integers by construction of
the inputs, not through any route of a kernel.

The split models (exact_cases.SPLIT_MODELS) give one GEMM layer's weights a bf16 low part, in units of 2^-8:
on them the 3xbf16 kernels' third product, Wl.Xh, multiplies the packs' lo fragments (bf16x3, bf16x3_w16, the
transposed bf16x3_t) or the low parts the unfused backward's GEMMs split off themselves, and one lo element a
block, a lane half or a k-step off, two swapped, or a lo product read against Xl shows as a difference of
2^-8s (proven on the CPU: test_exact_cases_cpu).  The fp32 formats run on them as a cross-check."""
import pytest
import torch

import exact_cases as E
from test_gpu_grad import decode_relu_masks, decode_relu_masks_w16, dev  # noqa: F401

pytestmark = pytest.mark.gpu

FORWARD_FORMATS = ("f32", "f32_w16", "bf16x3", "bf16x3_w16")
FX = [float(2 ** k) for k in range(10)]
FD = [float(2 ** k) for k in range(4)]

_DEV = {}
# every case list a test below runs, then the split models' cases of the same kind
TRAIN_FORWARD_CASES = E.train_forward_cases()[1:] + E.split_geometry_cases()
GEOMETRY_FORWARD_CASES = E.geometry_forward_cases() + E.split_geometry_cases()
FUSED_BACKWARD_CASES = E.fused_backward_cases() + E.split_geometry_cases()
UNFUSED_BACKWARD_CASES = E.unfused_backward_cases() + E.split_encoded_cases()


def ident(case):
    return "-".join(str(k) for k in case["key"])


def on_dev(dev, case):
    """The case's device tensors (parameters and packs cached per model)."""
    key = ("case",) + case["key"]
    if key not in _DEV:
        pk = ("params", id(case["params"]))
        if pk not in _DEV:
            _DEV[pk] = [t.to(dev) for t in E.params_list(case["params"])]
        d = {"params": _DEV[pk], "pk": pk}
        for k in ("zs", "zt", "code_index", "x", "ro", "rd", "z", "pts", "d_raw"):
            d[k] = case[k].to(dev) if case.get(k) is not None else None
        _DEV[key] = d
    return _DEV[key]


def packed(dev, case, fmt):
    from codenerf import ops
    d = on_dev(dev, case)
    key = ("pack", d["pk"], fmt)
    if key not in _DEV:
        _DEV[key] = ops.mlp_pack(d["params"], fmt)
    return _DEV[key]


def code_bias(dev, case):
    from codenerf import ops
    d = on_dev(dev, case)
    return ops.code_bias(d["params"], d["zs"], d["zt"])


def same(got, ref, what):
    """torch.equal(got, float64 reference cast to fp32), with the first difference in the message."""
    got, ref = got.detach().cpu(), ref.float()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} values differ; first at {i}: "
                             f"got {got[i].item()!r}, reference {ref[i].item()!r}")


def geo_inputs(case, d):
    """The point inputs of a geometry case: pts, or ro + z."""
    if case["mode"] == "pts":
        return dict(pts=d["pts"])
    return dict(ro=d["ro"], z=d["z"])


def same_masks(masks, ref, m):
    """The decoded ReLU masks equal the reference's decisions (``pre > 0``), zeros included."""
    for k in E.RELU_LAYERS:
        same(masks[k], ref["decisions"][k], f"ReLU decisions {k}")
        assert masks[k].shape[0] == m


def same_param_grads(case, names, grads, ref):
    for name, g in zip(names, grads):
        cols = E.exact_columns(name, case["geometry"])
        want = ref["grads"][name]
        if cols is not None:
            g, want = g[:, cols], want[:, cols]
        same(g, want, "d " + name)


# ---------------------------------------------------------------- 1. encoded forward


@pytest.mark.parametrize("fmt", FORWARD_FORMATS)
def test_encoded_forward_model_set(dev, fmt):
    """cn_mlp_forward, m = 257, the whole model set (every row and column of every pack nonzero somewhere,
    all columns different: test_exact_cases_cpu): raw; the fused code bias."""
    from codenerf import ops
    for j in range(E.N_MODELS):
        case = E.encoded_case(j, 257, "index")
        d, ref = on_dev(dev, case), E.reference(case)
        cb = code_bias(dev, case)
        same(cb, ref["code_bias"], f"model {j} code_bias")
        raw = ops.mlp_forward(packed(dev, case, fmt), cb, d["x"], d["code_index"], precision=fmt)
        same(raw, ref["raw"], f"model {j} raw")


@pytest.mark.parametrize("model", E.DENSE_MODELS)
@pytest.mark.parametrize("fmt", FORWARD_FORMATS)
def test_encoded_forward_dense_layer(dev, fmt, model):
    """cn_mlp_forward, m = 257, with one layer dense (every entry nonzero, neighbours mostly different): a
    single misplaced element of that layer's part of the pack, which the sparse set sees only where it
    holds a nonzero."""
    from codenerf import ops
    case = E.encoded_case(model, 257, "index")
    d, ref = on_dev(dev, case), E.reference(case)
    cb = code_bias(dev, case)
    same(cb, ref["code_bias"], "code_bias")
    raw = ops.mlp_forward(packed(dev, case, fmt), cb, d["x"], d["code_index"], precision=fmt)
    same(raw, ref["raw"], "raw")


@pytest.mark.parametrize("model", E.SPLIT_MODELS)
@pytest.mark.parametrize("fmt", FORWARD_FORMATS)
def test_encoded_forward_split_layer(dev, fmt, model):
    """cn_mlp_forward, m = 257, with one layer's weights carrying a bf16 low part: the lo fragments of the
    bf16x3 / bf16x3_w16 packs and the B operand the lo product reads; the fp32 formats as a cross-check."""
    from codenerf import ops
    case = E.encoded_case(model, 257, "index")
    d, ref = on_dev(dev, case), E.reference(case)
    cb = code_bias(dev, case)
    same(cb, ref["code_bias"], "code_bias")
    raw = ops.mlp_forward(packed(dev, case, fmt), cb, d["x"], d["code_index"], precision=fmt)
    same(raw, ref["raw"], "raw")


@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("m", E.ENCODED_SIZES)
@pytest.mark.parametrize("fmt", FORWARD_FORMATS)
def test_encoded_forward_sizes_and_code_layouts(dev, fmt, m, layout):
    """cn_mlp_forward around the 32-sample wave and the 128-sample tile with one code row, one per sample
    and a code_index with repeats, out of order, neighbouring rows on different codes."""
    from codenerf import ops
    case = E.encoded_case(0, m, layout)
    d, ref = on_dev(dev, case), E.reference(case)
    raw = ops.mlp_forward(packed(dev, case, fmt), code_bias(dev, case), d["x"], d["code_index"], precision=fmt)
    same(raw, ref["raw"], "raw")


@pytest.mark.parametrize("fmt", FORWARD_FORMATS)
def test_encoded_forward_second_tile_of_every_workgroup(dev, fmt):
    """m = 128 (CUs + 3) + 5: every persistent workgroup takes a second tile, the last tile is ragged."""
    from codenerf import ops
    m = E.persistent_rows(torch.cuda.get_device_properties(dev).multi_processor_count)
    case = E.encoded_case(0, m, "index")
    E.check_exact(case, backward=False)
    d, ref = on_dev(dev, case), E.reference(case)
    raw = ops.mlp_forward(packed(dev, case, fmt), code_bias(dev, case), d["x"], d["code_index"], precision=fmt)
    same(raw, ref["raw"], "raw")


@pytest.mark.parametrize("m,layout", [(257, "index"), (129, "per_row"), (33, "one")])
def test_density_encoded_rows(dev, m, layout):
    """cn_density_field on encoded rows ((m, 90) and the (m, 63) xyz columns alone): sigma_raw."""
    from codenerf import ops
    case = E.encoded_case(0, m, layout)
    d, ref = on_dev(dev, case), E.reference(case)
    cb = code_bias(dev, case)
    for x in (d["x"], d["x"][:, :63].contiguous()):
        sigma, raw = ops.density_field(packed(dev, case, "f32_w16"), cb, FX, x=x, code_index=d["code_index"],
                                       want_raw=True)
        same(sigma, ref["raw"][:, 3], "sigma")
        same(raw[:, 3], ref["raw"][:, 3], "raw sigma")
        assert not bool(raw[:, :3].any())


# ---------------------------------------------------------------- 2. training forwards


def test_encoded_forward_train(dev):
    """cn_mlp_forward_train: raw and the five saved planes."""
    from codenerf import ops
    case = E.train_forward_cases()[0]
    d, ref = on_dev(dev, case), E.reference(case)
    raw, saved = ops.mlp_forward_train(packed(dev, case, "f32"), code_bias(dev, case), d["x"], d["code_index"])
    same(raw, ref["raw"], "raw")
    for k, name in enumerate(E.PLANES):
        same(saved[k], ref["planes"][k], "plane " + name)


@pytest.mark.parametrize("case", TRAIN_FORWARD_CASES, ids=ident)
@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f32_v1"])
def test_geometry_forward_train(dev, case, precision):
    """cn_radiance_field_train_fmt ("f32": f32_w16, "bf16x3") and cn_radiance_field_train ("f32_v1", no
    masks): raw, all five planes, and the ReLU masks decoded to the reference's decisions, zeros included.
    On the split models' cases the training forward's lo fragments."""
    from codenerf import ops
    d, ref = on_dev(dev, case), E.reference(case)
    r, s, chunk = case["r"], case["s"], case["chunk"]
    cb = code_bias(dev, case)
    if precision == "f32_v1":
        raw, saved = ops.radiance_field_train(packed(dev, case, "f32"), cb, d["rd"], s, chunk, FX, FD,
                                              code_index=d["code_index"], **geo_inputs(case, d))
        masks = None
    else:
        fmt = "bf16x3" if precision == "bf16x3" else "f32_w16"
        raw, saved, masks = ops.radiance_field_train_w16(packed(dev, case, fmt), cb, d["rd"], s, chunk, FX, FD,
                                                         code_index=d["code_index"], precision=precision,
                                                         **geo_inputs(case, d))
    same(raw.reshape(-1, 4), ref["raw"], "raw")
    for k, name in enumerate(E.PLANES):
        same(saved[k], ref["planes"][k], "plane " + name)
    if masks is not None:
        decode = decode_relu_masks if precision == "bf16x3" else decode_relu_masks_w16
        same_masks(decode(masks, r * s), ref, r * s)


# ---------------------------------------------------------------- 3. geometry forward


@pytest.mark.parametrize("case", GEOMETRY_FORWARD_CASES, ids=ident)
@pytest.mark.parametrize("fmt", FORWARD_FORMATS + ("density",))
def test_geometry_forward(dev, case, fmt):
    """cn_radiance_field in the four inference formats and cn_density_field, from points and from rays +
    depths: short last chunks, chunks that are no multiple of the tile, the Q1 ray of every row, the code row
    of every ray.  On the split models' cases the lo fragments of both 3xbf16 packs."""
    from codenerf import ops
    d, ref = on_dev(dev, case), E.reference(case)
    r, s, chunk = case["r"], case["s"], case["chunk"]
    cb = code_bias(dev, case)
    if fmt == "density":
        kw = dict(pts=d["pts"]) if case["mode"] == "pts" else dict(ro=d["ro"], rd=d["rd"], z=d["z"])
        sigma = ops.density_field(packed(dev, case, "f32_w16"), cb, FX, code_index=d["code_index"], **kw)
        same(sigma.reshape(-1), ref["raw"][:, 3], "sigma")
        return
    raw = ops.radiance_field(packed(dev, case, fmt), cb, d["rd"], s, chunk, FX, FD, code_index=d["code_index"],
                             precision=fmt, **geo_inputs(case, d))
    same(raw.reshape(-1, 4), ref["raw"], "raw")


# ---------------------------------------------------------------- 4. backwards


@pytest.mark.parametrize("case", FUSED_BACKWARD_CASES, ids=ident)
@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_fused_backward_eval(dev, case, precision, deterministic):
    """cn_radiance_field_masks_fmt + cn_field_backward_fused_ws (``deterministic``: with whole waves per ray,
    the (3, 64, 2) shape, its form without float atomics; else, and with deterministic False, the atomic
    kernel): raw, the masks, g_code, d pts or d ro, d rd.  A tie at 0 gives gradient 0.  On the split models'
    cases the lo fragments of the transposed packs the dX chain streams."""
    from codenerf import ops
    d, ref = on_dev(dev, case), E.reference(case)
    r, s, chunk = case["r"], case["s"], case["chunk"]
    fmt = "bf16x3" if precision == "bf16x3" else "f32_w16"
    geo = geo_inputs(case, d)
    raw, masks = ops.radiance_field_masks(packed(dev, case, fmt), code_bias(dev, case), d["rd"], s, chunk, FX, FD,
                                          code_index=d["code_index"], precision=precision, **geo)
    same(raw.reshape(-1, 4), ref["raw"], "raw")
    decode = decode_relu_masks if precision == "bf16x3" else decode_relu_masks_w16
    same_masks(decode(masks, r * s), ref, r * s)
    pts_mode = case["mode"] == "pts"
    out = ops.field_backward_x3(packed(dev, case, fmt + "_t"), masks, d["d_raw"], r, s, chunk, case["zs"].shape[0],
                                FX, FD, d["rd"], code_index=d["code_index"], want_pts=pts_mode, want_ro=not pts_mode,
                                want_rd=True, precision=precision, deterministic=deterministic, **geo)
    same(out["g_code"], ref["g_code"], "g_code")
    same(out["d_rd"], ref["d_rd"], "d rd")
    if pts_mode:
        same(out["d_pts"].reshape(-1, 3), ref["d_pts"].reshape(-1, 3), "d pts")
    else:
        same(out["d_ro"], ref["d_ro"], "d ro")


@pytest.mark.parametrize("case", FUSED_BACKWARD_CASES, ids=ident)
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_fused_backward_train(dev, case, precision):
    """cn_radiance_field_train_fmt + cn_field_backward_train_multi (one field) + the code backward: every
    parameter gradient, g_code, d z_s / d z_t, d pts or d ro, d rd.  On the split models' cases the transposed
    pack's lo fragments, and dW GEMMs whose operands carry low parts on one side at a time."""
    from codenerf import ops
    d, ref = on_dev(dev, case), E.reference(case)
    r, s, chunk = case["r"], case["s"], case["chunk"]
    fmt = "bf16x3" if precision == "bf16x3" else "f32_w16"
    geo = geo_inputs(case, d)
    raw, saved, masks = ops.radiance_field_train_w16(packed(dev, case, fmt), code_bias(dev, case), d["rd"], s, chunk,
                                                     FX, FD, code_index=d["code_index"], precision=precision, **geo)
    same(raw.reshape(-1, 4), ref["raw"], "raw")
    pg = [torch.zeros_like(p) for p in d["params"]]
    pts_mode = case["mode"] == "pts"
    out = ops.field_backward_train_multi([dict(
        packed_t=packed(dev, case, fmt + "_t"), params=d["params"], masks=masks, saved=saved, x_enc=None,
        d_raw=d["d_raw"], n_rays=r, n_samples=s, chunk_rows=chunk, n_codes=case["zs"].shape[0], freqs_xyz=FX,
        freqs_dir=FD, rd=d["rd"], code_index=d["code_index"], param_grads=pg, want_pts=pts_mode,
        want_ro=not pts_mode, want_rd=True, **geo)], precision)[0]
    same(out["g_code"], ref["g_code"], "g_code")
    dz_s, dz_t = ops.code_bias_backward(d["params"], d["zs"], d["zt"], out["g_code"], pg)
    same(dz_s, ref["dz_s"], "d z_s")
    same(dz_t, ref["dz_t"], "d z_t")
    same_param_grads(case, list(case["params"]), pg, ref)
    same(out["d_rd"], ref["d_rd"], "d rd")
    if pts_mode:
        same(out["d_pts"].reshape(-1, 3), ref["d_pts"].reshape(-1, 3), "d pts")
    else:
        same(out["d_ro"], ref["d_ro"], "d ro")


@pytest.mark.parametrize("case", UNFUSED_BACKWARD_CASES, ids=ident)
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_unfused_backward_encoded(dev, case, precision):
    """cn_mlp_forward_train + cn_field_backward_fmt on encoded rows + the code backward: d x, every parameter
    gradient (all columns: the encodings are integers here), g_code, d z_s / d z_t.  On the split models the
    weight split that cn_gemm_nn_x3 makes itself from the fp32 weights."""
    from codenerf import ops
    d, ref = on_dev(dev, case), E.reference(case)
    m, n_codes = case["m"], case["zs"].shape[0]
    raw, saved = ops.mlp_forward_train(packed(dev, case, "f32"), code_bias(dev, case), d["x"], d["code_index"])
    same(raw, ref["raw"], "raw")
    pg = [torch.zeros_like(p) for p in d["params"]]
    out = ops.field_backward(d["params"], saved, d["x"], d["d_raw"], m, 1, m, n_codes, code_index=d["code_index"],
                             param_grads=pg, want_code=True, want_x=True, precision=precision)
    same(out["d_x"], ref["d_x"], "d x")
    same(out["g_code"], ref["g_code"], "g_code")
    dz_s, dz_t = ops.code_bias_backward(d["params"], d["zs"], d["zt"], out["g_code"], pg)
    same(dz_s, ref["dz_s"], "d z_s")
    same(dz_t, ref["dz_t"], "d z_t")
    same_param_grads(case, list(case["params"]), pg, ref)


@pytest.mark.parametrize("case", E.unfused_backward_cases(), ids=ident)
@pytest.mark.parametrize("single_launch", [False, True])
def test_code_backward(dev, case, single_launch):
    """cn_code_bias_backward and its two-launch form from the reference's g_code: d z_s, d z_t, the code
    layers' weight and bias gradients and the code halves of layer_xyz2 / fc_out / fc_rgb."""
    from codenerf import ops
    d, ref = on_dev(dev, case), E.reference(case)
    names = list(case["params"])
    pg = [torch.zeros_like(p) for p in d["params"]]
    dz_s, dz_t = ops.code_bias_backward(d["params"], d["zs"], d["zt"], ref["g_code"].float().to(dev), pg,
                                        single_launch=single_launch)
    same(dz_s, ref["dz_s"], "d z_s")
    same(dz_t, ref["dz_t"], "d z_t")
    for name, g in zip(names, pg):
        layer = name.split(".")[0]
        if layer in ("shape_code_layer1", "shape_code_layer2", "texture_code_layer1"):
            same(g, ref["grads"][name], "d " + name)
        elif name in ("layer_xyz2.weight", "fc_out.weight", "fc_rgb.weight"):
            same(g[:, E.HID:], ref["grads"][name][:, E.HID:], "d " + name + " (code half)")
