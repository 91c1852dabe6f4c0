"""Integer-exact probes of the field kernels (mlp.hip, mlp_f32.hip, mlp_x3.hip, mlp_x3w.hip and the
fused backwards of grad.hip): seeded builders, a float64 reference and the conditions under which
every fp32 / 3xbf16 kernel must return that reference bit for bit.

With small-integer weights, biases, codes and inputs every product and every partial sum of the
network is an integer; while the sum of the terms' magnitudes stays below 2^24, fp32 holds every
partial sum exactly in ANY summation order (MFMA tiles, butterflies, atomics).  A 3xbf16 product
Ah.Bh + Ah.Bl + Al.Bh drops only Al.Bl, so it is exact when one operand is a bf16 number (Al = 0:
every weight of the integer models is) or, for the dW GEMMs whose operands are both activations, when
no term has two operands with a bf16 low part; a value splits exactly into hi + lo when it is an
integer below 2^16.
check_exact() asserts those conditions on the float64 reference alone; tests/test_exact_cases_cpu.py
proves them (and that the fp32 oracle returns the reference bit for bit), tests/test_gpu_field_exact.py
runs the kernels.  Everything here is CPU torch / numpy; builders are seeded, references are computed
once per case and must not be modified.

Low weight fragments.  With bf16 weights the third product of every 3xbf16 group multiplies zeros, so
the models "split:<layer>" give the nonzero weights of ONE GEMM layer a bf16 low part (nine or ten
significant bits, dyadic: multiples of the unit u = 2^-8) and the argument above is restated in units
of u:
  - every quantity of the reference -- planes, pre-activations, raw, code_bias, the masked layer
    gradients, parameter gradients, g_code, dz and the input gradients -- is a multiple of u (the
    other layers' weights, the biases, codes, inputs and d_raw stay integers), and every bounded sum of
    |terms|, divided by u, stays below 2^24: fp32 again holds every partial sum in any order;
  - every 3xbf16 operand (x, h1, h2, feat, v1, v2, code_bias, every masked layer gradient and the
    weights) splits exactly, hi = bf16(v), lo = bf16(v - hi), hi + lo == v, both rounded to nearest
    even as the packs and the kernels round them; check_exact makes that split and compares (a
    multiple of u is no integer below 2^16, so that shortcut is not used for these models);
  - no term has two low parts, which is all that Ah.Bh + Ah.Bl + Al.Bh drops: forward, per layer, no
    input with a low part meets a weight with one; dX, per layer, no masked gradient with a low part
    meets such a weight; dW, as before, no masked gradient with a low part meets an input with one.
    In the split layer itself the inputs that meet its weights are therefore bf16 numbers, so Wl.Xl in
    place of Wl.Xh would lose exactly what dropping Wl.Xh loses;
  - fc_out row 0 (sigma) is an fp32 dot product in every kernel and stays a bf16 row.
So on a split model the lo fragments of the packs, the operand the lo product reads and the weight
split inside the unfused backward's GEMMs are compared bit for bit like everything else, forward and
backward.  x3_raw() / x3_swapped_lo() emulate the three-product rule in float64:
tests/test_exact_cases_cpu.py shows with them that the rule returns the reference exactly, and that a
dropped or misread lo product, or the lo parts of two neighbouring rows or columns changing places,
changes raw.

Geometry cases (points / rays instead of encoded rows): sin / cos encodings are not integers, so
geometry models carry zero weights on every sin / cos column of layer_xyz1 and layer_dir1 (finite x 0
is exactly 0 in every format); points, origins and depths are small integers and ray directions
+-e_i times a length in {1, 2, 4}, so ro + rd z, |rd|, rd / |rd| and its gradient are exact.  The
gradients of layer_xyz1 / layer_dir1 with respect to those zero sin / cos columns are sums of
non-integers and are NOT exact: exact_columns() names the columns a geometry case compares.  Ray
gradients are multiples of 1 / |rd| >= 1/4 (of u / 4 on a split model).
"""
import zlib
from collections import OrderedDict

import numpy as np
import torch

from codenerf import synthetic
from oracle import codenerf_oracle as O

F32, F64 = torch.float32, torch.float64
HID = 256
CB_STRIDE = 520          # include/codenerf.h CN_CODE_BIAS_STRIDE: c_xyz2[256] c_feat[256] c_sigma c_rgb[3] pad[4]
LIMIT_SUM = float(2 ** 24)
LIMIT_X3 = float(2 ** 16)
VALUES = np.array([-3, -2, -1, 1, 2, 3], dtype=np.float32)
PLANES = ("h1", "h2", "feat", "v1", "v2")
RELU_LAYERS = ("h1", "h2", "v1", "v2")
CODE_LAYERS = ("s1", "s2", "t1")

# Nonzeros per row.  The 256- / 512-wide layers stay sparse so that magnitudes grow slowly through the
# five layers; fc_rgb (3 rows) is half dense: with 4 models its 512 columns are 12 entries long,
# which is what makes them pairwise different and all nonzero somewhere (test_exact_cases_cpu).
NNZ = {"layer_xyz1": 4, "layer_xyz2": 4, "fc_out": 4, "shape_code_layer1": 4, "shape_code_layer2": 4,
       "texture_code_layer1": 4, "layer_dir1": 4, "layer_dir2": 4, "fc_rgb": 256}
N_MODELS = 4
N_GEO_MODELS = 4
NNZ_SIGMA = 64           # fc_out row 0: sigma_raw is one row, and 4 inputs would leave it constant on many codes
N_CODES = 5              # rows of the code table a code_index picks from
# The sparse set proves rows, columns and blocks; a single misplaced ELEMENT shows only where a weight is
# nonzero.  So each layer also gets a model in which it alone is dense (every allowed entry in +-{1, 2, 3})
# and the others are sparser still, to keep the sums inside the limits: model "dense:<layer>".
NNZ_THIN = {k: 2 for k in NNZ}
NNZ_THIN["fc_rgb"] = 32
NNZ_SIGMA_THIN = 16
DENSE_MODELS = tuple("dense:" + k for k in NNZ)
# Every weight above is a bf16 number, so the third product of a 3xbf16 group (Wl.Xh) multiplies zeros.
# Model "split:<layer>" (one of a set: "split:<layer>:<j>") gives the nonzero weights of one GEMM layer a
# bf16 low part: +-(1|2) +- (1|2)/256 (the four of those that need nine or ten significant bits: 1 + 2/256,
# 1 - 1/256, 1 - 2/256 and 2 - 2/256 are bf16 numbers), multiples of the unit U = 2^-8.  Every
# other layer stays thin with bf16 weights (some in +-1 only, where the magnitudes would otherwise outgrow an
# exact hi + lo split); fc_out row 0 (sigma, an fp32 dot product in every kernel) stays a bf16 row.
U = 2.0 ** -8
SPLIT_VALUES = np.array([257, 511, 513, 514]) * U    # those of (1|2) +- (1|2)/256 that are no bf16 numbers
SPLIT_LAYERS = ("layer_xyz1", "layer_xyz2", "fc_out", "layer_dir1", "layer_dir2", "fc_rgb")
# Models in a layer's set.  One model covers every row and column of a 256-row layer, but behind thin layers
# some units are dead on every row of a case, and a wrong fragment in front of them would not reach raw: two
# models, so that every pair of neighbouring rows and columns is seen in raw (test_exact_cases_cpu).  fc_rgb's
# 3 rows cannot fill 512 columns in one model and keep the rgb sums small.
SPLIT_COUNT = {k: 2 for k in SPLIT_LAYERS}
SPLIT_COUNT["fc_rgb"] = 4
SPLIT_NNZ = {k: 4 for k in SPLIT_LAYERS}
SPLIT_NNZ["fc_rgb"] = 64
SPLIT_MODELS = tuple("split:" + k if SPLIT_COUNT[k] == 1 else f"split:{k}:{j}"
                     for k in SPLIT_LAYERS for j in range(SPLIT_COUNT[k]))
# (layer, geometry) -> the layers of that model whose bf16 weights are drawn from +-1 alone.  Geometry: point
# coordinates reach 23, and with +-{1, 2} the activations behind the split layer outgrow an exact hi + lo
# split (about 2^16 units); fc_rgb: every v2 it reads must be a bf16 number, an integer of 8 significant bits.
SPLIT_ONES = {(k, True): tuple(NNZ) for k in SPLIT_LAYERS}
SPLIT_ONES[("fc_rgb", False)] = tuple(NNZ)
SPLIT_SEED = {("layer_xyz2", True): 1}           # redrawn until check_exact holds on every case of the set


def _rng(*key) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------------------------------------
# probe models
# ---------------------------------------------------------------------------------------------


def allowed_columns(name: str, width: int, geometry: bool) -> np.ndarray:
    """Columns of layer ``name`` a probe model may fill: all, or for a geometry model's layer_xyz1 /
    layer_dir1 only those that multiply raw inputs (x_d: 0..2; feat 0..255 and view d: 256..258)."""
    if geometry and name == "layer_xyz1":
        return np.arange(3)
    if geometry and name == "layer_dir1":
        return np.arange(HID + 3)
    return np.arange(width)


def exact_columns(name: str, geometry: bool):
    """Columns of parameter ``name``'s gradient that a case compares bit for bit (None: all)."""
    if geometry and name == "layer_xyz1.weight":
        return slice(0, 3)
    if geometry and name == "layer_dir1.weight":
        return slice(0, HID + 3)
    return None


_MODELS = {}


def probe_model(index, geometry: bool = False) -> "OrderedDict[str, torch.Tensor]":
    """Model "dense:<layer>" (see DENSE_MODELS), or model ``index`` of the encoded (N_MODELS) or geometry
    (N_GEO_MODELS) probe set: a CodeNeRFModel
    state dict (synthetic.layer_shapes(), fp32) of sparse weights in +-{1, 2, 3} (NNZ per row, then one
    more in every column the rows left empty: fc_rgb's in the columns c % (models in the set) == index only) and
    biases in -2..2."""
    key = (index, geometry)
    if key in _MODELS:
        return _MODELS[key]
    if isinstance(index, str) and index.startswith("split:"):
        _MODELS[key] = _split_model(index, geometry)
        return _MODELS[key]
    rng = _rng("model", index, geometry)
    dense = index[len("dense:"):] if isinstance(index, str) else None
    nnz, nnz_sigma = (NNZ_THIN, NNZ_SIGMA_THIN) if dense else (NNZ, NNZ_SIGMA)
    out = OrderedDict()
    for name, (o, i) in synthetic.layer_shapes().items():
        cols = allowed_columns(name, i, geometry)
        k = len(cols) if name == dense else min(nnz[name], max(1, len(cols) - 1))
        w = np.zeros((o, i), dtype=np.float32)
        for r in range(o):
            kr = max(k, nnz_sigma) if (name == "fc_out" and r == 0) else k
            w[r, rng.choice(cols, size=kr, replace=False)] = rng.choice(VALUES, size=kr)
        empty = cols[(w[:, cols] != 0).sum(axis=0) == 0]
        if name == "fc_rgb" and not dense:
            count = N_GEO_MODELS if geometry else N_MODELS
            empty = empty[empty % count == index % count]
        for c in empty:
            w[rng.integers(o), c] = rng.choice(VALUES)
        out[name + ".weight"] = torch.from_numpy(w)
        out[name + ".bias"] = torch.from_numpy(rng.integers(-2, 3, size=o).astype(np.float32))
    _MODELS[key] = out
    return out


def split_name(model):
    """("split:<layer>" | "split:<layer>:<j>") -> (layer, j, models in the layer's set); None for other models."""
    if not (isinstance(model, str) and model.startswith("split:")):
        return None
    parts = model.split(":")
    return parts[1], int(parts[2]) if len(parts) > 2 else 0, SPLIT_COUNT[parts[1]]


def split_set(layer: str):
    return tuple(m for m in SPLIT_MODELS if split_name(m)[0] == layer)


def _split_model(name: str, geometry: bool):
    """Model "split:<layer>[:<j>]" (see SPLIT_MODELS): the named layer holds SPLIT_NNZ weights per row in
    +-SPLIT_VALUES, then one more in every allowed column the rows left empty (of a set of several
    models: in the columns c % (models in the set) == j), fc_out row 0 excepted; every other layer is thin
    (NNZ_THIN per row in +-{1, 2}, or +-1 for SPLIT_ONES, then its empty columns) and biases are in -1..1."""
    layer, j, count = split_name(name)
    rng = _rng("model", name, geometry, SPLIT_SEED.get((layer, geometry), 0))
    ones = SPLIT_ONES.get((layer, geometry), ())
    out = OrderedDict()

    def draw(split: bool, only_ones: bool, size: int):
        sign = rng.choice([-1.0, 1.0], size=size)
        if split:
            return (sign * rng.choice(SPLIT_VALUES, size=size)).astype(np.float32)
        return (sign * (1.0 if only_ones else rng.choice([1.0, 2.0], size=size))).astype(np.float32)
    for lname, (o, i) in synthetic.layer_shapes().items():
        cols = allowed_columns(lname, i, geometry)
        split = lname == layer
        k = min(SPLIT_NNZ[lname] if split else NNZ_THIN[lname], max(1, len(cols) - 1))
        w = np.zeros((o, i), dtype=np.float32)
        for r in range(o):
            sigma = lname == "fc_out" and r == 0
            kr = max(k, NNZ_SIGMA_THIN) if sigma else k
            w[r, rng.choice(cols, size=kr, replace=False)] = draw(split and not sigma, lname in ones, kr)
        empty = cols[(w[int(lname == "fc_out"):, cols] != 0).sum(axis=0) == 0]
        if split:
            empty = empty[empty % count == j]
        for c in empty:
            w[rng.integers(int(lname == "fc_out"), o), c] = draw(split, lname in ones, 1)[0]
        out[lname + ".weight"] = torch.from_numpy(w)
        out[lname + ".bias"] = torch.from_numpy(rng.integers(-1, 2, size=o).astype(np.float32))
    return out


def model_set(geometry: bool = False):
    return [probe_model(j, geometry) for j in range(N_GEO_MODELS if geometry else N_MODELS)]


def params_list(p):
    """The 18 tensors in state_dict order (what the C ABI takes)."""
    return [p[k] for k in p]


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------

LAYOUTS = ("one", "per_row", "index")     # one code row | one per sample (ray) | picked by code_index


def _codes(rng, layout: str, owners: int):
    """z_s, z_t (n_codes, 256) in -2..2 and the code_index (owners,) or None.  "index": N_CODES rows picked
    by a random (hashed) index: repeats, out of order, neighbours on different rows."""
    n = {"one": 1, "per_row": owners, "index": N_CODES}[layout]
    zs = torch.from_numpy(rng.integers(-2, 3, size=(n, 256)).astype(np.float32))
    zt = torch.from_numpy(rng.integers(-2, 3, size=(n, 256)).astype(np.float32))
    ci = torch.from_numpy(rng.integers(0, n, size=owners)) if layout == "index" else None
    return zs, zt, ci


def _d_raw(rng, m: int):
    """Integer upstream gradient (m, 4) in +-{1, 2}, nonzero on about a quarter of the rows, at most about
    64 (and on the first and last): few enough for the dW / g_code sums to stay exact, spread enough that a wrong ray or
    code row shows."""
    d = rng.choice(np.array([-2, -1, 1, 2], dtype=np.float32), size=(m, 4))
    keep = rng.random(m) < min(0.25, 64.0 / m)
    keep[[0, m - 1]] = True
    return torch.from_numpy(d * keep[:, None].astype(np.float32))


_CASES = {}


def encoded_case(model, m: int, layout: str = "one"):
    """(m, 90) integer rows in -2..2 for cn_mlp_forward / cn_mlp_forward_train."""
    key = ("enc", model, m, layout)
    if key not in _CASES:
        rng = _rng(*key)
        zs, zt, ci = _codes(rng, layout, m)
        x = torch.from_numpy(rng.integers(-2, 3, size=(m, 90)).astype(np.float32))
        _CASES[key] = dict(key=key, mode="enc", geometry=False, params=probe_model(model), m=m, x=x, zs=zs, zt=zt,
                           code_index=ci, d_raw=_d_raw(rng, m))
    return _CASES[key]


def geometry_case(model: int, mode: str, r: int, s: int, chunk: int, layout: str = "one"):
    """``mode`` "pts" (points given) or "rayz" (origins + depths): r rays x s samples in chunks of ``chunk``
    rays.  ro in -3..3, depths 1..5, rd = +-e_i * {1, 2, 4} with axis, sign and length drawn per ray."""
    key = ("geo", model, mode, r, s, chunk, layout)
    if key not in _CASES:
        rng = _rng(*key)
        zs, zt, ci = _codes(rng, layout, r)
        ro = torch.from_numpy(rng.integers(-3, 4, size=(r, 3)).astype(np.float32))
        rd = torch.zeros(r, 3)
        rd[torch.arange(r), torch.from_numpy(rng.integers(0, 3, size=r))] = torch.from_numpy(
            (rng.choice([-1.0, 1.0], size=r) * rng.choice([1.0, 2.0, 4.0], size=r)).astype(np.float32))
        z = torch.from_numpy(rng.integers(1, 6, size=(r, s)).astype(np.float32))
        pts = ro[:, None, :] + rd[:, None, :] * z[..., None]
        _CASES[key] = dict(key=key, mode=mode, geometry=True, params=probe_model(model, True), m=r * s, r=r, s=s,
                           chunk=chunk, ro=ro, rd=rd, z=z, pts=pts, zs=zs, zt=zt, code_index=ci,
                           d_raw=_d_raw(rng, r * s))
    return _CASES[key]


# (rays, samples, chunk_rows): one sample; a short last chunk (7 = 3 + 3 + 1); chunks of 80 samples, not a
# multiple of the 128-sample tile, and a short last chunk (37 = 3 x 10 + 7); one chunk of 150 samples
# (ragged tile); 130 one-sample rays in chunks of 64 (short last chunk of 2); 64-sample rays in chunks of
# 2 (128 samples, a whole tile) with a short last chunk of 1
GEOMETRY_SHAPES = ((1, 1, 1), (7, 5, 3), (37, 8, 10), (50, 3, 50), (130, 1, 64), (3, 64, 2))
BACKWARD_SHAPES = ((37, 8, 10), (7, 5, 3))
ENCODED_SIZES = (1, 31, 32, 33, 127, 128, 129, 255, 256)


def persistent_rows(cu_count: int) -> int:
    """Rows at which every persistent workgroup (one per CU) takes a second 128-sample tile and the last
    tile is ragged."""
    return 128 * (cu_count + 3) + 5


def encoded_forward_cases():
    """Test 1: the whole model set at m = 257, then one model at every size with every code layout."""
    return ([encoded_case(j, 257, "index") for j in range(N_MODELS)]
            + [encoded_case(0, m, layout) for m in ENCODED_SIZES for layout in LAYOUTS])


def dense_forward_cases():
    """Test 1, single elements: one model per layer with that layer dense, m = 257."""
    return [encoded_case(name, 257, "index") for name in DENSE_MODELS]


def geometry_forward_cases():
    """Test 3: both modes at every shape; the three code layouts at (37, 8, 10), one other layout elsewhere."""
    out = []
    for i, (r, s, chunk) in enumerate(GEOMETRY_SHAPES):
        layouts = LAYOUTS if (r, s, chunk) == (37, 8, 10) else (("index", "per_row")[i % 2],)
        out += [geometry_case(i % N_GEO_MODELS, mode, r, s, chunk, layout) for mode in ("pts", "rayz")
                for layout in layouts]
    return out


def train_forward_cases():
    """Test 2: encoded rows, and geometry with one code row per wave (n_codes == 1) or picked per ray."""
    return [encoded_case(1, 257, "index"), geometry_case(0, "rayz", 37, 8, 10, "one"),
            geometry_case(1, "pts", 7, 5, 3, "one"), geometry_case(1, "rayz", 3, 64, 2, "index")]


def fused_backward_cases():
    """Test 4, fused backwards: one code row (what every fused backward takes at 8 and 5 samples per ray);
    (3, 64, 2) has whole waves per ray: the form without float atomics."""
    out = [geometry_case(i % N_GEO_MODELS, mode, r, s, chunk, "one") for i, (r, s, chunk) in
           enumerate(BACKWARD_SHAPES + ((3, 64, 2),)) for mode in ("pts", "rayz")]
    # whole waves per ray also admit a code row per ray: g_code rows picked by code_index
    return out + [geometry_case(3, mode, 3, 64, 2, "index") for mode in ("pts", "rayz")]


def unfused_backward_cases():
    return [encoded_case(2, 257, "index"), encoded_case(3, 257, "one")]


def backward_cases():
    return fused_backward_cases() + unfused_backward_cases() + split_encoded_cases() + split_geometry_cases()


def split_encoded_cases():
    """Low weight fragments, encoded rows: every split model at m = 257; forward and the unfused backward."""
    return [encoded_case(name, 257, "index") for name in SPLIT_MODELS]


def split_geometry_cases():
    """Low weight fragments, geometry (forwards and fused backwards): per layer and mode the whole-waves-per-ray
    shape (3, 64, 2) with one code row and with a code row per ray, and (37, 8, 10) with one code row; a
    layer's set of several models is spread over the cases."""
    out = []
    for layer in SPLIT_LAYERS:
        names = split_set(layer)
        shapes = (((3, 64, 2), "one"), ((3, 64, 2), "index"), ((37, 8, 10), "one"))
        for i, mode in enumerate(("pts", "rayz")):
            out += [geometry_case(names[(3 * i + k) % len(names)], mode, *shape, layout)
                    for k, (shape, layout) in enumerate(shapes)]
    return out


def all_cases():
    """Every case the GPU file runs (the persistent one at 256 CUs), once each."""
    seen = {}
    for c in (encoded_forward_cases() + dense_forward_cases() + geometry_forward_cases() + train_forward_cases()
              + backward_cases() + [encoded_case(0, persistent_rows(256), "index")]):
        seen[c["key"]] = c
    return list(seen.values())


def row_maps(case):
    """Per sample row: its code row, and (geometry) the ray whose view direction it takes (quirk Q1: row
    k = r S + s of a chunk of Rc rays takes ray k mod Rc of that chunk)."""
    m = case["m"]
    rows = torch.arange(m)
    if case["mode"] == "enc":
        owner, dray = rows, None
    else:
        r, s, chunk = case["r"], case["s"], case["chunk"]
        ray, smp = rows // s, rows % s
        base = (ray // chunk) * chunk
        rcnt = torch.clamp(r - base, max=chunk)
        dray = base + ((ray - base) * s + smp) % rcnt
        owner = ray
    ci, n = case["code_index"], case["zs"].shape[0]
    code = ci[owner] if ci is not None else (torch.zeros(m, dtype=torch.long) if n == 1 else owner)
    return code, dray


# ---------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------

_REFS = {}


def reference(case):
    """CodeNeRFModel.forward (and forward_pass for geometry) in float64, with the per-code terms formed once
    per code row as the kernels form them (mathematically the reference's), and its gradients for the
    case's integer d_raw by torch.autograd.

    -> dict: raw (m, 4) [rgb, sigma]; planes (5, m, 256) h1 h2 feat v1 v2; pre / decisions: {h1 h2 v1 v2
    s1 s2 t1} pre-activations and ``pre > 0`` as 0/1 (torch's ReLU rule at exactly 0); code_bias (n_codes,
    520); inputs x (m, 90); grads {parameter name -> gradient}; g_code (n_codes, 520); dz_s, dz_t; d_x
    (encoded) or d_pts, d_ro, d_rd (d_ro only for "rayz"); dpre {h1 h2 out v1 v2 rgb s1 s2 t1}: the masked
    layer-input gradients the dW GEMMs read."""
    if case["key"] in _REFS:
        return _REFS[case["key"]]
    relu = torch.nn.functional.relu
    P = {k: v.double().requires_grad_(True) for k, v in case["params"].items()}
    W = lambda n: P[n + ".weight"]   # noqa: E731
    B = lambda n: P[n + ".bias"]     # noqa: E731
    zs, zt = case["zs"].double().requires_grad_(True), case["zt"].double().requires_grad_(True)
    code, dray = row_maps(case)
    leaves = {}
    if case["mode"] == "enc":
        x = leaves["x"] = case["x"].double().requires_grad_(True)
    else:
        rd = leaves["rd"] = case["rd"].double().requires_grad_(True)
        if case["mode"] == "pts":
            pts = leaves["pts"] = case["pts"].double().requires_grad_(True)
        else:
            ro = leaves["ro"] = case["ro"].double().requires_grad_(True)
            pts = ro[:, None, :] + rd[:, None, :] * case["z"].double()[..., None]
        emb = O.EmbedCfg()
        vd = (rd / rd.norm(p=2, dim=-1).unsqueeze(-1))[dray]
        x = torch.cat((O.posenc(pts.reshape(-1, 3), emb.fx.double(), True), O.posenc(vd, emb.fd.double(), True)), dim=-1)
    pre, keep = {}, {}

    def held(name, t):
        t.retain_grad()
        keep[name] = t
        return t
    pre["s1"] = held("s1", zs @ W("shape_code_layer1").t() + B("shape_code_layer1"))
    pre["s2"] = held("s2", zs @ W("shape_code_layer2").t() + B("shape_code_layer2"))
    pre["t1"] = held("t1", zt @ W("texture_code_layer1").t() + B("texture_code_layer1"))
    s1, s2, t1 = relu(pre["s1"]), relu(pre["s2"]), relu(pre["t1"])
    c_xyz2 = held("c_xyz2", s1 @ W("layer_xyz2")[:, HID:].t() + B("layer_xyz2"))
    c_out = held("c_out", s2 @ W("fc_out")[:, HID:].t() + B("fc_out"))
    c_rgb = held("c_rgb", t1 @ W("fc_rgb")[:, HID:].t() + B("fc_rgb"))
    pre["h1"] = held("h1", x[:, :63] @ W("layer_xyz1").t() + B("layer_xyz1"))
    h1 = relu(pre["h1"])
    pre["h2"] = held("h2", h1 @ W("layer_xyz2")[:, :HID].t() + c_xyz2[code])
    h2 = relu(pre["h2"])
    o = held("out", h2 @ W("fc_out")[:, :HID].t() + c_out[code])
    feat = o[:, 1:]
    pre["v1"] = held("v1", torch.cat((feat, x[:, 63:]), dim=-1) @ W("layer_dir1").t() + B("layer_dir1"))
    v1 = relu(pre["v1"])
    pre["v2"] = held("v2", v1 @ W("layer_dir2").t() + B("layer_dir2"))
    v2 = relu(pre["v2"])
    rgb = held("rgb", v2 @ W("fc_rgb")[:, :HID].t() + c_rgb[code])
    raw = torch.cat((rgb, o[:, :1]), dim=-1)
    (raw * case["d_raw"].double()).sum().backward()

    n = zs.shape[0]
    cb, g_code = torch.zeros(n, CB_STRIDE, dtype=F64), torch.zeros(n, CB_STRIDE, dtype=F64)
    for dst, a, b, c in ((cb, c_xyz2.detach(), c_out.detach(), c_rgb.detach()),
                         (g_code, c_xyz2.grad, c_out.grad, c_rgb.grad)):
        dst[:, 0:256], dst[:, 256:512], dst[:, 512], dst[:, 513:516] = a, b[:, 1:], b[:, 0], c
    ref = dict(raw=raw.detach(), planes=torch.stack([t.detach() for t in (h1, h2, feat, v1, v2)]),
               pre={k: v.detach() for k, v in pre.items()},
               decisions={k: (v.detach() > 0).double() for k, v in pre.items()},
               acts=dict(s1=s1.detach(), s2=s2.detach(), t1=t1.detach()), code_bias=cb, x=x.detach(),
               grads={k: v.grad for k, v in P.items()}, g_code=g_code, dz_s=zs.grad, dz_t=zt.grad,
               dpre={k: keep[k].grad for k in ("h1", "h2", "out", "v1", "v2", "rgb", "s1", "s2", "t1")},
               code=code, dray=dray)
    for k, t in leaves.items():
        ref["d_" + k] = t.grad
    _REFS[case["key"]] = ref
    return ref


def oracle_raw(case) -> torch.Tensor:
    """The fp32 CPU oracle on the case: O.codenerf_mlp on encoded rows, O.forward_pass per chunk of rays
    (its own ``repeat`` form of Q1) on geometry -> raw (m, 4)."""
    p = case["params"]
    if case["mode"] == "enc":
        code, _ = row_maps(case)
        return O.codenerf_mlp(p, case["zs"][code], case["zt"][code], case["x"], 63)
    r, chunk = case["r"], case["chunk"]
    ci, n = case["code_index"], case["zs"].shape[0]
    ray_code = ci if ci is not None else (torch.zeros(r, dtype=torch.long) if n == 1 else torch.arange(r))
    zs, zt = case["zs"][ray_code], case["zt"][ray_code]
    pts = case["pts"] if case["mode"] == "pts" else case["ro"][:, None, :] + case["rd"][:, None, :] * case["z"][..., None]
    outs = [O.forward_pass(p, O.EmbedCfg(), case["rd"][c:c + chunk], pts[c:c + chunk], zs[c:c + chunk], zt[c:c + chunk])
            for c in range(0, r, chunk)]
    return torch.cat(outs).reshape(-1, 4)


# ---------------------------------------------------------------------------------------------
# the conditions that make the bitwise claim true
# ---------------------------------------------------------------------------------------------


def _is_bf16(t: torch.Tensor) -> torch.Tensor:
    return t.float().bfloat16().double() == t.double()


def _integers(t: torch.Tensor, unit: float = 1.0) -> bool:
    """Every value is a multiple of ``unit`` (a power of two, so the division is exact)."""
    t = t / unit
    return bool((t == t.round()).all())


def split_bf16(t: torch.Tensor):
    """hi = bf16(v), lo = bf16(v - hi), both rounded to nearest even as the kernels and the packs round
    them -> (hi, lo) in float64."""
    v = t.float()
    hi = v.bfloat16().float()
    lo = (v - hi).bfloat16().float()
    return hi.double(), lo.double()


def _splits(t: torch.Tensor) -> torch.Tensor:
    hi, lo = split_bf16(t)
    return (t.float().double() == t.double()) & (hi + lo == t.double())


def case_unit(case) -> float:
    """The unit every quantity of the case's reference is a multiple of: 1, or U for a split model."""
    return U if split_name(case["key"][1]) else 1.0


def check_exact(case, backward: bool = True) -> dict:
    """Assert, on the float64 reference alone, every condition of the module docstring (``backward`` False:
    those of the forward only, for a case no backward runs on); returns the largest magnitude sum (in units
    of the case's unit) and the largest 3xbf16 operand seen (for the record)."""
    ref = reference(case)
    geo = case["geometry"]
    split = split_name(case["key"][1])
    u = case_unit(case)
    P = {k: v.double() for k, v in case["params"].items()}
    W = lambda n: P[n + ".weight"]   # noqa: E731
    B = lambda n: P[n + ".bias"]     # noqa: E731
    top = {"sum": 0.0, "x3": 0.0}

    def sums(what, s):
        v = float(s.abs().max()) / u if s.numel() else 0.0
        top["sum"] = max(top["sum"], v)
        assert v < LIMIT_SUM, f"{case['key']} {what}: sum of |terms| / unit {v:.4g} >= 2^24"

    def x3(what, t):
        v = float(t.abs().max()) if t.numel() else 0.0
        top["x3"] = max(top["x3"], v)
        if split:
            # a multiple of U need not be an integer below 2^16: the split itself, as the kernels make it
            assert bool(_splits(t).all()), f"{case['key']} {what}: a 3xbf16 operand is not hi + lo exactly"
        else:
            assert v < LIMIT_X3, f"{case['key']} {what}: 3xbf16 operand {v:.4g} >= 2^16"

    def low(t):
        return (~_is_bf16(t)).double()

    if split:
        # weights: the named layer's nonzeros carry a bf16 low part (fc_out row 0 excepted), are multiples of
        # U and split exactly; every other weight is a bf16 integer, like biases and codes
        for k, v in P.items():
            if k == split[0] + ".weight":
                body = v[1:] if split[0] == "fc_out" else v
                assert _integers(v, u) and bool(_splits(v).all()), k
                assert not bool(_is_bf16(body)[body != 0].any()), k
                assert bool(_is_bf16(v[:1]).all()) or split[0] != "fc_out", k
            else:
                assert bool(_is_bf16(v).all()) and _integers(v), k
    else:
        # weights: bf16 numbers (Wl = 0), integers like biases and codes
        for k, v in P.items():
            assert bool(_is_bf16(v).all()) and _integers(v), k
    assert _integers(case["zs"]) and _integers(case["zt"]) and _integers(case["d_raw"])
    x = ref["x"]
    xin = x
    if geo:
        # the only non-integer inputs are the sin / cos columns, and every weight on them is 0
        live = torch.zeros(90, dtype=torch.bool)
        live[0:3], live[63:66] = True, True
        assert _integers(x[:, live]) and bool(torch.isfinite(x).all())
        assert not bool(W("layer_xyz1")[:, 3:].any()) and not bool(W("layer_dir1")[:, HID + 3:].any())
        for k in ("ro", "rd", "z", "pts"):
            assert _integers(case[k]), k
        nrm = case["rd"].double().norm(dim=-1)
        assert bool(((nrm == 1) | (nrm == 2) | (nrm == 4)).all()) and bool(((case["rd"] != 0).sum(-1) == 1).all())
        sums("ro + rd z",
             case["ro"].abs().double()[:, None, :] + (case["rd"].abs()[:, None, :] * case["z"][..., None]).double())
        xin = x * live
    h1, h2, feat, v1, v2 = ref["planes"]
    code, acts = ref["code"], ref["acts"]
    zs, zt = case["zs"].double(), case["zt"].double()
    for t in list(ref["planes"]) + list(ref["pre"].values()) + [ref["raw"], ref["code_bias"]]:
        assert _integers(t, u)

    # forward: every accumulated output, sum of |terms| (any partial sum in any order is bounded by it)
    def lin(what, inp, w, b):
        sums(what, inp.abs() @ w.abs().t() + b.abs())
    lin("s1", zs, W("shape_code_layer1"), B("shape_code_layer1"))
    lin("s2", zs, W("shape_code_layer2"), B("shape_code_layer2"))
    lin("t1", zt, W("texture_code_layer1"), B("texture_code_layer1"))
    lin("c_xyz2", acts["s1"], W("layer_xyz2")[:, HID:], B("layer_xyz2"))
    lin("c_out", acts["s2"], W("fc_out")[:, HID:], B("fc_out"))
    lin("c_rgb", acts["t1"], W("fc_rgb")[:, HID:], B("fc_rgb"))
    cbr = ref["code_bias"][code].abs()
    lin("h1", xin[:, :63], W("layer_xyz1"), B("layer_xyz1"))
    sums("h2", h1.abs() @ W("layer_xyz2")[:, :HID].abs().t() + cbr[:, 0:256])
    sums("feat", h2.abs() @ W("fc_out")[1:, :HID].abs().t() + cbr[:, 256:512])
    sums("sigma", h2.abs() @ W("fc_out")[:1, :HID].abs().t() + cbr[:, 512:513])
    lin("v1", torch.cat((feat, xin[:, 63:]), dim=-1), W("layer_dir1"), B("layer_dir1"))
    lin("v2", v1, W("layer_dir2"), B("layer_dir2"))
    sums("rgb", v2.abs() @ W("fc_rgb")[:, :HID].abs().t() + cbr[:, 513:516])
    # forward: what a 3xbf16 product reads next to a (bf16) weight
    # (a split model's test is of the values themselves: of a geometry case's x only the raw-input columns,
    # the sin / cos columns meet zeros in both fragments of every weight)
    for what, t in (("x", x[:, live] if geo and split else x), ("h1", h1), ("h2", h2), ("feat", feat), ("v1", v1),
                    ("v2", v2), ("code_bias", ref["code_bias"])):
        x3(what, t)
    # forward, 3xbf16: Xl.Wl is dropped, so no term may pair an input's low part with a weight's
    layers = (("layer_xyz1", x[:, :63], W("layer_xyz1")), ("layer_xyz2", h1, W("layer_xyz2")[:, :HID]),
              ("fc_out", h2, W("fc_out")[:, :HID]),
              ("layer_dir1", torch.cat((feat, x[:, 63:]), dim=-1), W("layer_dir1")),
              ("layer_dir2", v1, W("layer_dir2")), ("fc_rgb", v2, W("fc_rgb")[:, :HID]))
    for name, inp, w in layers:
        x3("W " + name, w)
        both = low(inp) @ low(w).t()
        assert float(both.max()) == 0.0, f"{case['key']} {name}: a forward term with two bf16 low parts"

    if not backward:
        return top
    # backward: the masked layer gradients (3xbf16 operands), the dX sums, the dW sums over rows, g_code
    d = ref["dpre"]
    for k, t in d.items():
        assert _integers(t, u), k
        x3("d " + k, t)
    # dX, 3xbf16: dpre_l.Wl is dropped
    for name, g in (("layer_xyz1", d["h1"]), ("layer_xyz2", d["h2"]), ("fc_out", d["out"]), ("layer_dir1", d["v1"]),
                    ("layer_dir2", d["v2"]), ("fc_rgb", d["rgb"])):
        both = low(g) @ low(W(name))
        assert float(both.max()) == 0.0, f"{case['key']} dX {name}: a term with two bf16 low parts"
    sums("d v2", d["rgb"].abs() @ W("fc_rgb")[:, :HID].abs())
    sums("d v1", d["v2"].abs() @ W("layer_dir2").abs())
    sums("d feat|view", d["v1"].abs() @ W("layer_dir1").abs())
    sums("d h2", d["out"].abs() @ W("fc_out")[:, :HID].abs())
    sums("d h1", d["h2"].abs() @ W("layer_xyz2")[:, :HID].abs())
    sums("d x", d["h1"].abs() @ W("layer_xyz1").abs())
    dv = torch.cat((feat, xin[:, 63:]), dim=-1)
    gemms = (("layer_xyz1", d["h1"], xin[:, :63]), ("layer_xyz2", d["h2"], h1), ("fc_out", d["out"], h2),
             ("layer_dir1", d["v1"], dv), ("layer_dir2", d["v2"], v1), ("fc_rgb", d["rgb"], v2))
    for name, g, a in gemms:
        sums("dW " + name, g.abs().t() @ a.abs())
        sums("db " + name, g.abs().sum(0))
        # 3xbf16 dW: both operands are activations; Al.Bl is dropped, so no term may have two low parts
        both = (~_is_bf16(g)).double().t() @ (~_is_bf16(a)).double()
        assert float(both.max()) == 0.0, f"{case['key']} dW {name}: a term with two bf16 low parts"
    n = zs.shape[0]
    onehot = torch.zeros(case["m"], n, dtype=F64)
    onehot[torch.arange(case["m"]), code] = 1.0
    for k, g in (("h2", d["h2"]), ("out", d["out"]), ("rgb", d["rgb"])):
        sums("g_code " + k, onehot.t() @ g.abs())
    # the code backward: d s1 / s2 / t1, then dz and the outer products summed over the code rows
    gc = ref["g_code"].abs()
    sums("d s1", gc[:, 0:256] @ W("layer_xyz2")[:, HID:].abs())
    sums("d s2", torch.cat((gc[:, 512:513], gc[:, 256:512]), dim=-1) @ W("fc_out")[:, HID:].abs())
    sums("d t1", gc[:, 513:516] @ W("fc_rgb")[:, HID:].abs())
    sums("dz_s", d["s1"].abs() @ W("shape_code_layer1").abs() + d["s2"].abs() @ W("shape_code_layer2").abs())
    sums("dz_t", d["t1"].abs() @ W("texture_code_layer1").abs())
    for g, a in ((d["s1"], zs), (d["s2"], zs), (d["t1"], zt), (ref["g_code"][:, 0:256], acts["s1"]),
                 (ref["g_code"][:, 256:513], acts["s2"]), (ref["g_code"][:, 513:516], acts["t1"])):
        sums("code dW", g.abs().t() @ a.abs())
    compared = tuple(ref["grads"][k][..., exact_columns(k, geo) or slice(None)] for k in ref["grads"])
    for t in (ref["dz_s"], ref["dz_t"], ref["g_code"]) + compared:
        assert _integers(t, u)
    if geo:
        # d pts = d x[:, 0:3] (the sin / cos columns' gradients are 0 x finite); d ro = sum_s d pts,
        # d rd = sum_s d pts z + the Q1 rows' d vd / |rd| with the radial part removed
        dx = (d["h1"].abs() @ W("layer_xyz1").abs())[:, :3].reshape(case["r"], case["s"], 3)
        sums("d ro", dx.sum(1))
        dvd = (d["v1"].abs() @ W("layer_dir1").abs())[:, HID:HID + 3]
        q1 = torch.zeros(case["r"], 3, dtype=F64).index_add_(0, ref["dray"], dvd)
        # (in units of 1/4: the view-direction part is a multiple of 1 / |rd|, |rd| <= 4)
        sums("d rd", 4 * ((dx * case["z"].double()[..., None]).sum(1) * (case["mode"] == "rayz") + 2 * q1))
        for k in ("d_pts", "d_ro", "d_rd"):
            if k in ref:
                assert _integers(ref[k], u / 4), k     # multiples of unit / |rd|, |rd| <= 4
    else:
        assert _integers(ref["d_x"], u)
    return top


# ---------------------------------------------------------------------------------------------
# the three-product rule in float64, and what a wrong low fragment would change
# ---------------------------------------------------------------------------------------------

# per-sample GEMM layer -> (the plane it reads, the plane it writes, ReLU behind it)
_CHAIN = (("layer_xyz1", "x", "h1", True), ("layer_xyz2", "h1", "h2", True), ("fc_out", "h2", "feat", False),
          ("layer_dir1", "feat", "v1", True), ("layer_dir2", "v1", "v2", True), ("fc_rgb", "v2", "rgb", False))


def x3_weight(case, layer: str) -> torch.Tensor:
    """The block of ``layer``'s weight the field kernels' MFMAs read: the per-sample columns (the code halves
    go through the fp32 code bias), of fc_out the 256 feature rows (row 0 is an fp32 dot product)."""
    w = case["params"][layer + ".weight"].double()
    if layer in ("layer_xyz2", "fc_out", "fc_rgb"):
        w = w[:, :HID]
    return w[1:] if layer == "fc_out" else w


def _x3_product(inp, w, rule: str):
    """Wh.Xh + Wh.Xl + Wl.Xh with both operands split as the kernels split them; ``rule`` "drop" leaves the
    third product out, "lolo" forms Wl.Xl in its place."""
    xh, xl = split_bf16(inp)
    wh, wl = split_bf16(w)
    third = {"x3": xh @ wl.t(), "drop": 0.0, "lolo": xl @ wl.t()}[rule]
    return xh @ wh.t() + xl @ wh.t() + third


def _x3_tail(case, ref, layer: str, pre: torch.Tensor, rows) -> torch.Tensor:
    """raw (..., rows, 4) from ``layer``'s GEMM result ``pre`` (bias not yet added) on sample rows ``rows``,
    every later layer by the three-product rule."""
    P = case["params"]
    cb = ref["code_bias"][ref["code"]][rows]
    x = ref["x"][rows]
    started, h2 = False, ref["planes"][1][rows]
    for name, _, dst, relu in _CHAIN:
        if name == layer:
            started, t = True, pre
        elif started:
            t = _x3_product(t, x3_weight(case, name), "x3")
        else:
            continue
        if name == "layer_xyz2":
            t = t + cb[:, 0:256]
        elif name == "fc_out":
            t = t + cb[:, 256:512]
        elif name == "fc_rgb":
            t = t + cb[:, 513:516]
        else:
            t = t + P[name + ".bias"].double()
        if relu:
            t = torch.relu(t)
        if dst == "h2":
            h2 = t
        if dst == "feat":
            t = torch.cat((t, x[:, 63:].expand(t.shape[:-1] + (27,))), dim=-1)
    # sigma: fc_out row 0 as an fp32 dot product of the unsplit h2
    sigma = h2 @ P["fc_out.weight"].double()[0, :HID] + cb[:, 512]
    return torch.cat((t, sigma.expand(t.shape[:-1]).unsqueeze(-1)), dim=-1)


def _x3_input(ref, layer: str, rows) -> torch.Tensor:
    src = {name: s for name, s, _, _ in _CHAIN}[layer]
    if src == "x":
        return ref["x"][rows, :63]
    if src == "feat":
        return torch.cat((ref["planes"][2][rows], ref["x"][rows, 63:]), dim=-1)
    return ref["planes"][PLANES.index(src)][rows]


def x3_raw(case, layer: str = "layer_xyz1", rule: str = "x3") -> torch.Tensor:
    """raw (m, 4) of the case by the three-product rule in float64: ``layer`` by ``rule`` (see _x3_product),
    every layer behind it by the rule proper.  With layer_xyz1 and "x3": the whole network."""
    ref = reference(case)
    rows = slice(None)
    return _x3_tail(case, ref, layer, _x3_product(_x3_input(ref, layer, rows), x3_weight(case, layer), rule), rows)


def x3_swapped_lo(case, layer: str, axis: str, rows: int = 96) -> torch.Tensor:
    """For every pair of neighbouring output rows (``axis`` "rows": r, r + 1 of x3_weight) or input columns
    ("cols": c, c + 1) of ``layer``: does raw change, on some of the first ``rows`` sample rows, when the low
    parts of the pair's weights change places?  -> bool per pair.  Only the third product moves: with
    T = Xh Wl^T, swapped rows swap two columns of T, swapped columns add (Xh_c - Xh_c+1) (Wl_c+1 - Wl_c)^T."""
    ref = reference(case)
    rows = slice(0, min(rows, case["m"]))
    inp, w = _x3_input(ref, layer, rows), x3_weight(case, layer)
    base = _x3_product(inp, w, "x3")
    xh, _ = split_bf16(inp)
    _, wl = split_bf16(w)
    third = xh @ wl.t()
    if axis == "rows":
        n = w.shape[0] - 1
        pre = base.repeat(n, 1, 1)
        r = torch.arange(n)
        pre[r, :, r] += third[:, 1:].t() - third[:, :-1].t()
        pre[r, :, r + 1] += third[:, :-1].t() - third[:, 1:].t()
    else:
        n = w.shape[1] - 1
        pre = base + (xh[:, :-1] - xh[:, 1:]).t()[:, :, None] * (wl[:, 1:] - wl[:, :-1]).t()[:, None, :]
    want = _x3_tail(case, ref, layer, base, rows)
    got = _x3_tail(case, ref, layer, pre, rows)
    return (got != want).flatten(1).any(1)


def reach(case) -> dict:
    """What the case reaches: per ReLU layer the counts of pre-activations < 0, == 0, > 0; the share of rows
    with every raw channel nonzero."""
    ref = reference(case)
    out = {k: (int((v < 0).sum()), int((v == 0).sum()), int((v > 0).sum())) for k, v in ref["pre"].items()}
    out["raw_rows"] = float((ref["raw"] != 0).all(-1).double().mean())
    return out
