"""The integer-exact probes of tests/exact_cases.py, proven on the CPU: every case the GPU file runs
meets the derived exactness conditions, the fp32 oracle returns the float64 reference bit for bit (the
proof that the inputs are exact, taken on the reference and not on the kernels), the model set covers
every row and column of every weight matrix, and every case reaches the ties and ragged chunks it is
built for.  For the split models (a bf16 low part in one layer's weights): the conditions in units of 2^-8,
the cover of every row and column by a low-part weight, and, with a float64 emulation of the three-product
rule, that a dropped, misread or misplaced low fragment changes raw."""
import numpy as np
import pytest
import torch

import exact_cases as E
from codenerf import synthetic

CASES = E.all_cases()
IDS = ["-".join(str(k) for k in c["key"]) for c in CASES]
BACKWARD = {c["key"] for c in E.backward_cases()}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_exact(case):
    """check_exact's conditions hold, with room: they are limits on the inputs, not measurements of a kernel."""
    top = E.check_exact(case, backward=case["key"] in BACKWARD)
    assert top["sum"] < E.LIMIT_SUM and top["x3"] < E.LIMIT_X3


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_equals_reference_bitwise(case):
    """O.codenerf_mlp / O.forward_pass in fp32 (aten's own summation order, the oracle's ``repeat`` form of
    Q1, codes expanded per row) == the float64 reference cast to fp32, every bit."""
    ref = E.reference(case)
    got = E.oracle_raw(case)
    assert got.dtype == torch.float32
    assert torch.equal(got, ref["raw"].float()) and torch.equal(got.double(), ref["raw"])


def test_reference_gradients_match_oracle_autograd():
    """The reference's gradients are those of the oracle: fp32 autograd over O.codenerf_mlp on an encoded
    case gives the same bits (codes per row summed back onto their rows)."""
    case = E.encoded_case(2, 257, "index")
    ref = E.reference(case)
    p = {k: v.clone().requires_grad_(True) for k, v in case["params"].items()}
    zs, zt, x = [case[k].clone().requires_grad_(True) for k in ("zs", "zt", "x")]
    code = ref["code"]
    from oracle import codenerf_oracle as O
    (O.codenerf_mlp(p, zs[code], zt[code], x, 63) * case["d_raw"]).sum().backward()
    for k in p:
        assert torch.equal(p[k].grad.double(), ref["grads"][k]), k
    assert torch.equal(zs.grad.double(), ref["dz_s"]) and torch.equal(zt.grad.double(), ref["dz_t"])
    assert torch.equal(x.grad.double(), ref["d_x"])


@pytest.mark.parametrize("geometry", [False, True])
def test_model_set_covers_every_row_and_column(geometry):
    """Over the model set every row and every (allowed) column of every weight matrix is nonzero in some
    model, no two columns of a layer are equal across the set, and every weight is in +-{1, 2, 3}."""
    models = E.model_set(geometry)
    for name, (o, i) in synthetic.layer_shapes().items():
        ws = np.stack([m[name + ".weight"].numpy() for m in models])          # (models, o, i)
        assert set(np.unique(ws)) <= {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
        cols = E.allowed_columns(name, i, geometry)
        assert bool((ws != 0).any(axis=(0, 2)).all()), f"{name}: a row is zero in every model"
        assert bool((ws != 0).any(axis=(0, 1))[cols].all()), f"{name}: a column is zero in every model"
        rest = np.setdiff1d(np.arange(i), cols)
        assert not ws[:, :, rest].any(), f"{name}: a weight on a sin / cos column"
        stacked = ws.reshape(-1, i)[:, cols]
        assert np.unique(stacked, axis=1).shape[1] == len(cols), f"{name}: two equal columns"


@pytest.mark.parametrize("model", E.DENSE_MODELS)
def test_dense_models_fill_their_layer(model):
    """Every entry of the dense layer is nonzero, and an entry differs from its neighbour in the next row and
    in the next column on most positions (5 in 6 for independent draws from six values): what shows one
    element moved by one."""
    w = E.probe_model(model)[model[len("dense:"):] + ".weight"]
    assert bool((w != 0).all())
    assert float((w[1:] != w[:-1]).double().mean()) > 0.75 and float((w[:, 1:] != w[:, :-1]).double().mean()) > 0.75


SPLIT_CASES = E.split_encoded_cases() + E.split_geometry_cases()
SPLIT_IDS = ["-".join(str(k) for k in c["key"]) for c in SPLIT_CASES]


@pytest.mark.parametrize("geometry", [False, True])
@pytest.mark.parametrize("layer", E.SPLIT_LAYERS)
def test_split_set_covers_every_row_and_column(layer, geometry):
    """Over a layer's split set every row (fc_out's sigma row excepted: it must be a bf16 row) and every allowed
    column holds a weight with a bf16 low part; every nonzero of the layer has one, and every weight of the
    other layers is a bf16 integer."""
    models = [E.probe_model(name, geometry) for name in E.split_set(layer)]
    assert len(models) == E.SPLIT_COUNT[layer]
    ws = torch.stack([m[layer + ".weight"] for m in models])
    lowp = ~E._is_bf16(ws)
    body = slice(1, None) if layer == "fc_out" else slice(None)
    assert bool(lowp[:, body].any(2).any(0).all()), "a row has no low-part weight in any model"
    cols = E.allowed_columns(layer, ws.shape[2], geometry)
    assert bool(lowp.any(1).any(0)[cols].all()), "an allowed column has no low-part weight in any model"
    assert bool((lowp == (ws != 0))[:, body].all()), "a nonzero weight of the split layer is a bf16 number"
    rest = np.setdiff1d(np.arange(ws.shape[2]), cols)
    assert not bool(ws[:, :, rest].any())
    if layer == "fc_out":
        assert not bool(lowp[:, 0].any()) and bool(ws[:, 0].any())
    for m in models:
        for k, v in m.items():
            if k != layer + ".weight":
                assert bool(E._is_bf16(v).all()) and bool((v == v.round()).all()), k
        # nine or ten significant bits, multiples of 2^-8, and an exact hi + lo
        w = m[layer + ".weight"].double()
        assert bool((w / E.U == (w / E.U).round()).all()) and float(w.abs().max()) < 4
        hi, lo = E.split_bf16(w)
        assert bool((hi + lo == w).all())


def test_case_unit():
    assert E.case_unit(E.encoded_case(0, 257, "index")) == 1.0 and E.case_unit(SPLIT_CASES[0]) == 2.0 ** -8


@pytest.mark.parametrize("case", SPLIT_CASES, ids=SPLIT_IDS)
def test_split_cases_move_every_raw_channel(case):
    """Every raw channel is nonzero on at least a quarter of the rows (a condition on the inputs), and the
    split layer's low parts reach raw: some raw value is no integer."""
    raw = E.reference(case)["raw"]
    assert float((raw != 0).double().mean(0).min()) >= 0.25
    assert bool((raw != raw.round()).any())


@pytest.mark.parametrize("case", SPLIT_CASES, ids=SPLIT_IDS)
def test_three_product_rule_equals_reference(case):
    """The float64 emulation of the kernels' rule (both operands split, Wh.Xh + Wh.Xl + Wl.Xh per layer, sigma
    as a plain dot product) returns the reference exactly: nothing the rule drops is nonzero."""
    assert torch.equal(E.x3_raw(case), E.reference(case)["raw"])


@pytest.mark.parametrize("case", SPLIT_CASES, ids=SPLIT_IDS)
def test_dropped_or_misread_low_product_shows(case):
    """Sensitivity: with the split layer's Wl.Xh dropped raw changes on at least a quarter of the rows, and
    with Wl.Xl in its place on the same rows (Xl is no copy of Xh anywhere it matters)."""
    layer = E.split_name(case["key"][1])[0]
    want = E.reference(case)["raw"]
    dropped = (E.x3_raw(case, layer, "drop") != want).any(-1)
    assert float(dropped.double().mean()) >= 0.25, float(dropped.double().mean())
    lolo = (E.x3_raw(case, layer, "lolo") != want).any(-1)
    assert torch.equal(lolo, dropped)


@pytest.mark.parametrize("axis", ["rows", "cols"])
@pytest.mark.parametrize("layer", E.SPLIT_LAYERS)
def test_swapped_low_parts_show(layer, axis):
    """Sensitivity: the low parts of two neighbouring output rows, or of two neighbouring input columns, of the
    split layer's MFMA block changing places changes raw on some row of the encoded case of some model of the
    layer's set -- for EVERY such pair."""
    seen = None
    for name in E.split_set(layer):
        hit = E.x3_swapped_lo(E.encoded_case(name, 257, "index"), layer, axis)
        seen = hit if seen is None else seen | hit
    w = E.x3_weight(E.encoded_case(E.split_set(layer)[0], 257, "index"), layer)
    assert seen.shape[0] == w.shape[0 if axis == "rows" else 1] - 1
    assert bool(seen.all()), f"pairs not seen: {(~seen).nonzero().flatten().tolist()}"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_reaches_ties_and_signal(case):
    """Pre-activations exactly 0 and on both sides of it in h1, h2, v1, v2 and the three code layers (cases
    of fewer than 31 rows: h1, h2 and the code layers; one row's 256 v1 / v2 values need not hold a 0), raw
    nonzero on most rows."""
    got = E.reach(case)
    layers = E.RELU_LAYERS + E.CODE_LAYERS if case["m"] >= 31 else ("h1", "h2") + E.CODE_LAYERS
    for k in layers:
        neg, zero, pos = got[k]
        assert neg > 0 and zero > 0 and pos > 0, (case["key"], k, got[k])
    assert got["raw_rows"] > 0.5, (case["key"], got["raw_rows"])


def test_ties_give_zero_gradient():
    """At a tie the reference's masked gradient is 0 (torch's ReLU backward: grad * (out > 0)), and some tie
    had a nonzero gradient arriving, so a kernel that let ties through would differ."""
    case = E.encoded_case(2, 257, "index")
    ref = E.reference(case)
    for k in E.RELU_LAYERS:
        tie = ref["pre"][k] == 0
        assert bool(tie.any()) and not bool(ref["dpre"][k][tie].any()), k
    # the gradient arriving at v2's ties: d rgb @ W_rgb[:, :256]
    arriving = ref["dpre"]["rgb"] @ case["params"]["fc_rgb.weight"].double()[:, :256]
    assert bool(arriving[ref["pre"]["v2"] == 0].any())


@pytest.mark.parametrize("r,s,chunk", E.GEOMETRY_SHAPES)
def test_q1_shapes_are_ragged(r, s, chunk):
    """Every Q1 shape has a short last chunk or a chunk that is not a multiple of the 128-sample tile."""
    assert r % chunk != 0 or (min(chunk, r) * s) % 128 != 0


def test_q1_and_codes_are_not_periodic():
    """Directions and codes are drawn per ray: in the 37-ray case the Q1 ray of a row differs from its own ray
    on most rows, those rays' directions differ, and neighbouring rows sit on different code rows."""
    case = E.geometry_case(0, "rayz", 37, 8, 10, "index")
    code, dray = E.row_maps(case)
    own = torch.arange(case["m"]) // case["s"]
    moved = dray != own
    assert float(moved.double().mean()) > 0.5
    assert float((case["rd"][dray] != case["rd"][own]).any(-1)[moved].double().mean()) > 0.5
    enc = E.encoded_case(0, 129, "index")
    c, _ = E.row_maps(enc)
    assert float((c[1:] != c[:-1]).double().mean()) > 0.5 and len(set(c.tolist())) == E.N_CODES


def test_persistent_case_takes_second_tiles():
    m = E.persistent_rows(256)
    assert m % 128 != 0 and m // 128 >= 256 + 3
