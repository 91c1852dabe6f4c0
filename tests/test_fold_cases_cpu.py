"""The fold of fc_out's feature rows into layer_dir1 (CN_FMT_F32_W16_FOLD), proven on the CPU for the
integer-exact probes of tests/exact_cases.py: on every forward case the GPU file runs, W_f and c_v1 are
integers, the folded pre-activation equals the float64 reference's pre["v1"] exactly, and every sum of
|terms| the folded kernel, its pack and its bias launch accumulate stays below 2^24 -- so the folded
kernel, like every other fp32 kernel, must return the reference bit for bit
(tests/test_gpu_field_fold.py)."""
import pytest
import torch

import exact_cases as E

HID = E.HID


def fold_cases(cu_count: int = 256):
    """Every forward case of exact_cases (the persistent one at ``cu_count`` CUs), once each."""
    seen = {}
    for c in (E.encoded_forward_cases() + E.dense_forward_cases() + E.geometry_forward_cases()
              + [E.encoded_case(0, E.persistent_rows(cu_count), "index")]):
        seen[c["key"]] = c
    return list(seen.values())


CASES = fold_cases()
IDS = ["-".join(str(k) for k in c["key"]) for c in CASES]


def fold_terms(case):
    """W_f (256, 256), c_v1 (n_codes, 256) in float64, and the sums of |terms| behind them."""
    ref = E.reference(case)
    wd1 = case["params"]["layer_dir1.weight"].double()
    wo = case["params"]["fc_out.weight"].double()
    bd1 = case["params"]["layer_dir1.bias"].double()
    a, b = wd1[:, :HID], wo[1:, :HID]
    c_feat = ref["code_bias"][:, 256:512]
    return dict(w_f=a @ b, w_f_sum=a.abs() @ b.abs(), c_v1=c_feat @ a.t() + bd1,
                c_v1_sum=c_feat.abs() @ a.abs().t() + bd1.abs(), w_view=wd1[:, HID:])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fold_is_exact(case):
    ref, t = E.reference(case), fold_terms(case)
    assert E._integers(t["w_f"]) and E._integers(t["c_v1"])
    h2, view, code = ref["planes"][1], ref["x"][:, 63:], ref["code"]
    v1_pre = h2 @ t["w_f"].t() + view @ t["w_view"].t() + t["c_v1"][code]
    assert torch.equal(v1_pre, ref["pre"]["v1"])
    # the sums of |terms|: W_f's dot products, c_v1's, the folded layer's (a geometry model's weights on
    # the sin / cos columns are 0, so those columns add nothing: exact_cases.check_exact)
    live = view
    if case["geometry"]:
        live = view.clone()
        live[:, 3:] = 0.0
    layer = h2.abs() @ t["w_f"].abs().t() + live.abs() @ t["w_view"].abs().t() + t["c_v1"][code].abs()
    top = max(float(t["w_f_sum"].max()), float(t["c_v1_sum"].max()), float(layer.max()))
    print(f"{case['key']}: largest sum of |terms| {top:.0f}")
    assert top < E.LIMIT_SUM


def test_case_list_matches_exact_cases():
    """The list is every forward case: the model set, the dense models, every size and layout, every
    geometry shape in both modes, the persistent case."""
    keys = {c["key"] for c in CASES}
    assert len(keys) == len(CASES) >= E.N_MODELS + len(E.DENSE_MODELS) + 3 * len(E.ENCODED_SIZES) + 2 * len(E.GEOMETRY_SHAPES)
    assert ("enc", 0, E.persistent_rows(256), "index") in keys
