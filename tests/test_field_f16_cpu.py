"""The fp16 rule reference (tests/field_f16_cases.py) is a valid bitwise yardstick for the fp16 field kernel
on the integer probes, and the probes pin the rounding: proven here on the CPU, on the float64 rule alone.

Per case field_f16_cases.check asserts that every result is an integer, no operand rounds to inf and every
accumulator's sum of |terms| stays below 2^24 (so fp32 accumulation is exact in any order and the device has
one right answer).  Over all cases: some operands are no fp16 numbers, some are exact ties that
round-half-away would round the other way, some round up where truncation rounds down -- a kernel that
converts with another rounding differs in bits -- and the rule's raw differs from the unrounded reference's on
most cases, so an fp32 kernel does not pass either."""
import pytest
import torch

import exact_cases as E
import field_f16_cases as H

CASES = H.probe_cases()


@pytest.fixture(scope="module")
def tops():
    return [H.check(c) for c in CASES]


def test_case_count():
    assert len(CASES) == 56 and len({c["key"] for c in CASES}) == 56


def test_rule_is_exact_on_every_probe(tops):
    """check() asserted integers, no inf and the 2^24 bound per case; the record over all of them."""
    operand = max(t["operand"] for t in tops)
    total = max(t["sum"] for t in tops)
    print(f"max |operand| {operand:.0f}, max magnitude sum {total:.0f}")
    assert 0 < operand <= H.F16_MAX and 0 < total < H.LIMIT_SUM


def test_probes_pin_the_rounding(tops):
    n = sum(t["n"] for t in tops)
    counts = {k: sum(t[k] for t in tops) for k in ("not_f16", "ties_to_zero", "up_not_truncated")}
    print(f"{n} operands: {counts}")
    assert counts["not_f16"] > 0            # the rounding happens at all
    assert counts["ties_to_zero"] > 0       # round-half-away would differ
    assert counts["up_not_truncated"] > 0   # truncation (cvt_pkrtz) would differ


def test_rule_differs_from_the_unrounded_reference():
    differ = sum(not torch.equal(H.rule(c), E.reference(c)["raw"]) for c in CASES)
    print(f"rule != reference on {differ} of {len(CASES)} cases")
    assert differ > len(CASES) // 2


def test_identity_rounding_is_the_reference():
    """The rule's network with no rounding is exact_cases.reference's: the rule changes the rounding alone."""
    for c in (CASES[0], CASES[-1]):
        ref = E.reference(c)
        assert torch.equal(H.unrounded(c["params"], ref["x"], ref["code_bias"], ref["code"]), ref["raw"])


def test_second_tile_case_is_exact():
    """The extra GPU case (one row past exact_cases.persistent_rows, at 256 CUs) meets the same conditions."""
    top = H.check(H.second_tile_case(256))
    assert top["not_f16"] > 0


def test_non_finite_rows_follow_ieee():
    """The edge case of the GPU tests: |x| = 1e5 rounds to inf, inf x 0 is NaN, and ReLU takes a NaN to 0."""
    c = E.encoded_case("dense:layer_xyz1", 33, "one")
    ref = E.reference(c)
    x = ref["x"].clone()
    x[7, 5] = 1e5
    raw = H.forward(c["params"], x, ref["code_bias"], ref["code"])
    keep = torch.ones(33, dtype=torch.bool)
    keep[7] = False
    assert torch.equal(raw[keep], H.rule(c)[keep])
    assert float(H.relu(torch.tensor([float("nan"), -1.0, 2.0], dtype=torch.float64)).sum()) == 2.0
