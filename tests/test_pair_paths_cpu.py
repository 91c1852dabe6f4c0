"""The float64 reference of tests/test_gpu_pair_paths.py against the float32 oracle, on the CPU: the
reference alone must sit well inside the bound the kernels are held to, or the bound would test the
reference's rounding instead of the step."""
import pytest
import torch

import pair_path_cases as C


@pytest.mark.parametrize("loss", C.LOSSES)
@pytest.mark.parametrize("nc,nf", C.SAMPLES)
def test_eval_reference_fp32_within_bound(nc, nf, loss):
    """The oracle's eval step in float32 (its own fine depths) against the same op sequence in float64 on
    those depths: loss to 1e-6, every gradient within half of the GPU test's bound (measured: at most
    4.9e-4 of the scale for the pose scalars, 2.8e-4 for the codes, over the nine cases)."""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    inp = C.eval_inputs(nc, nf)
    l32, g32, z_f = C.eval_reference(inp, nc, nf, loss, torch.float32)
    l64, g64, _ = C.eval_reference(inp, nc, nf, loss, torch.float64, z_fine=z_f)
    assert z_f.shape == (C.N_RAYS, nc + nf)
    err = C.relative_errors(g32, g64)
    print("PAIR_PATH_REFERENCE", (nc, nf), loss, {k: float(f"{v:.3e}") for k, v in err.items()})
    assert abs(l32 - l64) <= 1e-6 * max(1.0, abs(l64))
    for k, e in err.items():
        assert e <= C.RTOL / 2, (k, e)
    # the gradient a dropped field would take with it is far above the bound: the loss's other half
    if loss == "both":
        _, g_fine, _ = C.eval_reference(inp, nc, nf, "fine", torch.float64, z_fine=z_f)
        dropped = C.relative_errors(g_fine, g64)
        assert max(dropped[k] for k in ("theta", "phi", "rho")) > 5 * C.RTOL, dropped


def test_code_grads_pair_adds_both_fields_dz(monkeypatch):
    """autograd._code_grads_pair returns the code rows' gradient its sinks did not take: with no sink to
    defer to, BOTH fields' dz, summed (both read the same code rows) -- the first field's is not
    overwritten by the second's.  The two launches are stubbed: this is the host's bookkeeping."""
    from types import SimpleNamespace as NS
    from codenerf import autograd as A, ops
    monkeypatch.setattr(ops, "code_ds_outer_multi", lambda items, z_s, z_t: ["ws0", "ws1"])
    dz = {"ws0": (torch.full((1, 4), 1.0), torch.full((1, 4), 10.0)),
          "ws1": (torch.full((1, 4), 2.0), torch.full((1, 4), 20.0))}
    monkeypatch.setattr(ops, "code_dz", lambda jobs, n: dz[jobs[0][2]])
    z = torch.zeros(1, 4)
    taken = []
    sink = NS(defer=lambda params, g_code, ws: taken.append(ws) or True)

    def item(meta, want_z=True):
        return (meta, "params", z, z, "g_code", None, want_z, "act")
    out = A._code_grads_pair(item(NS(sink=None)), item(NS(sink=None)))
    assert torch.equal(out[0], torch.full((1, 4), 3.0)) and torch.equal(out[1], torch.full((1, 4), 30.0))
    out = A._code_grads_pair(item(NS(sink=None)), item(NS(sink=sink)))      # the second deferred: the first's
    assert taken == ["ws1"] and torch.equal(out[0], dz["ws0"][0]) and torch.equal(out[1], dz["ws0"][1])
    assert A._code_grads_pair(item(NS(sink=sink)), item(NS(sink=sink))) == (None, None)
    assert A._code_grads_pair(item(NS(sink=None), False), item(NS(sink=None), False)) == (None, None)
