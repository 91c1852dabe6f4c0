"""The fp16 field kernel's rule (include/codenerf.h, CN_FMT_F16) in float64, and what makes it a bitwise
yardstick on the integer probes of tests/exact_cases.py.

The rule.  The six GEMM weight matrices -- layer_xyz1, layer_xyz2[:, :256], fc_out[1:, :256], layer_dir1,
layer_dir2, fc_rgb[:, :256] -- are rounded to fp16 (round to nearest even) once.  Every vector an MFMA reads
-- the 63 position encodings, h1, h2, feat, the 27 view encodings, v1, v2 -- is rounded to fp16 (RNE; beyond
the range: +-inf) where it is read.  Everything else is unrounded: the encodings' arithmetic, every bias, the
per-code terms (cn_code_bias rows, stride 520) and the accumulation.  sigma_raw is the dot product of
fc_out[0, :256] (fp32, unrounded) with the unrounded h2 plus its per-code term.  ReLU is max(x, 0) with a NaN
giving 0 (v_max_f32; torch.fmax).

Bitwise on the probes.  With small-integer weights and inputs every operand is an integer; an integer rounds
to an fp16 integer, the product of two fp16 numbers is exact in fp32, and while the sum of the terms'
magnitudes stays below 2^24 fp32 holds every partial sum exactly in ANY order.  So the device must return
rule()'s bits if no operand rounds to inf -- check() asserts those conditions on the float64 rule alone and
counts what the cases pin: operands that are no fp16 numbers, exact ties that round-half-away would take the
other way, and values RNE rounds up where truncation rounds down.

Everything here is CPU torch / numpy; results are cached per case and must not be modified."""
import numpy as np
import torch

import exact_cases as E

F64 = torch.float64
HID = 256
LIMIT_SUM = float(2 ** 24)
F16_MAX = 65504.0


def f16(t: torch.Tensor) -> torch.Tensor:
    """t rounded to fp16, round to nearest even, beyond the range +-inf (through fp32, as the device holds it)."""
    return t.float().half().double()


def relu(t: torch.Tensor) -> torch.Tensor:
    return torch.fmax(t, torch.zeros((), dtype=t.dtype))


def _mm(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """a @ w.T with IEEE products on rows that hold a non-finite value (inf x 0 = NaN, whatever the GEMM
    library does with zeros)."""
    out = a @ w.t()
    bad = ~torch.isfinite(a).all(-1)
    if bool(bad.any()):
        out[bad] = (a[bad][:, None, :] * w[None, :, :]).sum(-1)
    return out


def forward(params, x, cb, code, rounding=f16, trace=None) -> torch.Tensor:
    """The rule on encoded rows.  params: a CodeNeRFModel state dict; x (m, 90) the encodings; cb (n, 520) the
    cn_code_bias rows; code (m,) the code row of every sample -> raw (m, 4) [rgb, sigma_raw], float64.
    ``rounding``: what stands for the fp16 rounding of weights and operands (identity: the unrounded model).
    ``trace`` (a dict): gets "operands", (input width or 0, values) of the vectors the MFMAs read before their
    rounding and of the weight matrices, and "sums", each accumulator's sum of |terms|."""
    P = {k: v.double() for k, v in params.items()}
    x, cb = x.double(), cb.double()
    r = rounding
    ops, sums = [], []

    def gemm(inp, w, bias):
        a, wr = r(inp), r(w)
        ops.extend(((inp.shape[-1], inp), (0, w)))      # (input width or 0 for a weight matrix, values)
        sums.append(a.abs() @ wr.abs().t() + bias.abs())
        return _mm(a, wr) + bias

    W = lambda n: P[n + ".weight"]   # noqa: E731
    B = lambda n: P[n + ".bias"]     # noqa: E731
    c = cb[code]
    h1 = relu(gemm(x[:, :63], W("layer_xyz1"), B("layer_xyz1")))
    h2 = relu(gemm(h1, W("layer_xyz2")[:, :HID], c[:, 0:256]))
    feat = gemm(h2, W("fc_out")[1:, :HID], c[:, 256:512])
    w0 = W("fc_out")[:1, :HID]
    sigma = _mm(h2, w0) + c[:, 512:513]
    sums.append(h2.abs() @ w0.abs().t() + c[:, 512:513].abs())
    v1 = relu(gemm(torch.cat((feat, x[:, 63:]), dim=-1), W("layer_dir1"), B("layer_dir1")))
    v2 = relu(gemm(v1, W("layer_dir2"), B("layer_dir2")))
    rgb = gemm(v2, W("fc_rgb")[:, :HID], c[:, 513:516])
    if trace is not None:
        trace["operands"], trace["sums"] = ops, sums
    return torch.cat((rgb, sigma), dim=-1)


def unrounded(params, x, cb, code) -> torch.Tensor:
    """The same network with no rounding at all: the float64 model the rule departs from."""
    return forward(params, x, cb, code, rounding=lambda t: t)


_RULES = {}


def rule(case) -> torch.Tensor:
    """The rule's raw (m, 4) on a case of tests/exact_cases.py (its encodings, code rows and code terms are
    the float64 reference's: exact there)."""
    key = case["key"]
    if key not in _RULES:
        ref = E.reference(case)
        _RULES[key] = forward(case["params"], ref["x"], ref["code_bias"], ref["code"])
    return _RULES[key]


def rounding_counts(v: torch.Tensor) -> dict:
    """Of the operand values v: how many are no fp16 numbers; of those, how many are exact ties that RNE takes
    towards zero (round-half-away would take the other neighbour) and how many RNE rounds up in magnitude
    (truncation rounds down)."""
    a = v.reshape(-1).abs().numpy()
    a = a[a <= F16_MAX]
    r = a.astype(np.float32).astype(np.float16)
    rd = r.astype(np.float64)
    off = rd != a
    down = np.where(rd > a, np.nextafter(r, np.float16(0)), r)
    up = np.nextafter(down, np.float16(np.inf)).astype(np.float64)
    down = down.astype(np.float64)
    tie = off & ((a - down) == (up - a))
    return dict(n=int(a.size), not_f16=int(off.sum()), ties_to_zero=int((tie & (rd < a)).sum()),
                up_not_truncated=int((off & (rd > a)).sum()))


def check(case) -> dict:
    """Assert on the float64 rule alone the conditions of the module docstring; -> the largest operand and
    magnitude sum seen and rounding_counts() over every operand."""
    ref = E.reference(case)
    trace = {}
    raw = forward(case["params"], ref["x"], ref["code_bias"], ref["code"], trace=trace)
    live = None
    if case["geometry"]:
        # sin / cos columns are no integers, and every weight on them is 0 (exact_cases.check_exact)
        live = torch.zeros(90, dtype=torch.bool)
        live[0:3], live[63:66] = True, True
    assert bool((raw == raw.round()).all()) and bool(torch.isfinite(raw).all()), case["key"]
    top = dict(operand=0.0, sum=0.0, n=0, not_f16=0, ties_to_zero=0, up_not_truncated=0)
    for width, v in trace["operands"]:
        if live is not None and width in (63, 256 + 27):
            keep = live[:63] if width == 63 else torch.cat((torch.ones(256, dtype=torch.bool), live[63:]))
            assert bool(torch.isfinite(v).all())
            v = v[:, keep]
        assert bool((v == v.round()).all()), case["key"]
        big = float(v.abs().max())
        assert big <= F16_MAX, f"{case['key']}: operand {big} rounds to inf"
        top["operand"] = max(top["operand"], big)
        for k, n in rounding_counts(v).items():
            top[k] += n
    for s in trace["sums"]:
        if live is not None:
            s = torch.nan_to_num(s)      # |sin| x 0: finite
        big = float(s.abs().max())
        assert big < LIMIT_SUM, f"{case['key']}: sum of |terms| {big:.4g} >= 2^24"
        top["sum"] = max(top["sum"], big)
    return top


def probe_cases():
    """The 56 forward probes: encoded sizes x code layouts, the model set, a dense model per layer, geometry."""
    return E.encoded_forward_cases() + E.dense_forward_cases() + E.geometry_forward_cases()


def second_tile_case(cu_count: int):
    """One row more than exact_cases.persistent_rows: every persistent workgroup loops to a second tile."""
    return E.encoded_case(0, E.persistent_rows(cu_count) + 1, "index")


# ---------------------------------------------------------------------------------------------
# random weights: the inputs the GPU tests compare on
# ---------------------------------------------------------------------------------------------


def random_inputs(seed: int, m: int = 4096, n_codes: int = 5):
    """m random points in [-1, 1]^3, directions (not normalised), n_codes code rows and a code index."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(m, 1, 3, generator=g) * 2 - 1
    rd = torch.randn(m, 3, generator=g)
    zs = torch.randn(n_codes, 256, generator=g) * 0.5
    zt = torch.randn(n_codes, 256, generator=g) * 0.5
    ci = torch.randint(0, n_codes, (m,), generator=g)
    return pts, rd, zs, zt, ci


def encode(pts, rd) -> torch.Tensor:
    """(m, 90) encodings in float64 of fp32 points (m, 1, 3) and the fp32-normalised directions (one sample
    per ray, chunk_rows = m: each row takes its own ray's direction)."""
    from oracle import codenerf_oracle as O
    emb = O.EmbedCfg()
    vd = (rd / rd.norm(p=2, dim=-1).unsqueeze(-1)).double()
    return torch.cat((O.posenc(pts.reshape(-1, 3).double(), emb.fx.double(), True),
                      O.posenc(vd, emb.fd.double(), True)), dim=-1)
