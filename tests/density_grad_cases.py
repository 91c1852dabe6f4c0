"""The density's gradient stated in float64, and the rules built on it, for the density-gradient kernel's
tests: everything here is CPU torch / numpy.

d sigma_raw / d p of CodeNeRFModel.forward's density (model.py:174-186) two ways -- autograd through the
oracle's model in double, and the explicit chain the kernel runs (ReLU masks, W_out[0], W_xyz2^T, W_xyz1^T,
the encoding's derivative) -- plus the normals rule, the activated scaling, the "normal_fine" composition
and readers for the mesh files' vertex attributes.  References are computed once per test module and
must not be modified.
"""
import numpy as np
import torch

from oracle import codenerf_oracle as O

F64 = torch.float64
DIM_XYZ, DIM_DIR, HID = 63, 27, 256


def _double(params):
    return {k: v.detach().cpu().to(F64) for k, v in params.items()}


def _rows(z_s, n):
    z = z_s.detach().cpu().to(F64)
    return z.expand(n, -1) if z.shape[0] == 1 else z


def sigma_autograd(params, z_s, pts):
    """(d sigma_raw / d pts (N, 3), sigma_raw (N,)) in float64 by autograd through the oracle's
    CodeNeRFModel.forward (O.posenc + O.codenerf_mlp in double; the view direction and the texture code
    do not reach sigma_raw and are zeros).  ``z_s``: (1, 256) or (N, 256).  A non-finite point gives NaN."""
    p = _double(params)
    x = pts.detach().cpu().to(F64).reshape(-1, 3).clone().requires_grad_(True)
    n = x.shape[0]
    zs = _rows(z_s, n)
    enc = O.posenc(x, O.frequency_bands(10, True).to(F64), True)
    rows = torch.cat((enc, torch.zeros(n, DIM_DIR, dtype=F64)), dim=-1)
    raw = O.codenerf_mlp(p, zs, torch.zeros_like(zs), rows, DIM_XYZ)
    sigma = raw[:, 3]
    grad, = torch.autograd.grad(sigma.sum(), x)
    return grad.detach(), sigma.detach()


def sigma_chain(params, z_s, pts):
    """The same two values as the explicit chain, without autograd:
    g_h2 = W_out[0, :256] . [pre_h2 > 0]; g_h1 = (W_xyz2[:, :256]^T g_h2) . [pre_h1 > 0];
    g_enc = W_xyz1^T g_h1; d/dx_d = g_enc[d] + sum_k f_k (g_enc[sin k d] cos(f_k x_d) - g_enc[cos k d] sin(f_k x_d))."""
    p = _double(params)
    x = pts.detach().cpu().to(F64).reshape(-1, 3)
    n = x.shape[0]
    zs = _rows(z_s, n)
    relu = torch.relu
    freqs = O.frequency_bands(10, True).to(F64)
    enc = O.posenc(x, freqs, True)
    zs1 = relu(zs @ p["shape_code_layer1.weight"].T + p["shape_code_layer1.bias"])
    zs2 = relu(zs @ p["shape_code_layer2.weight"].T + p["shape_code_layer2.bias"])
    pre1 = enc @ p["layer_xyz1.weight"].T + p["layer_xyz1.bias"]
    h1 = relu(pre1)
    pre2 = torch.cat((h1, zs1), dim=-1) @ p["layer_xyz2.weight"].T + p["layer_xyz2.bias"]
    h2 = relu(pre2)
    sigma = torch.cat((h2, zs2), dim=-1) @ p["fc_out.weight"][0] + p["fc_out.bias"][0]
    g_h2 = p["fc_out.weight"][0, :HID] * (pre2 > 0).to(F64)
    g_h1 = (g_h2 @ p["layer_xyz2.weight"][:, :HID]) * (pre1 > 0).to(F64)
    g_enc = g_h1 @ p["layer_xyz1.weight"]
    grad = g_enc[:, :3].clone()
    for k, f in enumerate(freqs):
        s, c = g_enc[:, 3 + 6 * k:6 + 6 * k], g_enc[:, 6 + 6 * k:9 + 6 * k]
        grad = grad + f * (s * torch.cos(x * f) - c * torch.sin(x * f))
    return grad, sigma


def normals_rule(g):
    """n = -g / |g| per row of g (N, 3) in numpy: exactly 0 where |g| is 0, NaN where g is not finite."""
    g = np.asarray(g)
    out = np.empty_like(g)
    for i, row in enumerate(g):
        if not np.all(np.isfinite(row)):
            out[i] = np.nan
        elif not np.any(row != 0):
            out[i] = 0.0
        else:
            out[i] = -row / np.sqrt(np.sum(row.astype(np.float64) ** 2)).astype(g.dtype)
    return out


def composite_rule(weights, n):
    """sum_s w_s n_s per ray in numpy loops, a sample of weight exactly 0 skipped whatever its normal."""
    w, n = np.asarray(weights), np.asarray(n)
    out = np.zeros((w.shape[0], 3), dtype=n.dtype)
    for r in range(w.shape[0]):
        for s in range(w.shape[1]):
            if w[r, s] != 0:
                out[r] += w[r, s] * n[r, s]
    return out


# ---------------------------------------------------------------- mesh files


def read_ply(path):
    """-> (header property names of the vertex element, structured vertex rows, faces (T, 3) int32)."""
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = nf = 0
    props, element = [], None
    for ln in lines[2:]:
        t = ln.split()
        if t[:1] == ["element"]:
            element = t[1]
            if element == "vertex":
                nv = int(t[2])
            else:
                nf = int(t[2])
        elif t[:1] == ["property"] and element == "vertex":
            props.append((t[2], {"float": "<f4", "uchar": "u1"}[t[1]]))
    vdt = np.dtype(props)
    verts = np.frombuffer(body[:nv * vdt.itemsize], dtype=vdt)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    faces = np.frombuffer(body[nv * vdt.itemsize:], dtype=fdt)
    assert faces.shape[0] == nf and (faces["n"] == 3).all()
    return [p[0] for p in props], verts, faces["i"]


def read_obj(path):
    """-> (v rows as float lists, vn rows, f rows as lists of "a", "a//a" tokens)."""
    v, vn, f = [], [], []
    for ln in open(path):
        t = ln.split()
        if t[0] == "v":
            v.append([float(x) for x in t[1:]])
        elif t[0] == "vn":
            vn.append([float(x) for x in t[1:]])
        elif t[0] == "f":
            f.append(t[1:])
    return v, vn, f
