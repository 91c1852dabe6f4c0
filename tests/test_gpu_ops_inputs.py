"""The field wrappers' shared input checks (ops._ray_inputs, ops._point_inputs): every wrapper refuses a
wrongly shaped input with AssertionError before anything is launched, and accepts strided views of rd, ro
and z, giving the bits of the same call on contiguous copies.

Synthetic model, 3 rays x 16 samples, chunk_rows 2, one code row.  A row is left out only where the wrapper
has no such argument or rule: the density wrappers take points of any (R, S, 3) and no freqs_dir, and
encode_inputs takes no codes."""
import pytest
import torch

from test_gpu_field_exact import FD, FX
from test_gpu_grad import dev  # noqa: F401

pytestmark = pytest.mark.gpu

N, S, CHUNK = 3, 16, 2

# every C entry a wrapper below can reach: none may be called for a refused input
ENTRIES = ("cn_radiance_field", "cn_radiance_field_fold", "cn_radiance_field_fold_rows", "cn_view_rows",
           "cn_radiance_field_train", "cn_radiance_field_train_fmt", "cn_radiance_field_masks_fmt", "cn_encode_inputs",
           "cn_field_backward_fused_ws", "cn_field_backward_train_multi", "cn_density_field", "cn_density_gradient")


@pytest.fixture(scope="module")
def model(dev):
    """Weights, packs and code terms (1 and 2 code rows), and the forwards' products the backwards read."""
    from codenerf import ops, synthetic
    params = [t.to(dev) for t in synthetic.codenerf_params(0).values()]
    m = dict(params=params, packs={f: ops.mlp_pack(params, f) for f in ("f32", "f32_w16", "f32_w16_t", "f32_w16_fold")})
    for k in (1, 2):
        m[f"cb{k}"] = ops.code_bias(params, synthetic.latent_codes(5, k).to(dev), synthetic.latent_codes(6, k).to(dev))
    m["fold"] = ops.fold_bias(params, m["cb1"])
    g = torch.Generator().manual_seed(11)
    m["geo"] = dict(rd=torch.randn(N, 3, generator=g).to(dev), ro=torch.randn(N, 3, generator=g).to(dev),
                    z=(0.8 + torch.rand(N, S, generator=g)).to(dev), pts=None, code_index=None, cb=m["cb1"], fx=FX,
                    fd=FD)
    m["d_raw"] = torch.randn(N, S, 4, generator=g).to(dev)
    geo = m["geo"]
    _, m["masks"] = ops.radiance_field_masks(m["packs"]["f32_w16"], geo["cb"], geo["rd"], S, CHUNK, FX, FD, ro=geo["ro"],
                                             z=geo["z"], precision="f32")
    _, m["saved"], m["train_masks"] = ops.radiance_field_train_w16(m["packs"]["f32_w16"], geo["cb"], geo["rd"], S,
                                                                   CHUNK, FX, FD, ro=geo["ro"], z=geo["z"])
    return m


def _field(precision, **kw):
    def run(m, g, **_):
        from codenerf import ops
        fold = m["fold"] if precision == "f32_w16_fold" else None
        return ops.radiance_field(m["packs"][precision], g["cb"], g["rd"], S, CHUNK, g["fx"], g["fd"], pts=g["pts"],
                                  ro=g["ro"], z=g["z"], code_index=g["code_index"], precision=precision,
                                  fold_bias=fold, **kw)
    return run


def _forward(name, pack, **kw):
    def run(m, g, **_):
        from codenerf import ops
        return getattr(ops, name)(m["packs"][pack], g["cb"], g["rd"], S, CHUNK, g["fx"], g["fd"], pts=g["pts"],
                                  ro=g["ro"], z=g["z"], code_index=g["code_index"], **kw)
    return run


def _encode(m, g, **_):
    from codenerf import ops
    return ops.encode_inputs(g["rd"], S, CHUNK, g["fx"], g["fd"], pts=g["pts"], ro=g["ro"], z=g["z"])


def _backward_x3(m, g, into=None):
    from codenerf import ops
    n_codes = g["cb"].shape[0]
    return ops.field_backward_x3(m["packs"]["f32_w16_t"], m["masks"], m["d_raw"], N, S, CHUNK, n_codes, g["fx"],
                                 g["fd"], g["rd"], pts=g["pts"], ro=g["ro"], z=g["z"], code_index=g["code_index"],
                                 want_ro=g["pts"] is None, want_rd=g["pts"] is None, precision="f32", acc=into)


def _backward_train(m, g, into=None):
    from codenerf import ops
    n_codes = g["cb"].shape[0]
    # one code row and parameter gradients: g_code and every dW are fixed-order sums.  No ray gradients: the
    # training backward adds d ro / d rd up with float atomics, which do not repeat their own bits.
    grads = [torch.zeros_like(p) for p in m["params"]]
    r = ops.field_backward_train(m["packs"]["f32_w16_t"], m["params"], m["train_masks"], m["saved"], None, m["d_raw"],
                                 N, S, CHUNK, n_codes, g["fx"], g["fd"], g["rd"], pts=g["pts"], ro=g["ro"], z=g["z"],
                                 code_index=g["code_index"], param_grads=grads, g_code=into)
    return dict(r, grads=grads)


def _density(m, g, **_):
    from codenerf import ops
    rays = {} if g["pts"] is not None else dict(ro=g["ro"], rd=g["rd"], z=g["z"])
    return ops.density_field(m["packs"]["f32_w16"], g["cb"], g["fx"], pts=g["pts"], code_index=g["code_index"],
                             want_raw=True, **rays)


def _density_gradient(m, g, **_):
    from codenerf import ops
    rays = {} if g["pts"] is not None else dict(ro=g["ro"], rd=g["rd"], z=g["z"])
    return ops.density_gradient(m["packs"]["f32_w16"], m["packs"]["f32_w16_t"], g["cb"], g["fx"], pts=g["pts"],
                                code_index=g["code_index"], **rays)


WRAPPERS = {
    "radiance_field": _field("f32_w16"),
    "radiance_field-fold": _field("f32_w16_fold", view_rows=False),
    "radiance_field-fold-view_rows": _field("f32_w16_fold", view_rows=True),
    "radiance_field_train": _forward("radiance_field_train", "f32"),
    "radiance_field_train_w16": _forward("radiance_field_train_w16", "f32_w16"),
    "radiance_field_masks": _forward("radiance_field_masks", "f32_w16", precision="f32"),
    "encode_inputs": _encode,
    "field_backward_x3": _backward_x3,
    "field_backward_train": _backward_train,
    "density_field": _density,
    "density_gradient": _density_gradient,
}
DENSITY = ("density_field", "density_gradient")


def _bad_inputs(m):
    dev = m["geo"]["rd"].device
    return {
        "pts (3, 17, 3)": dict(pts=torch.zeros(N, S + 1, 3, device=dev), ro=None, z=None),
        "z (4, 16)": dict(z=torch.ones(N + 1, S, device=dev)),
        "ro (3, 2)": dict(ro=torch.zeros(N, 2, device=dev)),
        "rd (3, 4)": dict(rd=torch.ones(N, 4, device=dev)),
        "code_index (2,)": dict(code_index=torch.zeros(2, device=dev, dtype=torch.int64)),
        "two code rows, three rays, no code_index": dict(cb=m["cb2"]),
        "nine freqs_xyz": dict(fx=FX[:9]),
        "three freqs_dir": dict(fd=FD[:3]),
    }


BAD = ("pts (3, 17, 3)", "z (4, 16)", "ro (3, 2)", "rd (3, 4)", "code_index (2,)",
       "two code rows, three rays, no code_index", "nine freqs_xyz", "three freqs_dir")


def _applies(wrapper, bad):
    if wrapper in DENSITY and bad in ("pts (3, 17, 3)", "three freqs_dir"):
        return False      # any (R, S, 3) is a valid point set there, and there is no freqs_dir
    if wrapper == "encode_inputs" and bad in ("code_index (2,)", "two code rows, three rays, no code_index"):
        return False      # no codes
    return True


@pytest.mark.parametrize("wrapper,bad", [(w, b) for w in sorted(WRAPPERS) for b in BAD if _applies(w, b)])
def test_refused_before_any_launch(model, monkeypatch, wrapper, bad):
    from codenerf import _lib
    lib = _lib.load()

    def reached(*a, **k):
        pytest.fail(f"{wrapper}: the C entry was called for {bad}")
    for name in ENTRIES:
        monkeypatch.setattr(lib, name, reached)
    g = dict(model["geo"], **_bad_inputs(model)[bad])
    # the accumulators a caller hands in stay as they were
    n_codes = g["cb"].shape[0]
    into = None
    if wrapper == "field_backward_x3":
        from codenerf import ops
        into = torch.full((ops.field_backward_x3_acc_floats(n_codes, N, g["pts"] is None, g["pts"] is None),), 7.0,
                          device=g["rd"].device)
    elif wrapper == "field_backward_train":
        into = torch.full((n_codes, _lib.CN_CODE_BIAS_STRIDE), 7.0, device=g["rd"].device)
    with pytest.raises(AssertionError):
        WRAPPERS[wrapper](model, g, into=into)
    if into is not None:
        assert bool((into == 7.0).all())


def _tensors(out):
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        out = [out[k] for k in sorted(out)]
    return [t for o in out if o is not None for t in _tensors(o)]


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_strided_views_give_the_contiguous_bits(model, wrapper):
    geo = model["geo"]
    dev = geo["rd"].device
    strided = {}
    for k in ("rd", "ro", "z"):
        wide = torch.zeros(N, 2 * geo[k].shape[1], device=dev)
        wide[:, ::2] = geo[k]
        strided[k] = wide[:, ::2]
        assert not strided[k].is_contiguous() and torch.equal(strided[k], geo[k])
    got = _tensors(WRAPPERS[wrapper](model, dict(geo, **strided)))
    ref = _tensors(WRAPPERS[wrapper](model, dict(geo, **{k: v.contiguous() for k, v in strided.items()})))
    assert len(got) == len(ref) > 0
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
