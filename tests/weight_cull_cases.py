"""A numpy model of weight-bounded colour culling (include/codenerf.h, "Weight-bounded colour
culling"): the kept rule, the thresholds of a tolerance, the dropped weight, and cn_weight_cull's
outputs built from occupancy_cases' ray points and Q1 map -- written from the stated rule, plus the
weight rows the CPU and GPU tests share.

The tails are summed in float64 in numpy's own order, which is not the kernel's.  The tests do not
depend on the order: their weights are multiples of 2^-30 (every partial sum of <= 512 such weights
<= 1 is exact in float64, whatever the order), or they assert first that no tail lies within 1e-9
relative of eps_tail (``band_count``), far more than two orders can differ by."""
import numpy as np

import occupancy_cases as OC

F = np.float32
DYADIC = 2.0 ** -30
BAND = 1e-9


def thresholds(tol, n_samples):
    """(eps_weight float32, eps_tail float) of render_rays' rgb_tolerance: the largest float32 <=
    tol / (2 S), and tol / 2."""
    x = tol / (2.0 * n_samples)
    f = F(x)
    if float(f) > x:
        f = np.nextafter(f, F(-np.inf), dtype=F)
    return F(f), tol / 2.0


def tails(w):
    """tail_i = sum_{k >= i} (double)w_k per row -> float64 (R, S); NaN from a NaN weight on."""
    w64 = np.asarray(w, dtype=F).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.cumsum(w64[..., ::-1], axis=-1)[..., ::-1]


def keep_mask(w, eps_weight, eps_tail):
    """Kept iff w > 0, w >= eps_weight (both float32 comparisons) and tail >= (double)eps_tail; NaN fails."""
    w = np.asarray(w, dtype=F)
    with np.errstate(invalid="ignore"):
        return (w > F(0)) & (w >= F(eps_weight)) & (tails(w) >= np.float64(eps_tail))


def dropped_weight(w, keep):
    """The culled samples' weights, summed per ray in float64 (NaN weights count as 0 here)."""
    w64 = np.nan_to_num(np.asarray(w, dtype=F).astype(np.float64), nan=0.0)
    return np.where(keep, 0.0, w64).sum(axis=-1)


def band_count(w, eps_tail, rel=BAND):
    """How many tails lie within ``rel`` relative of eps_tail (where the summation order could decide)."""
    t = tails(w)
    with np.errstate(invalid="ignore"):
        return int((np.abs(t - eps_tail) <= rel * eps_tail).sum()) if eps_tail > 0 else 0


def cull(w, ro, rd, z, chunk_rows, code_index, eps_weight, eps_tail):
    """cn_weight_cull's outputs -> dict(keep (R, S), count, sample_index, pts, vdir, code_out)."""
    rd = np.asarray(rd, dtype=F)
    n, s = np.asarray(z).shape
    keep = keep_mask(w, eps_weight, eps_tail)
    p = OC.ray_points(ro, rd, z)
    k = np.nonzero(keep.reshape(-1))[0]                       # ascending sample order
    code = np.arange(n, dtype=np.int64) if code_index is None else np.asarray(code_index, dtype=np.int64)
    return dict(keep=keep, count=int(k.size), sample_index=k.astype(np.int32), pts=p.reshape(-1, 3)[k],
                vdir=rd[OC.q1_ray(n, s, chunk_rows).reshape(-1)[k]], code_out=code[k // s])


# ---------------------------------------------------------------- weight rows

EPS_WEIGHT = F(2.0 ** -12)       # the shared dyadic thresholds of the ops-level tests
EPS_TAIL = 2.0 ** -7


def dyadic_weights(n_rays, n_samples, seed):
    """Rows of multiples of 2^-30 that sum to <= 1, shaped like a render's (a bump that dies away at a
    random rate), with the special rows the rule has branches for (as far as R allows): all zero
    (count 0), all kept, a NaN in the middle, ties at both thresholds, and exact zeros between
    kept samples."""
    rng = np.random.default_rng(seed)
    r, s = n_rays, n_samples
    rate = rng.uniform(0.02, 1.5, size=(r, 1))
    raw = rng.random((r, s)) * np.exp(-rate * np.arange(s)[None, :])
    raw[rng.random((r, s)) < 0.1] = 0.0
    w = np.floor(raw / np.maximum(raw.sum(axis=-1, keepdims=True), 1e-30) * 0.999 / DYADIC) * DYADIC
    rows = iter(range(r))

    def take():
        return next(rows, None)
    i = take()
    if i is not None and r > 1:
        w[i] = 0.0                                            # nothing kept
    i = take()
    if i is not None:                                         # every sample kept: equal weights, each
        v = max(float(EPS_WEIGHT), np.ceil(EPS_TAIL / DYADIC) * DYADIC)    # >= both thresholds alone
        w[i] = v if v * s <= 1.0 else w[i]
    i = take()
    if i is not None:
        w[i, s // 2] = np.nan                                 # culls itself and all before it
    i = take()
    if i is not None:                                         # ties: w == eps_weight with a big tail behind,
        w[i] = 0.0                                            # and a last sample whose tail == eps_tail
        w[i, 0] = float(EPS_WEIGHT)
        w[i, -1] = EPS_TAIL
        if s > 2:
            w[i, 1] = float(EPS_WEIGHT) - DYADIC              # just below: culled
    i = take()
    if i is not None:                                         # tail just below eps_tail: all culled
        w[i] = 0.0
        w[i, -1] = EPS_TAIL - DYADIC
        w[i, 0] = 0.0 if s > 1 else w[i, 0]
    w = w.astype(F)
    assert np.array_equal(np.nan_to_num(w.astype(np.float64)) % DYADIC, np.zeros((r, s)))      # still dyadic in fp32
    return w


def adversarial_weights(n_samples):
    """Rows that push the dropped weight towards the bound of a tolerance: every sample just below
    eps_weight; a long flat tail just below eps_tail after one heavy sample; both at once."""
    def rows(tol):
        ew, et = thresholds(tol, n_samples)
        below = np.nextafter(ew, F(0))
        a = np.full(n_samples, below, dtype=F)
        b = np.zeros(n_samples, dtype=F)
        b[0] = F(0.9)
        if n_samples > 1:
            b[1:] = F(et * 0.999 / (n_samples - 1))
        c = np.full(n_samples, below, dtype=F)
        c[0] = F(0.5)
        c[n_samples // 2:] = F(et * 0.999 / max(1, n_samples - n_samples // 2))
        return np.stack([a, b, c])
    return rows
