"""Iso-surface ray casting stated in numpy: the three rules of include/codenerf.h ("Iso-surface ray casting") with
every operation a separately rounded float32 one, and the whole of render_surface driven from a callable
``sigma_at(points (R, K, 3)) -> (R, K)`` densities.  The device kernels are held to these bit for bit."""
import numpy as np

F = np.float32
EMPTY = F(-1.0e4)                          # CN_EMPTY_SIGMA_RAW: a culled slot's sigma_raw
NAN, INF = F(np.nan), F(np.inf)


def known(s):
    """s > CN_EMPTY_SIGMA_RAW: false for the marker and for NaN."""
    with np.errstate(invalid="ignore"):
        return np.asarray(s, dtype=F) > EMPTY


def reached(s, level):
    """s >= level: a tie counts, a NaN does not."""
    with np.errstate(invalid="ignore"):
        return np.asarray(s, dtype=F) >= F(level)


def bracket(sigma, z, level):
    """sigma, z (R, S) -> bracket (R, 4) = [t_lo, t_hi, s_lo, s_hi], hit (R,) int32."""
    sigma, z = np.asarray(sigma, dtype=F), np.asarray(z, dtype=F)
    r, s = sigma.shape
    assert z.shape == (r, s) and s >= 2
    up = reached(sigma, level)
    some = up.any(axis=1)
    j = up.argmax(axis=1)                  # the first one
    hit = np.where(~some, 0, np.where(j == 0, 2, 1)).astype(np.int32)
    lo = np.where(~some, s - 1, np.maximum(j - 1, 0))
    hi = np.where(~some, s - 1, j)
    rows = np.arange(r)
    return np.stack([z[rows, lo], z[rows, hi], sigma[rows, lo], sigma[rows, hi]], axis=1).astype(F), hit


def step(ro, rd, hit, brk, level, t=None, probe=None, finish=False):
    """One round -> (bracket, t, pts), all new arrays.  ``probe``: the density at ``t``, or None (the first call)."""
    level = F(level)
    b = np.array(brk, dtype=F, copy=True)
    if probe is not None:
        probe, t = np.asarray(probe, dtype=F), np.asarray(t, dtype=F)
        live = hit == 1
        up = live & reached(probe, level)
        dn = live & ~reached(probe, level)            # below the level, or NaN
        b[up, 1], b[up, 3] = t[up], probe[up]
        b[dn, 0], b[dn, 2] = t[dn], probe[dn]
    t_lo, t_hi, s_lo, s_hi = b.T
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if finish:
            ds = s_hi - s_lo
            q = (level - s_lo) / ds
            q = np.where(q > 0, q, F(0))              # max(q, 0): 0 for a NaN quotient
            q = np.where(q < 1, q, F(1))
            w = np.where(known(s_lo) & ~(ds <= 0), q, F(1)).astype(F)
        else:
            w = np.full_like(t_lo, 0.5)
        t_new = (t_lo + w * (t_hi - t_lo)).astype(F)
        pts = (np.asarray(ro, dtype=F) + np.asarray(rd, dtype=F) * t_new[:, None]).astype(F)
    return b, t_new, pts


def colour(raw):
    """sigmoid(x) * 1.002 - 0.001 in float64: the device's sigmoid_hw is within 2e-7 of it."""
    x = np.asarray(raw, dtype=np.float64)
    return 1.002 / (1.0 + np.exp(-x)) - 0.001


def shade(raw, hit, t, pts, background):
    """-> (rgb float64 (R, 3), depth (R,), pts (R, 3)): the hit rows' rgb is the exact formula, everything else
    (depth, pts, the missed rows' rgb) is what the kernel must give bit for bit."""
    miss = np.asarray(hit) == 0
    rgb = colour(np.asarray(raw)[:, :3])
    rgb[miss] = np.asarray(background, dtype=F).astype(np.float64)
    depth = np.where(miss, INF, np.asarray(t, dtype=F)).astype(F)
    out = np.array(pts, dtype=F, copy=True)
    out[miss] = NAN
    return rgb, depth, out


def ray_points(ro, rd, z):
    """ro + rd z, the product and the sum each rounded: (R, 3) x 2, (R, S) -> (R, S, 3)."""
    ro, rd, z = (np.asarray(a, dtype=F) for a in (ro, rd, z))
    return (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).astype(F)


def render_surface(ro, rd, z, level, refine, sigma_at, sigma_search=None, trace=None):
    """The launch sequence of render_surface on the rule -> dict(hit, bracket (R, 4), t, depth, point).
    ``sigma_search``: the search densities (R, S) when they do not come from ``sigma_at`` (a culled call's).
    ``trace``: a list that receives every (bracket, t) in turn."""
    ro, rd, z = (np.asarray(a, dtype=F) for a in (ro, rd, z))
    if sigma_search is None:
        sigma_search = sigma_at(ray_points(ro, rd, z))
    brk, hit = bracket(sigma_search, z, level)
    brk, t, pts = step(ro, rd, hit, brk, level, finish=refine == 0)
    if trace is not None:
        trace.append((brk, t))
    for i in range(refine):
        probe = np.asarray(sigma_at(pts[:, None, :]), dtype=F)[:, 0]
        brk, t, pts = step(ro, rd, hit, brk, level, t=t, probe=probe, finish=i == refine - 1)
        if trace is not None:
            trace.append((brk, t))
    _, depth, point = shade(np.zeros((len(hit), 4), dtype=F), hit, t, pts, (1.0, 1.0, 1.0))
    return dict(hit=hit, bracket=brk, t=t, depth=depth, point=point)


# ---------------------------------------------------------------- hand-made rows: every class of the bracket rule

CLASSES = ("none", "first", "j1", "last", "tie", "nan_before", "nan_at", "pos_inf", "neg_inf", "marker_before",
           "second_crossing")


def class_row(kind, s, level, rng):
    """One ray's S densities of class ``kind`` for ``level`` -> (sigma (S,), the expected (hit, j))."""
    lo = (level - F(1.0) - rng.random(s).astype(F)).astype(F)         # all below the level
    hi = F(level + F(0.5))
    row = lo.copy()
    if kind == "none":
        return row, (0, None)
    if kind == "first":
        row[0] = hi
        return row, (2, 0)
    if kind == "j1":
        row[1] = hi
        return row, (1, 1)
    if kind == "last":
        row[s - 1] = hi
        return row, (1, s - 1)
    j = max(1, (2 * s) // 3)
    if kind == "tie":
        row[j] = F(level)
    elif kind == "nan_before":             # a NaN below the crossing is not a crossing; it can be the low end
        row[j - 1], row[j] = NAN, hi
    elif kind == "nan_at":                 # a NaN where the crossing would be: the next sample is the crossing
        if j == s - 1:
            j -= 1
        if j == 0:                         # S = 2: the NaN is sample 0, the crossing sample 1
            row[0], row[1] = NAN, hi
            return row, (1, 1)
        row[j], row[j + 1] = NAN, hi
        j += 1
    elif kind == "pos_inf":
        row[j] = INF
    elif kind == "neg_inf":
        row[j - 1], row[j] = -INF, hi
    elif kind == "marker_before":
        row[:j], row[j] = EMPTY, hi
    elif kind == "second_crossing":
        row[j] = hi
        if j + 1 < s:
            row[j + 1:] = lo[j + 1:]
            row[s - 1] = hi
    else:
        raise ValueError(kind)
    return row, (1, j)


def class_case(r, s, level=0.25, seed=0, first=0):
    """R rays cycling through CLASSES from class ``first`` on -> (sigma (R, S), z (R, S) ascending, kinds,
    expected [(hit, j)])."""
    rng = np.random.default_rng(seed)
    level = F(level)
    kinds = [CLASSES[(first + k) % len(CLASSES)] for k in range(r)]
    rows, want = zip(*(class_row(k, s, level, rng) for k in kinds))
    z = np.sort(rng.random((r, s)).astype(F) * F(2.0) + F(0.5), axis=1)
    return np.stack(rows).astype(F), z, kinds, list(want)


def rays(r, seed=0):
    """R rays from around (0, 0, -1.3) towards the origin, unnormalised directions."""
    rng = np.random.default_rng(seed)
    ro = (np.array([0.0, 0.0, -1.3]) + 0.05 * rng.standard_normal((r, 3))).astype(F)
    rd = (np.array([0.0, 0.0, 1.0]) + 0.3 * rng.standard_normal((r, 3))).astype(F)
    return ro, rd
