"""The numpy oracle of the occupancy grid (tests/occupancy_cases.py) against the stated rules: the
float32 lookup against a float64 formulation away from cell faces, the exact-boundary cases as exactly
representable numbers, the build rule's edge cases and the Q1 map's ragged last chunk."""
import numpy as np

import occupancy_cases as OC

F = np.float32


def test_lookup_matches_float64_away_from_faces():
    rng = np.random.default_rng(0)
    for g, bound in ((32, 1.0), (64, 1.5), (128, 0.7), (512, 1.0)):
        p = (rng.random((20000, 3)) * 2.6 - 1.3) * bound
        in64, c64, face = OC.lookup_cells_f64(p.astype(F), g, bound)
        in32, c32 = OC.lookup_cells(p, g, bound)
        # float32 error of u: a few ulp of G (2^-24 G relative to a cell) -- 1e-3 cells is far outside it
        safe = face > 1e-3
        assert safe.mean() > 0.9
        assert np.array_equal(in32[safe], in64[safe])
        assert np.array_equal(c32[safe & in64], c64[safe & in64])
        assert in64.any() and not in64.all()


def test_lookup_exact_boundaries():
    """bound 1, G 32: the cell width is 1/16; u = 0 is inside, u = G outside, a face belongs to the cell
    above it."""
    g, bound = 32, 1.0
    mid = 0.03125
    p = np.array([[-1.0, mid, mid],          # u_x = 0: cell 0
                  [1.0, mid, mid],           # u_x = G: outside
                  [1.0 - 2.0 ** -23, mid, mid],   # p - lo = 2 - 2^-23 is exact: u < G, cell G - 1
                  [-1.0 - 2.0 ** -23, mid, mid],  # the first float below -1: outside
                  [0.0, 0.0, 0.0],           # on three faces: cell (16, 16, 16)
                  [-0.0625, 0.0625, mid],    # faces 15 and 17
                  [np.nan, mid, mid], [mid, np.inf, mid], [mid, mid, -np.inf], [1e30, 0, 0]], dtype=F)
    inside, c = OC.lookup_cells(p, g, bound)
    assert inside.tolist() == [True, False, True, False, True, True, False, False, False, False]
    cell = lambda ix, iy, iz: (ix * g + iy) * g + iz
    assert c[0] == cell(0, 16, 16) and c[2] == cell(31, 16, 16)
    assert c[4] == cell(16, 16, 16) and c[5] == cell(15, 17, 16)
    # the last float below 1 is inside the cube, but p - lo rounds to 2 and u to G: empty by the rule
    assert not OC.lookup_cells(np.array([[1.0 - 2.0 ** -24, mid, mid]], dtype=F), g, bound)[0][0]


def test_bit_layout():
    g = 32
    occ = np.zeros((g, g, g), dtype=bool)
    occ[1, 2, 3] = occ[0, 0, 31] = occ[31, 31, 31] = True
    bits = OC.pack_cells(occ)
    assert bits.dtype == np.uint32 and bits.shape == (g ** 3 // 32,)
    for ix, iy, iz in ((1, 2, 3), (0, 0, 31), (31, 31, 31)):
        c = (ix * g + iy) * g + iz
        assert bits[c >> 5] >> (c & 31) & 1
    assert sum(bin(int(w)).count("1") for w in bits) == 3
    assert np.array_equal(OC.unpack_cells(bits, g), occ)
    assert OC.bit_of(bits, np.array([(1 * g + 2) * g + 3, 5])).tolist() == [True, False]


def test_build_rule_edges():
    g = 32
    nodes = np.zeros((g + 1,) * 3, dtype=F)
    nodes[5, 6, 7] = 1.0        # equal to the threshold: not occupied
    nodes[10, 10, 10] = np.nan  # NaN: occupied (conservative)
    nodes[20, 20, 20] = np.nextafter(F(1.0), F(2.0))
    occ = OC.build_cells(nodes, 1.0, 0)
    assert not occ[4:7, 5:8, 6:9].any()
    # a node is a corner of the 8 cells around it
    want = np.zeros_like(occ)
    want[9:11, 9:11, 9:11] = True
    want[19:21, 19:21, 19:21] = True
    assert np.array_equal(occ, want)
    for d in (1, 2):
        want = np.zeros_like(occ)
        want[9 - d:11 + d, 9 - d:11 + d, 9 - d:11 + d] = True
        want[19 - d:21 + d, 19 - d:21 + d, 19 - d:21 + d] = True
        assert np.array_equal(OC.build_cells(nodes, 1.0, d), want)


def test_build_dilation_clamped_at_faces():
    g = 32
    nodes = np.zeros((g + 1,) * 3, dtype=F)
    nodes[0, 0, 0] = 2.0          # the corner node: one cell at dilate 0
    nodes[g, 16, g] = 2.0         # a node on two faces
    for d in (0, 1, 2):
        occ = OC.build_cells(nodes, 1.0, d)
        want = np.zeros_like(occ)
        want[:1 + d, :1 + d, :1 + d] = True
        want[g - 1 - d:, 15 - d:17 + d, g - 1 - d:] = True
        assert np.array_equal(occ, want), d
    # dilation = growing the dilate-0 cells by d cells in Chebyshev distance
    rng = np.random.default_rng(1)
    nodes = rng.random((g + 1,) * 3).astype(F)
    base = OC.build_cells(nodes, 0.999, 0)
    assert 0 < base.sum() < base.size
    for d in (1, 2):
        grown = np.zeros_like(base)
        pad = np.pad(base, d)
        for off in np.ndindex(2 * d + 1, 2 * d + 1, 2 * d + 1):
            grown |= pad[off[0]:off[0] + g, off[1]:off[1] + g, off[2]:off[2] + g]
        assert np.array_equal(OC.build_cells(nodes, 0.999, d), grown), d


def test_q1_map():
    # one chunk: sample row k takes ray k mod R
    q = OC.q1_ray(5, 3, 5)
    assert np.array_equal(q.reshape(-1), np.arange(15) % 5)
    # chunk_rows 1: every sample its own ray
    assert np.array_equal(OC.q1_ray(4, 6, 1), np.repeat(np.arange(4)[:, None], 6, axis=1))
    # ragged last chunk: rays 32..36 form a chunk of 5
    q = OC.q1_ray(37, 64, 16)
    assert np.array_equal(q[:16].reshape(-1), np.arange(16 * 64) % 16)
    assert np.array_equal(q[32:].reshape(-1), 32 + np.arange(5 * 64) % 5)


def test_cull_oracle_order_and_faces():
    g, bound = 32, 1.0
    ro, rd, z = OC.face_rays(40, g)
    bits = OC.grid_bits("full", g)
    out = OC.cull(ro, rd, z, 6, None, bits, g, bound)
    # + rays start at u = 0 (inside) and reach u = G at depth 2 = sample 32 (outside); - rays start at
    # u = G (outside) and leave through u = 0 at sample 32, which is still inside
    keep = out["keep"]
    for ray in (0, 2, 4):
        assert keep[ray, :32].all() and not keep[ray, 32:].any()
    for ray in (1, 3, 5):
        assert not keep[ray, 0] and keep[ray, 1:33].all() and not keep[ray, 33:].any()
    assert out["count"] == keep.sum() and np.all(np.diff(out["sample_index"]) > 0)
    assert np.array_equal(out["code_out"], out["sample_index"] // 40)
    half = OC.cull(ro, rd, z, 6, None, OC.grid_bits("half", g), g, bound)
    # along +x the half space x < 0 ends at the face x = 0 (sample 16), which belongs to cell 16
    assert half["keep"][0, :16].all() and not half["keep"][0, 16:].any()
    assert not half["keep"][1, :17].any() and half["keep"][1, 17:33].all()
