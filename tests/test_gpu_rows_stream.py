"""The folded table variant's schedule (field_w16_kernel<.., FOLD, ROWS>): the weight DMA spread over a
chunk's last k-steps, one code row staged before the tile loop, the next tile's inputs loaded during
layer_dir2 and carried across the tile boundary (27 weight chunks per tile, counter folded mod 108).

None of that changes an arithmetic operation or its order, so every case is bitwise against the in-kernel
folded path (``view_rows=False``), whose code this schedule does not touch."""
import pytest
import torch

import buffers as B
from test_gpu_grad import dev  # noqa: F401
from test_gpu_view_rows import field, hash_model, random_rays

pytestmark = pytest.mark.gpu

TILE = 128


def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def both(dev, d, s, chunk, mode="rayz"):
    params, pk, cb, fb = hash_model(dev)
    on = field(pk, cb, fb, d, s, chunk, mode, view_rows=True)
    off = field(pk, cb, fb, d, s, chunk, mode, view_rows=False)
    return on, off


# ---------------------------------------------------------------- small M

# (rays, samples): M = 1, 16, 17, 127, 128, 129 -- fewer tiles than workgroups; a workgroup's only tile,
# partial or full, takes its inputs from the kernel's prologue and has no next tile to load for
SMALL = ((1, 1), (2, 8), (17, 1), (127, 1), (16, 8), (43, 3))


@pytest.mark.parametrize("mode", ["rayz", "pts"])
@pytest.mark.parametrize("r,s", SMALL)
def test_small_m(dev, r, s, mode):
    d = random_rays(dev, r, s, 31 * r + s)
    on, off = both(dev, d, s, 5, mode)
    assert bool(torch.isfinite(off).all())
    assert torch.equal(on, off)


# ---------------------------------------------------------------- tile counts, counter fold, lazy / up-front

def tile_count_shapes(dev):
    """S = 64, R = (4 cus 128) / 64 + 3: four tiles per workgroup and 1.5 more, so two workgroups run a fifth
    tile past the counter's fold and the last tile is half full; one ray less; and S = 8."""
    r = (4 * cus(dev) * TILE) // 64 + 3
    return ((r, 64), (r - 1, 64), (r, 8))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_tile_counts(dev, which):
    r, s = tile_count_shapes(dev)[which]
    d = random_rays(dev, r, s, 77 + which)
    on, off = both(dev, d, s, 512)
    assert bool(torch.isfinite(off).all())
    assert torch.equal(on, off)


@pytest.mark.parametrize("k", [0, 1, 5])
def test_lazy_and_up_front_tiles_mixed(dev, k):
    """ro = 40 in the two rays of tile cus + k sends that tile's waves to the up-front sincosf path, while
    tiles k and 2 cus + k of the same workgroup stay lazy: inputs loaded during a lazy tile feed an up-front
    one and the other way round.  Finite, equal to forced off, and every other ray keeps the bits of a launch
    without the 40."""
    r, s = tile_count_shapes(dev)[0]
    n = cus(dev)
    d = random_rays(dev, r, s, 77)
    params, pk, cb, fb = hash_model(dev)
    plain = field(pk, cb, fb, d, s, 512, view_rows=True)
    far = dict(d, ro=d["ro"].clone())
    far["ro"][2 * (n + k):2 * (n + k) + 2] = 40.0
    on = field(pk, cb, fb, far, s, 512, view_rows=True)
    off = field(pk, cb, fb, far, s, 512, view_rows=False)
    assert bool(torch.isfinite(on).all())
    assert torch.equal(on, off)
    keep = torch.ones(r, dtype=torch.bool, device=on.device)
    keep[2 * (n + k):2 * (n + k) + 2] = False
    assert torch.equal(on.reshape(r, s, 4)[keep], plain.reshape(r, s, 4)[keep])
    assert not torch.equal(on.reshape(r, s, 4)[~keep], plain.reshape(r, s, 4)[~keep])


# ---------------------------------------------------------------- buffers

def test_last_row_is_the_last_element(dev):
    """z, ro and rd each end at their trailing guard and the outputs come poisoned (zeros, then NaN): no
    guard is stored into, no NaN is left in the output (every row was written), and both fills equal the
    in-kernel path in every bit.  A read past an input's end would not be seen here: the guards catch stores
    only.  M = 3 tiles and a part of a fourth, so the last tile's rows past m and the missing next tile are
    both on the path."""
    params, pk, cb, fb = hash_model(dev)
    r, s, chunk = 83, 5, 16
    src = random_rays(dev, r, s, 5)
    off = field(pk, cb, fb, src, s, chunk, view_rows=False)
    outs = []
    for fill in B.FILLS:
        with B.contracts(fill) as arena:
            d = {k: arena.empty(tuple(src[k].shape), torch.float32, dev).copy_(src[k]) for k in ("rd", "ro", "z")}
            outs.append(field(pk, cb, fb, d, s, chunk, view_rows=True))
            assert arena.n_allocations > 3      # the three inputs, and what ops.radiance_field allocated
    for o in outs:
        assert not bool(torch.isnan(o).any())
        assert torch.equal(B.tensor_bytes(o), B.tensor_bytes(off))


def test_two_launches_into_poisoned_outputs_agree(dev):
    params, pk, cb, fb = hash_model(dev)
    r, s = tile_count_shapes(dev)[1]
    d = random_rays(dev, r, s, 9)
    with B.contracts("poison"):
        a = field(pk, cb, fb, d, s, 512, view_rows=True)
        b = field(pk, cb, fb, d, s, 512, view_rows=True)
    assert not bool(torch.isnan(a).any())
    assert torch.equal(B.tensor_bytes(a), B.tensor_bytes(b))
