"""The trace kernel's path-id arithmetic on the device (drt_selftest_path_ids) against the plain 64-bit form.

A wave of the trace kernel draws a chunk of consecutive path ids, divides the chunk's first id by n_samples once (64 bits), and
from there on finds each lane's (pixel, sample) and the wave's own position with 32-bit arithmetic; a tile pixel below 2^32 is
split into (i, j) by a 32-bit division. Every one of these must be the integer the 64-bit division gives:
    q = id // n_samples, s = id % n_samples, j = q // tile_w, i = q % tile_w.
"""
import numpy as np
import pytest

import pydrt

pytestmark = pytest.mark.gpu

N_SAMPLES = [1, 3, 16, 63, 64, 65, 256, 1024]
TILE_WIDTHS = [1, 3, 37, 1000, 1023, 2049, 65537]  # none but 1 is a power of two

# ids handed out per refill: whole waves, single lanes, odd counts -- 1024 ids in all, the largest chunk the launcher hands a wave
STEPS = np.array([64, 1, 37, 64, 5, 63, 2, 64, 20] * 3 + [64], dtype=np.uint32)


def _bases(n_samples, tile_w):
    two32 = 1 << 32
    b = {0, 1, 63, 64, 1024, 3 * 1024 + 64}
    # chunk boundaries of every chunk size the launcher hands out, at and around a pixel's last sample
    for chunk in (64, 256, 1024):
        for k in (1, 7, 1000003):
            b.add(k * chunk)
    for q in (1, tile_w - 1, tile_w, tile_w + 1, 5 * tile_w - 1, 1000 * tile_w + 7):
        for d in (-65, -64, -1, 0, 1):
            b.add(max(0, q * n_samples + d))
    # ids around 2^32 (a launch of 2^32 paths: 2048^2 pixels of 1024 samples), and pixels around 2^32 (the 64-bit tile split)
    for d in (-1024, -65, -64, -1, 0, 1, 64, 1000):
        b.add(two32 + d)
        b.add(3 * two32 + d)
        b.add(max(0, two32 * n_samples + d))
        b.add(max(0, (two32 - 1) * n_samples + d))
    return np.array(sorted(b), dtype=np.uint64)


@pytest.mark.parametrize("n_samples", N_SAMPLES)
def test_path_ids_match_the_64_bit_division(n_samples):
    assert STEPS.min() >= 1 and STEPS.max() <= 64 and int(STEPS.sum()) == 1024
    for tile_w in TILE_WIDTHS:
        bases = _bases(n_samples, tile_w)
        got = pydrt.selftest_path_ids(bases, STEPS, n_samples, tile_w)
        ids = bases[:, None] + np.arange(int(STEPS.sum()), dtype=np.uint64)[None, :]
        q = ids // np.uint64(n_samples)
        s = ids - q * np.uint64(n_samples)
        j = (q // np.uint64(tile_w)).astype(np.uint32).astype(np.uint64)  # the kernel keeps 32 bits of j, as it always did
        i = ((q - (q // np.uint64(tile_w)) * np.uint64(tile_w))).astype(np.uint32).astype(np.uint64)
        for name, want, k in (("pixel", q, 0), ("sample", s, 1), ("i", i, 2), ("j", j, 3)):
            bad = np.argwhere(got[:, :, k] != want)
            assert bad.size == 0, "%s differs for n_samples %d, tile_w %d: id %d gives %d, not %d" % (
                name, n_samples, tile_w, int(ids[tuple(bad[0])]), int(got[tuple(bad[0]) + (k,)]), int(want[tuple(bad[0])]))


def test_path_ids_steps_of_every_size():
    """every refill size 1..64 at every offset within a pixel's samples, for sample counts below, at and above the wave's width"""
    steps = np.arange(1, 65, dtype=np.uint32)
    n = int(steps.sum())
    for n_samples in (1, 2, 3, 5, 63, 64, 65, 127, 0xFFFFFFFF):
        bases = np.array([0, 1, n_samples - 1, n_samples, 7 * n_samples + 3, (1 << 32) - 17, (1 << 40) + 5], dtype=np.uint64)
        got = pydrt.selftest_path_ids(bases, steps, n_samples, 1001)
        ids = bases[:, None] + np.arange(n, dtype=np.uint64)[None, :]
        q = ids // np.uint64(n_samples)
        assert np.array_equal(got[:, :, 0], q), n_samples
        assert np.array_equal(got[:, :, 1], ids - q * np.uint64(n_samples)), n_samples
        assert np.array_equal(got[:, :, 2], q % np.uint64(1001)), n_samples
        assert np.array_equal(got[:, :, 3], q // np.uint64(1001)), n_samples
