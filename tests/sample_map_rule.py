"""The rule of drt_render_sample_map (include/drt_hip.h), restated in numpy. Not a test file: the tests of
the sample maps import it.

Every tile pixel p holds a count n_p (its filter sum) and is given a target. Absolute mode: R_p = target - n_p where the target is the
larger, else 0 (the pixel is "above" when n_p > target). Add mode: R_p = target. With B the OR of all R_p, one round per set bit b of
B, ascending, renders the next 2^b samples of every pixel whose R_p has bit b, each from the count it holds then, the pixels listed in
ascending tile order."""
import numpy as np

LIMIT = 0xFFFFFFFF


def plan(counts, targets, add=False):
    """-> dict: remainders [P] (uint32), B, rounds [(b, pixels ascending, 2^b)], starts (per round: the count each listed pixel holds
    when the round begins), final counts [P], and the report words the call returns."""
    n = np.asarray(counts).astype(np.int64).reshape(-1)
    t = np.asarray(targets).astype(np.int64).reshape(-1)
    assert n.shape == t.shape and (n >= 0).all() and (n <= LIMIT).all() and (t >= 0).all() and (t <= LIMIT).all()
    if add:
        over = np.nonzero(n + t > LIMIT)[0]
        if over.size:
            raise OverflowError(int(over[0]))  # the first tile pixel whose count would pass 2^32 - 1
        R = t.copy()
        above = 0
    else:
        R = np.where(t > n, t - n, 0)
        above = int((n > t).sum())
    B = int(np.bitwise_or.reduce(R)) if R.size else 0
    rounds, starts, held = [], [], n.copy()
    for b in range(32):
        if not (B >> b) & 1:
            continue
        pixels = np.nonzero((R >> b) & 1)[0]
        rounds.append((b, pixels, 1 << b))
        starts.append(held[pixels].copy())
        held[pixels] += 1 << b
    return {"remainders": R.astype(np.uint32), "B": B, "rounds": rounds, "starts": starts, "final": held.astype(np.uint32),
            "report": {"rounds": bin(B).count("1"), "paths": int(R.sum()), "pixels_rendered": int((R > 0).sum()),
                       "pixels_above": above, "max_count": int(held.max()) if held.size else 0}}


def region_map(tile_w, tile_h, base, regions):
    """base everywhere; inside a region (x, y, w, h, spp), clipped to the tile, the largest spp of the regions over the pixel (and base)"""
    m = np.full((tile_h, tile_w), base, dtype=np.int64)
    for y in range(tile_h):
        for x in range(tile_w):
            for rx, ry, rw, rh, spp in regions:
                if rx <= x < rx + rw and ry <= y < ry + rh:
                    m[y, x] = max(m[y, x], spp)
    return m.astype(np.uint32)


def coverage_map(coverage, base, extra):
    """base + ceil(extra * coverage)"""
    c = np.asarray(coverage, dtype=np.float64)
    return (base + np.ceil(extra * c)).astype(np.uint32)
