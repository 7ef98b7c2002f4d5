"""GPU (-m gpu): the material layer gives a lane the same bits whatever its neighbours in the wave do.

sample_direction runs the six direction samplers as phases shared by the lanes of a wave, and eval_coefficients shares
normalise(out + in) between glossy and GGX lanes, with each lane choosing its operands by select. This test compares waves that mix
all six samplers (and all materials) lane by lane with the same records run one sampler (one material) per launch. It compares
directions, reciprocal pdfs, RNG states and draw counts, and spectra and flags, bit for bit. It is a smoke check for cross-lane
interference only, such as a wave-wide decision or loop exit that leaks from one lane's sampler into another's. A lane-local
mistake gives the same wrong bits both ways and passes here. The guard for that is tests/test_gpu_materials.py, which holds every
sampler and evaluation against the oracle."""
import numpy as np
import pytest

from cases import same_bits
import pydrt
from test_gpu_materials import bdsf_materials, dot3, eval_rec, incomings, material_scene, media, sample_rec, unit

pytestmark = pytest.mark.gpu

N_DIRF = 6


def _point(rng):
    nrm, out = unit(rng), unit(rng)
    if dot3(nrm, out) < 0:
        out = -out
    return np.concatenate([rng.uniform(-2, 2, 3), nrm, out, [dot3(nrm, out)]])


def test_samplers_mixed_lane_by_lane_equal_one_sampler_per_launch():
    bundle, r = material_scene()
    rng = np.random.default_rng(20261015)
    water = bundle.material_names().index("water")
    mats_ok = bdsf_materials(bundle)
    recs = []
    for k in range(64 * 96):
        m = int(rng.choice(mats_ok))
        mats = media(bundle, m, water)[int(rng.integers(0, 4))]
        recs.append(sample_rec(_point(rng), mats, k % N_DIRF, int(rng.integers(1, 2 ** 63))))  # lane k samples with function k mod 6
    recs = np.array(recs)
    mixed = pydrt.selftest_material(r, pydrt.MAT_SAMPLE, recs)
    for f in range(N_DIRF):
        sel = np.flatnonzero(recs[:, 13] == f)
        alone = pydrt.selftest_material(r, pydrt.MAT_SAMPLE, recs[sel])
        bad = [i for i in range(len(sel)) if not same_bits(mixed[sel[i]], alone[i])]
        assert not bad, "sampler %d: %d of %d records differ between mixed and single-sampler waves; first: %s -> %s vs %s" % (
            f, len(bad), len(sel), recs[sel[bad[0]]].tolist(), mixed[sel[bad[0]]].tolist(), alone[bad[0]].tolist())
    # every sampler drew what it draws: two per pass of the disc's and the GGX loop, one coin, none for the fixed directions
    draws, f = mixed[:, 5], recs[:, 13]
    assert (draws[(f == 0) | (f == 1) | (f == 5)] % 2 == 0).all() and (draws[(f == 0) | (f == 1) | (f == 5)] >= 2).all()
    assert (draws[f == 4] == 1).all() and (draws[(f == 2) | (f == 3)] == 0).all()


def test_evaluations_mixed_lane_by_lane_equal_one_material_per_launch():
    bundle, r = material_scene()
    rng = np.random.default_rng(1016)
    water = bundle.material_names().index("water")
    mats_ok = bdsf_materials(bundle)
    recs = []
    for k in range(64 * 64):
        m = mats_ok[k % len(mats_ok)]
        mats = media(bundle, m, water)[int(rng.integers(0, 4))]
        pt = _point(rng)
        ins = incomings(bundle, pt, mats, rng)  # the exact mirror and refracted directions among them
        recs.append(eval_rec(pt, mats, ins[int(rng.integers(0, len(ins)))]))
    recs = np.array(recs)
    mixed = pydrt.selftest_material(r, pydrt.MAT_EVALUATE, recs)
    for m in mats_ok:
        sel = np.flatnonzero(recs[:, 10] == m)
        alone = pydrt.selftest_material(r, pydrt.MAT_EVALUATE, recs[sel])
        bad = [i for i in range(len(sel)) if not same_bits(mixed[sel[i]], alone[i])]
        assert not bad, "material %d: %d of %d records differ between mixed and single-material waves" % (m, len(bad), len(sel))
    flags = mixed[:, -1].astype(np.int64)
    assert (flags & 1).any() and (flags & 2).any()
