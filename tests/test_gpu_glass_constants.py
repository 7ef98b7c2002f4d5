"""The glass constants of the trace kernel (csrc/drt_const_rule.h, drt_glass_constants; csrc/drt_kernels.h, vertex_dirs and the
reflect-or-transmit sampler): a glass vertex takes ir / tr of its pair of media, and its media's indices at trans_wl, from values its
workgroup tabulated once per launch instead of dividing them out itself. The operations are the vertex's own, so NOTHING may change:
tiles of 32 x 32 pixels, 4 samples, depth 8, whose film, hit log and path statistics must be the CPU oracle's bit for bit.

The oracle is also what a library built with the step switched off (-DDRT_GLASS_CONSTANTS=0) is held to by the rest of the suite, so
equality with the oracle is equality with that library; it is not built here (a build takes longer than the whole suite).

Scenes: every shipped scene with a dielectric in it, and cornell_plane_light.scn rewritten:
  - a dense glass sphere inside the glass sphere,
  - a base material that is not vacuum (water), alone and with the dense sphere,
  - the camera inside a glass ball dense enough that most of its rays meet total internal reflection (a NaN direction),
  - glass, GGX gold and mirror spheres side by side, so that single waves hold all three,
  - trans_wl between two samples of the wavelength grid (a 4 nm grid), so that the index at trans_wl really interpolates.
And a live context after an update that changes the glass's or the base material's refraction spectrum, in host mode and in device
mode (the cases of tests/material_update_cases.py): the constants are made again at every launch, so no update can leave them stale.
"""
import os

import numpy as np
import pytest

import cases
import material_update_cases as MU
import pydrt
import test_gpu_material_update as TU

W = H = 32
DENSE = ("\nMaterial\nname dense_glass\nrefract constant 1.9\nglossy constant 1.0\nshininess 16.0\n"
         "bdsfs fs_dielectric_reflectance_bdsf, fs_dielectric_transmittance_bdsf\ndir_func sample_reflect_or_transmit_direction\n")


def _transmits(bundle):
    return any(MU.FS_TRANSMIT in MU.bdsfs_of(bundle.scene.materials[i]) for i in range(int(bundle.scene.num_materials)))


def shipped():
    out = []
    for f in sorted(os.listdir(os.path.join(cases.REPO, "scenes"))):
        if f.endswith(".scn") and f != "example_scene.scn":  # (its camera is NaN: no ray meets anything)
            if _transmits(pydrt.load_scene(cases.scene_path(f), W, H)):
                out.append(f)
    return out


def authored():
    base = open(cases.scene_path("cornell_plane_light.scn")).read()
    inner = cases._surface("inner", "sphere", "position -1.5, -1.8, 2.0\nradius 0.5", "dense_glass")
    water = base.replace("refract constant 1.0", "refract constant 1.33")
    inside = cases.degenerate_scenes()["camera_inside_the_glass_ball"]
    assert water != base and "refract csv glass.csv" in inside and "position -1.5, -1.8, 2.2" in inside
    return {
        "glass in glass": base + DENSE + inner,
        "base material water": water,
        "base material water, glass in glass": water + DENSE + inner,
        "camera inside the glass ball": inside,
        # 0.9 radii off the centre of a ball of index 2.4 (critical angle 24.6 degrees): rays meet its inside at up to 64 degrees
        "camera inside a dense ball: total internal reflection": inside.replace("refract csv glass.csv", "refract constant 2.4")
                                                                       .replace("position -1.5, -1.8, 2.2", "position -1.5, -1.8, 2.9"),
        "glass, gold and mirror side by side": base + DENSE
        + cases._surface("g2", "sphere", "position 0.9, -2.3, 0.2\nradius 0.55", "dielectric")
        + cases._surface("g3", "sphere", "position 2.0, -0.9, -0.3\nradius 0.4", "dense_glass")
        + cases._surface("m2", "sphere", "position 1.2, -1.2, -1.0\nradius 0.5", "mirror")
        + cases._surface("au2", "sphere", "position 0.2, -2.5, 1.2\nradius 0.45", "gold"),
    }


def check(bundle, what, seed=1):
    assert _transmits(bundle), what
    params = pydrt.make_params(W, H, spp=4, max_depth=8, seed=seed, flags=pydrt.FLAG_RECORD_HITS, batch_spp=2)
    r = pydrt.Renderer(bundle, params)
    try:
        assert not (r.stats().path_flags & pydrt.PATH_BVH), what  # the LDS-scene trace kernel: the one that tabulates
        r.render()
        film, log, counts = r.read_film(), r.read_hit_indices(4), cases.stat_counts(r.stats())
    finally:
        r.close()
    px, av, va, olog, ost = cases.oracle_render_device_pow(bundle, params, want_hits=True)
    assert np.array_equal(log, olog), "%s: the hit log differs from the oracle's in %d entries" % (what, int((log != olog).sum()))
    assert counts == cases.stat_counts(ost), "%s: path statistics %r, the oracle's %r" % (what, counts, cases.stat_counts(ost))
    TU.assert_same_film(film, (px, av, va), what + " against the oracle")
    return film, counts


@pytest.mark.gpu
def test_shipped_scenes_with_glass():
    names = shipped()
    assert "cornell_plane_light.scn" in names and "cornell_gold_mirror.scn" in names
    for f in names:
        check(pydrt.load_scene(cases.scene_path(f), W, H), f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(authored()))
def test_authored_scenes(name):
    film, counts = check(pydrt.load_scene_text(authored()[name], W, H), name)
    assert counts[2] > 4 * W * H  # more than one shaded vertex per path: the glass is met


@pytest.mark.gpu
def test_trans_wl_between_two_samples():
    text = authored()["base material water, glass in glass"]
    check(pydrt.load_scene_text(text, W, H, min_wl=380.0, max_wl=720.0, wl_interval=4.0), "4 nm grid", seed=3)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host mode", "device mode"])
@pytest.mark.parametrize("name", ["glass_refract", "base_refract"])
def test_a_live_context_after_a_refraction_spectrum_changes(name, device):
    if device:
        pytest.importorskip("torch")
    p = MU.load(name)["params"]
    with TU.context(name) as r:
        TU.assert_is_before(TU.rendered(r, p), name, "before the update")
        r.reset_film()
        TU.apply(r, name, device=device)
        TU.assert_is_after(TU.rendered(r, p), name, "device mode" if device else "host mode", r=r)
        r.reset_film()
        TU.apply(r, name, to="before", device=device)
        TU.assert_is_before(TU.rendered(r, p), name, "the first scene again")
