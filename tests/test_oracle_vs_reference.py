"""CPU: the oracle against the REAL reference code, bit for bit, at sizes the golden files do not hold (incl. BASELINE config 1 in
full: 256x256, 4 spp, depth 4). The reference's answers come from tests/reference_records.py: asked live where oracle/_ref was
built, stored (digests of its films and hit logs) everywhere else."""
import ctypes as C

import numpy as np
import pytest

import cases
import fuzz_scenes
import oracle_py as O
import pydrt
import reference_records as RR


def ref_film(key, bundle, params):
    """digest of the reference's film (pixels, avgs, vars) of the tile"""
    return RR.reference("film/" + key, lambda: {"film": RR.digest(*O.ref_render_tile(bundle, params))}, bundle)["film"]


def ref_film_and_hits(key, bundle, params):
    """the reference's film digest and, for a pinhole camera (the harness's hit log replays pinhole paths only, oracle/ref_harness.c),
    the digest of its hit-index log and whether replaying cast_ray gave the bits of its real cast_ray (NaN for NaN)"""
    def live():
        out = {"film": RR.digest(*O.ref_render_tile(bundle, params))}
        if bundle.camera.aperture_radius == 0.0:
            hits, replay, real = O.ref_trace_hits(bundle, params)
            out.update(hits=RR.digest(hits), replay_is_real=fuzz_scenes.same(replay, real))
        return out
    return RR.reference("film_hits/" + key, live, bundle)


@pytest.mark.parametrize("name", list(cases.RENDER_CASES))
def test_film_bit_identical(name):
    bundle, params = cases.load_case(name)
    op, oa, ov, _, _ = O.oracle_render_tile(bundle, params, math_mode=O.MATH_REFERENCE)
    assert not np.isnan(op).any() and not np.isnan(oa).any()
    assert RR.digest(op, oa, ov) == ref_film(name, bundle, params)


@pytest.mark.parametrize("name", list(cases.NAN_CASES))
def test_film_bit_identical_nan_for_nan(name):
    """example_scene.scn: a camera without fov / fdepth / flength makes every ray NaN (cases.NAN_CASES); the reference's film is
    NaN in every wavelength and the filter sums still count the samples -- and so is the oracle's, NaN for NaN."""
    bundle, params = cases.load_case(name)
    op, oa, ov, _, st = O.oracle_render_tile(bundle, params, math_mode=O.MATH_REFERENCE)
    assert RR.digest(op, oa, ov) == ref_film(name, bundle, params)  # NaN for NaN: the film below is the reference's
    assert np.isnan(op[:, :bundle.S]).all() and np.all(op[:, bundle.S] == float(params.spp)) and st.shaded_vertices == 0


def test_config1_full_size_bit_identical():
    """BASELINE.json configs[0]: init_cornell.scn 256x256, 4 spp, depth 4, single thread, fixed seed."""
    bundle = pydrt.load_scene(cases.scene_path("init_cornell.scn"), 256, 256)
    params = pydrt.make_params(256, 256, spp=4, max_depth=4, seed=1)
    op, oa, ov, _, st = O.oracle_render_tile(bundle, params, math_mode=O.MATH_REFERENCE)
    assert st.paths == 256 * 256 * 4
    assert not (np.isnan(op).any() or np.isnan(oa).any() or np.isnan(ov).any())
    assert RR.digest(op, oa, ov) == ref_film("config1_256x256", bundle, params)


def test_hit_sequences_and_replay_identity():
    """The hit-index log comes from replaying cast_ray with the reference's own functions; the replay must give
    the bits of the reference's real cast_ray, and the oracle must log the same surfaces."""
    bundle, params = cases.load_case("plane_light_16")

    def live():
        hits, replay, real = O.ref_trace_hits(bundle, params)
        return {"hits": RR.digest(hits), "replay_is_real": bool(np.array_equal(replay, real))}
    ref = RR.reference("hits/plane_light_16", live, bundle)
    assert ref["replay_is_real"]
    _, _, _, ohits, _ = O.oracle_render_tile(bundle, params, want_hits=True, math_mode=O.MATH_REFERENCE)
    assert RR.digest(ohits) == ref["hits"]
    assert (ohits[:, 0] >= -1).all() and (ohits == -1).any() and (ohits >= 0).any()


def test_traversal_order_independence_of_the_reference():
    """with per-path seeding the reference's own sample_scene gives the same spectrum whether the
    pixels are visited forward or in reverse -- and so does the oracle's, visited in reverse."""
    bundle, params = cases.load_case("plane_light_16")
    S = bundle.S
    filt = C.c_double()
    order = [(x, y) for y in range(16) for x in range(16)]

    def visit(sample_scene, seq):
        buf = np.zeros((16 * 16, S))
        for (x, y) in seq:
            sample_scene(x, y, buf[y * 16 + x].ctypes.data_as(C.POINTER(C.c_double)))
        return buf

    def live():
        R = O.ref_lib()
        R.ref_set_scene(C.byref(bundle.scene))
        f = lambda x, y, out: R.ref_sample_scene(C.byref(bundle.camera), C.byref(params), x, y, 2, out, C.byref(filt))
        fwd, rev = visit(f, order), visit(f, order[::-1])
        assert not np.isnan(fwd).any()
        return {"forward": RR.digest(fwd), "reverse": RR.digest(rev)}
    ref = RR.reference("sample_scene_order/plane_light_16", live, bundle)
    assert ref["forward"] == ref["reverse"]
    L = O.oracle_lib()
    O.set_math_mode(O.MATH_REFERENCE)
    g = lambda x, y, out: L.drt_oracle_sample_scene(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(params), x, y, 2, out,
                                                    C.byref(filt), None)
    rev = visit(g, order[::-1])
    assert not np.isnan(rev).any() and RR.digest(rev) == ref["forward"]


@pytest.mark.parametrize("seed", fuzz_scenes.FUZZ_SEEDS)
def test_random_scenes_bit_identical(seed):
    """Random scenes (tests/fuzz_scenes.py: every BDSF and sampler, mixed lights, nested media, lens cameras): the oracle in
    reference arithmetic against the compiled reference, film and hit indices, NaN for NaN."""
    bundle, params = fuzz_scenes.load(seed, pydrt)
    ref = ref_film_and_hits("fuzz_%d" % seed, bundle, params)
    op, oa, ov, ohits, _ = O.oracle_render_tile(bundle, params, want_hits=True, math_mode=O.MATH_REFERENCE)
    assert RR.digest(op, oa, ov) == ref["film"]
    if bundle.camera.aperture_radius == 0.0:
        assert ref["replay_is_real"] and RR.digest(ohits) == ref["hits"]


@pytest.mark.parametrize("name", list(cases.degenerate_scenes()))
def test_degenerate_geometry_and_materials_bit_identical(name):
    """tests/cases.py degenerate_scenes() -- coincident surfaces, radius 0 and negative, planes with parallel or zero edges, a 900 km
    sphere, roughness 0 (NaN films), the camera inside glass: whatever the reference's arithmetic makes of them, the oracle in reference
    arithmetic makes the same, film and hit indices, NaN for NaN."""
    bundle = pydrt.load_scene_text(cases.degenerate_scenes()[name], 24, 24)
    params = pydrt.make_params(24, 24, spp=4, max_depth=8, seed=3)
    ref = ref_film_and_hits("degenerate_" + name, bundle, params)
    op, oa, ov, ohits, _ = O.oracle_render_tile(bundle, params, want_hits=True, math_mode=O.MATH_REFERENCE)
    assert RR.digest(op, oa, ov) == ref["film"]
    if bundle.camera.aperture_radius == 0.0:
        assert ref["replay_is_real"] and RR.digest(ohits) == ref["hits"]


@pytest.mark.parametrize("S", list(fuzz_scenes.FUZZ_GRIDS))
def test_random_scenes_on_other_wavelength_grids_bit_identical(S):
    """The same comparison on grids from 2 to 256 wavelengths (incl. grids that end below the 630 nm the dielectric
    sampler looks up, src/daily_ray_trace.c:381)."""
    bundle, params = fuzz_scenes.load(3 + S % 7, pydrt, fuzz_scenes.FUZZ_GRIDS[S])
    assert bundle.S == S
    op, oa, ov, _, _ = O.oracle_render_tile(bundle, params, math_mode=O.MATH_REFERENCE)
    assert RR.digest(op, oa, ov) == ref_film("fuzz_grid_%d" % S, bundle, params)


def test_host_scene_build_pieces_on_random_inputs():
    """The product's host code (host/drt_scene.c, host/drt_spectrum.c) against the reference's own init_camera,
    rgb_f64_to_spectrum, generate_blackbody_spectrum and spectrum_to_rgb on random inputs, on the reference grid and on a
    10 nm one. rgb -> spectrum is bit for bit; the camera and the black body go through tan / expl / powl and are held to 1e-13."""
    H = pydrt.host_lib()
    f64p = C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(f64p)
    H.drt_host_spectrum_to_rgb.argtypes = [f64p, C.c_uint32, C.c_double, f64p, f64p]
    r = np.random.default_rng(99)
    for wl_interval in (5.0, 10.0):
        bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 32, 32, wl_interval=wl_interval)
        S = bundle.S
        sc = bundle.scene
        block = np.ctypeslib.as_array(sc.spds, shape=(sc.num_spds, S))
        tables = np.ascontiguousarray(np.stack([block[sc.cmf_rw], block[sc.cmf_x], block[sc.cmf_y], block[sc.cmf_z]] +
                                               [block[sc.cmf_z + 1 + k] for k in range(7)]))  # host/drt_scene.c: 11 adjacent rows
        rgb_tables = np.ascontiguousarray(tables[4:11])
        rgbs, temps, spds = [], [], []
        for _ in range(200):
            rgb = r.uniform(0.0, 1.2, 3)
            if r.random() < 0.3:
                rgb[int(r.integers(0, 3))] = rgb[int(r.integers(0, 3))]  # ties between channels pick the branches' edges
            rgbs.append(rgb)
            temps.append(float(r.uniform(800.0, 12000.0)))
            spds.append(r.uniform(0.0, 3.0, S))
        host = {"rgb_to_spectrum": np.zeros((200, S)), "blackbody": np.zeros((200, S)), "spectrum_to_rgb": np.zeros((200, 3))}
        for i in range(200):
            H.drt_host_rgb_to_spectrum(p(rgb_tables), S, p(rgbs[i].copy()), p(host["rgb_to_spectrum"][i]))
            H.drt_host_blackbody_spectrum(380.0, wl_interval, S, temps[i], p(host["blackbody"][i]))
            H.drt_host_spectrum_to_rgb(p(np.ascontiguousarray(tables[0:4])), S, wl_interval, p(spds[i]), p(host["spectrum_to_rgb"][i]))

        def live():
            R = O.ref_lib()
            R.ref_set_grid(S, 380.0, wl_interval)
            R.ref_set_tables(p(tables))
            out = {k: np.zeros_like(v) for k, v in host.items()}
            for i in range(200):
                R.ref_rgb_to_spectrum(p(rgbs[i].copy()), p(out["rgb_to_spectrum"][i]))
                R.ref_blackbody(temps[i], p(out["blackbody"][i]))
                R.ref_spectrum_to_rgb(p(spds[i].copy()), p(out["spectrum_to_rgb"][i]))
            return out
        grid = "%gnm" % wl_interval
        exact = RR.reference("host_pieces/" + grid, lambda: {k: RR.digest(v) for k, v in live().items() if k != "blackbody"})
        assert not np.isnan(host["rgb_to_spectrum"]).any() and not np.isnan(host["spectrum_to_rgb"]).any()
        assert RR.digest(host["rgb_to_spectrum"]) == exact["rgb_to_spectrum"]
        assert RR.digest(host["spectrum_to_rgb"]) == exact["spectrum_to_rgb"]
        np.testing.assert_allclose(host["blackbody"], RR.reference_array("blackbody_" + grid, lambda: live()["blackbody"]), rtol=1e-13)
    inputs = []
    for _ in range(300):
        pos = r.uniform(-10, 10, 3); tgt = r.uniform(-10, 10, 3)
        roll, fov = float(r.uniform(-180, 180)), float(r.uniform(10, 140))
        fdepth, flength, aperture = float(r.uniform(0.5, 20)), float(r.uniform(0.05, 2)), float(r.choice([0.0, r.uniform(0.01, 0.5)]))
        w, h = int(r.integers(1, 3000)), int(r.integers(1, 3000))
        inputs.append((pos, tgt, roll, fov, fdepth, flength, aperture, w, h))
    cams = lambda init: np.stack([np.frombuffer(bytes(init(*a)), dtype=np.float64) for a in inputs])

    def ref_init_camera(pos, tgt, *rest):
        cam = pydrt.Camera()
        O.ref_lib().ref_init_camera(C.byref(cam), p(pos.copy()), p(tgt.copy()), *rest)
        return cam
    np.testing.assert_allclose(cams(pydrt.init_camera), RR.reference_array("init_camera", lambda: cams(ref_init_camera)), rtol=1e-13, atol=1e-13)


@pytest.mark.skipif(not O.ref_available(), reason="the stub is compiled against the reference's own headers: only in oracle/_ref")
@pytest.mark.parametrize("name", ["plane_light_16", "gold_mirror", "lights", "init_cornell"])
def test_integration_stub_round_trips_a_scene(name):
    """INTEGRATION.md's reference-side binding (include/drt_reference_binding.inc, compiled here against the reference's own
    headers as a maintainer would add it to src/daily_ray_trace.c): the reference's scene_data / camera_data / config go in,
    the boundary structs of include/drt_hip.h come out and reach drt_render_tile -- here the oracle behind that signature.
    The film must be, bit for bit, the film of the scene the boundary structs came from, i.e. flattening loses nothing."""
    bundle, params = cases.load_case(name)
    R = O.ref_lib()
    R.ref_set_scene(C.byref(bundle.scene))
    S = bundle.S
    n = int(params.width) * int(params.height)
    seen = {}

    def render_tile(sc, cam, p, px, av, va, st):
        sc, cam, p = sc.contents, cam.contents, p.contents
        seen.update(num_spds=int(sc.num_spds), num_materials=int(sc.num_materials), num_surfaces=int(sc.num_surfaces),
                    cmf=(int(sc.cmf_rw), int(sc.cmf_x), int(sc.cmf_y), int(sc.cmf_z)), flags=int(p.flags), spp=int(p.spp),
                    base=int(sc.base_material), escape=int(sc.escape_material))
        b2 = pydrt.SceneBundle(sc, cam)
        opx, oav, ova, _, ost = O.oracle_render_tile(b2, p, math_mode=O.MATH_REFERENCE)
        for dst, src in ((px, opx), (av, oav), (va, ova)):
            C.memmove(dst, src.ctypes.data, src.nbytes)
        st.contents.paths = ost.paths
        return 0

    px, av, va = np.zeros((n, S + 1)), np.zeros((n, S)), np.zeros((n, S))
    p1 = pydrt.make_params(int(params.width), int(params.height), spp=int(params.spp), max_depth=int(params.max_depth), seed=1,
                           pixel_scheme=int(params.pixel_scheme))
    rc = R.ref_run_binding(C.byref(bundle.camera), C.byref(p1), O.RENDER_TILE_FN(render_tile), O._ptr(px), O._ptr(av), O._ptr(va))
    assert rc == 0
    sc = bundle.scene
    assert seen["num_materials"] == sc.num_materials and seen["num_surfaces"] == sc.num_surfaces
    assert seen["num_spds"] == 11 + sc.num_spds + 1 and seen["cmf"] == (0, 1, 2, 3)  # tables, the scene's rows, the zero row
    assert seen["base"] == sc.base_material and seen["escape"] == sc.escape_material
    assert seen["flags"] == pydrt.FLAG_FILM_ZERO and seen["spp"] == int(params.spp)
    opx, oav, ova, _, _ = O.oracle_render_tile(bundle, p1, math_mode=O.MATH_REFERENCE)
    assert np.array_equal(px, opx) and np.array_equal(av, oav) and np.array_equal(va, ova)
    # and the reference's own pixel loop on the same scene agrees (the stub replaces exactly that loop)
    rp, ra, rv = O.ref_render_tile(bundle, p1)
    assert np.array_equal(px, rp) and np.array_equal(av, ra) and np.array_equal(va, rv)
    # a failing launcher takes the stub's exit(-1) path
    assert R.ref_run_binding(C.byref(bundle.camera), C.byref(p1), O.RENDER_TILE_FN(lambda *a: -7), O._ptr(px), O._ptr(av), O._ptr(va)) != 0


def test_integration_md_shows_the_compiled_stub():
    """The code block in INTEGRATION.md is the file that is compiled above, character for character."""
    import os
    stub = open(os.path.join(cases.REPO, "include", "drt_reference_binding.inc")).read().strip()
    doc = open(os.path.join(cases.REPO, "INTEGRATION.md")).read()
    assert stub in doc
