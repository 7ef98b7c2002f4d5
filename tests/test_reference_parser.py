"""CPU: the host loader (host/drt_scene.c, host/drt_spectrum.c) against the reference's OWN tokenizer + parse_scene + parse_config
(src/read_scene.c:1-796) and its own CSV resampling (the body of load_csv_file_to_spectrum, :812-end), compiled from the reference's
files by oracle/Makefile. The reference's answers come from tests/reference_records.py: asked live where oracle/_ref was built,
stored everywhere else.

init_scene / init_spd (src/daily_ray_trace.c:79-211) need the Win32 alloc and file calls and are not built; what they do
with the parsed input is restated below in a few lines of Python over the reference's own primitives (rgb_f64_to_spectrum,
generate_blackbody_spectrum, spectrum_normalise, const_spectrum, spectral_mul_by_scalar, create_plane_from_points,
init_camera), and the host loader's finished drt_scene / drt_camera must equal that bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import fuzz_scenes
import oracle_py as O
import pydrt
import reference_records as RR

SPECTRA = os.path.join(cases.REPO, "spectra")
TABLE_CSVS = ["white_rgb_to_spd", "cmf_x", "cmf_y", "cmf_z", "white_rgb_to_spd", "red_rgb_to_spd", "green_rgb_to_spd",
              "blue_rgb_to_spd", "cyan_rgb_to_spd", "magenta_rgb_to_spd", "yellow_rgb_to_spd"]  # rw, x, y, z, white, r, g, b, c, m, y
SPD_FIELDS = ("emission_spd", "diffuse_spd", "glossy_spd", "mirror_spd", "refract_spd", "extinct_spd")
LEGACY_SCENES = ("init_cornell.scn", "cornell_large_box.scn", "cornell_downward.scn", "first_scene.scn", "example_scene.scn")


def ref_tables(n, min_wl, interval):
    """init_spd_tables (src/spectrum.c:1-47): the 11 tables through the reference's CSV resampling."""
    R = O.ref_lib()
    R.ref_set_grid(n, min_wl, interval)
    t = np.zeros((11, n))
    for k, name in enumerate(TABLE_CSVS):
        assert R.ref_csv_to_spectrum(os.path.join(SPECTRA, name + ".csv").encode(), O._ptr(t[k])) == 1
    R.ref_set_tables(O._ptr(t))
    return t


def ref_init_spd(inp, n):
    """init_spd, src/daily_ray_trace.c:79-123, over the reference's own spectral functions. None = no spectrum."""
    R = O.ref_lib()
    s = np.zeros(n)
    if inp.method == O.SPD_METHOD_RGB:
        R.ref_rgb_to_spectrum(O._v3(inp.value), O._ptr(s))
    elif inp.method == O.SPD_METHOD_CSV:
        assert R.ref_csv_to_spectrum(os.path.join(SPECTRA, inp.csv.decode()).encode(), O._ptr(s)) == 1
    elif inp.method == O.SPD_METHOD_BLACKBODY:
        R.ref_blackbody(inp.value[0], O._ptr(s))
        R.ref_spectrum_normalise(O._ptr(s))
    elif inp.method == O.SPD_METHOD_CONST:
        R.ref_const_spectrum(O._ptr(s), inp.value[0])
    else:
        return None
    if inp.has_scale_factor:
        R.ref_spectral_mul_by_scalar(O._ptr(s), inp.scale_factor)
    return s


def reference_scene(text, w, h, grid):
    """What the reference makes of a .scn text: its parser's output through init_spd_tables, init_camera and init_scene
    (restated above), as JSON values -- spectra as digests."""
    R = O.ref_lib()
    rc, cam, mats, surfs = O.ref_parse_scene(text)
    if rc != 0:
        return {"rc": int(rc)}
    n = int(((grid[1] - grid[0]) / grid[2]) + 1.0)  # src/spectrum.c:3
    tables = ref_tables(n, grid[0], grid[2])
    rcam = pydrt.Camera()
    R.ref_init_camera(C.byref(rcam), O._v3(cam[3:6]), O._v3(cam[0:3]), cam[6], cam[7], cam[8], cam[9], cam[10], w, h)
    out = {"rc": 0, "n": n, "tables": RR.digest(tables), "camera": bytes(rcam).hex(), "materials": [], "surfaces": []}
    for m in mats:  # init_scene :133-162 -- the escape material is forced black body
        spds = {}
        for k, field in enumerate(SPD_FIELDS):
            s = ref_init_spd(m.spd[k], n)
            spds[field] = None if s is None else RR.digest(s)
        out["materials"].append({"name": m.name.decode(), "is_black_body": 1 if m.is_escape_material else int(m.is_black_body),
                                 "is_emissive": int(m.is_emissive), "shininess": m.shininess, "roughness": m.roughness,
                                 "bdsfs": list(m.bdsfs)[:m.num_bdsfs], "dir_func": int(m.dir_func) if m.dir_func >= 0 else None,
                                 "spds": spds, "escape": bool(m.is_escape_material), "base": bool(m.is_base_material)})
    ref_names = [m.name for m in mats] + [b""]
    for s in surfs:  # init_scene :172-210 -- planes through create_plane_from_points, material by first name match (else 0)
        su = {"type": int(s.type), "position": list(s.position),
              "material": ref_names.index(s.material_name) if s.material_name in ref_names else 0}
        if s.type == pydrt.GEO_SPHERE:
            su["radius"] = s.radius
        elif s.type == pydrt.GEO_PLANE:
            u, v, nrm = np.zeros(3), np.zeros(3), np.zeros(3)
            R.ref_create_plane(O._v3(s.position), O._v3(s.u), O._v3(s.v), O._ptr(u), O._ptr(v), O._ptr(nrm))
            su["u"], su["v"], su["normal"] = list(u), list(v), list(nrm)
        out["surfaces"].append(su)
    return out


def check_scene_against_reference_parser(key, text, w, h, grid=(380.0, 720.0, 5.0)):
    ref = RR.reference("scene/%s/%dx%d/%g-%g-%g" % ((key, w, h) + tuple(grid)), lambda: reference_scene(text, w, h, grid))
    assert ref["rc"] == 0
    bundle = pydrt.load_scene_text(text, w, h, min_wl=grid[0], max_wl=grid[1], wl_interval=grid[2])
    sc, n = bundle.scene, bundle.S
    assert n == ref["n"] == int(((grid[1] - grid[0]) / grid[2]) + 1.0)  # src/spectrum.c:3
    spds = bundle.spds()
    assert not np.isnan(spds[:11]).any() and RR.digest(spds[:11]) == ref["tables"]  # the host's CSV reader == the reference's, on all 11 tables
    assert (sc.cmf_rw, sc.cmf_x, sc.cmf_y, sc.cmf_z) == (0, 1, 2, 3)
    # camera: init_camera (reference code) on the reference parser's camera block
    assert bytes(bundle.camera).hex() == ref["camera"]
    # materials: init_scene :133-162 -- parsed + 1 trailing all-zero material, escape forced black body
    mats = ref["materials"]
    assert sc.num_materials == len(mats) + 1
    names = bundle.material_names()
    base = escape = None
    for i, m in enumerate(mats):
        hm = sc.materials[i]
        assert names[i] == m["name"]
        assert hm.is_black_body == m["is_black_body"]
        assert hm.is_emissive == m["is_emissive"]
        assert hm.shininess == m["shininess"] and hm.roughness == m["roughness"]
        assert hm.num_bdsfs == len(m["bdsfs"])
        assert list(hm.bdsfs)[:hm.num_bdsfs] == m["bdsfs"]
        if m["dir_func"] is not None:
            assert hm.dir_func == m["dir_func"]
        for field in SPD_FIELDS:
            want = m["spds"][field]
            idx = getattr(hm, field)
            if want is None:
                assert idx == -1, (m["name"], field)
            else:
                assert idx >= 11 and not np.isnan(spds[idx]).any() and RR.digest(spds[idx]) == want, (m["name"], field)
        if m["escape"]:
            escape = i
        if m["base"]:
            base = i
    last = sc.materials[len(mats)]
    assert (last.is_black_body, last.is_emissive, last.num_bdsfs) == (0, 0, 0)
    assert all(getattr(last, f) == -1 for f in SPD_FIELDS)
    assert sc.base_material == base and sc.escape_material == escape
    # surfaces: init_scene :172-210 -- planes through create_plane_from_points, material by first name match (else 0)
    assert sc.num_surfaces == len(ref["surfaces"])
    for i, s in enumerate(ref["surfaces"]):
        hs = sc.surfaces[i]
        assert hs.type == s["type"] and list(hs.position) == s["position"]
        if s["type"] == pydrt.GEO_SPHERE:
            assert hs.radius == s["radius"]
        elif s["type"] == pydrt.GEO_PLANE:
            assert list(hs.u) == s["u"] and list(hs.v) == s["v"] and list(hs.normal) == s["normal"]
        assert hs.material == s["material"]
    return bundle


def test_cornell_plane_light_loads_like_the_reference():
    """The one shipped scene the reference's parser accepts, at the bench size and at config.cfg's."""
    text = open(cases.scene_path("cornell_plane_light.scn")).read()
    check_scene_against_reference_parser("cornell_plane_light.scn", text, 1024, 1024)
    check_scene_against_reference_parser("cornell_plane_light.scn", text, 800, 600)


def test_authored_modern_scenes_load_like_the_reference():
    """The scenes this repo authored in the current grammar (gold mirror, lights, thin lens): <= 16 materials and surfaces."""
    for name, grid in (("cornell_gold_mirror.scn", (380.0, 720.0, 5.0)), ("test_lights.scn", (380.0, 720.0, 5.0)),
                       ("test_lens.scn", (380.0, 720.0, 10.0)), ("cornell_plane_light.scn", (380.0, 720.0, 4.0))):
        text = open(cases.scene_path(name)).read()
        if text.count("Material") > 16 or text.count("Surface") > 16:
            continue
        check_scene_against_reference_parser(name, text, 64, 48, grid)


@pytest.mark.parametrize("seed", fuzz_scenes.FUZZ_SEEDS[:24])
def test_random_scenes_load_like_the_reference(seed):
    """Random scenes in the .scn grammar (every BDSF, sampler, SPD method, light kind) that fit the reference's fixed arrays."""
    text = fuzz_scenes.random_scene_text(seed)
    if text.count("Material") > 16 or text.count("Surface") > 16:
        pytest.skip("more than 16 materials or surfaces: the reference's parser arrays overflow (src/read_scene.h:85-86)")
    check_scene_against_reference_parser("fuzz_%d" % seed, text, 40, 30)


def test_legacy_scenes_are_rejected_by_the_reference_parser():
    """the five legacy-syntax scenes end in parse_error() -> exit(-1) in the reference (the host loads them
    through its superset grammar: tests/test_host.py)."""
    rcs = RR.reference("legacy_scene_rc", lambda: {name: int(O.ref_parse_scene(open(cases.scene_path(name)).read())[0])
                                                   for name in LEGACY_SCENES})
    for name in LEGACY_SCENES:
        assert rcs[name] != 0, name
        assert pydrt.load_scene(cases.scene_path(name), 16, 16).scene.num_surfaces > 0, name


def test_config_cfg_parses_like_the_reference():
    """parse_config on the reference's own config.cfg -- this repository's config.cfg with Windows `\\` separators: `/` is not a
    word character of the reference's tokenizer (src/read_scene.c:76-79) -- gives the same 1136-byte config_arguments as the host's
    parse_config on either form, path separators aside (the POSIX host stores `/`)."""
    H = pydrt.host_lib()
    H.parse_config.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]
    H.parse_config.restype = None
    text = open(os.path.join(cases.REPO, "config.cfg"), "rb").read()
    ref_text = text.replace(b"/", b"\\")
    ref = RR.reference("config_cfg", lambda: (lambda rc, raw: {"rc": int(rc), "raw": raw.hex()})(*O.ref_parse_config(ref_text)))
    raw = bytes.fromhex(ref["raw"])
    assert ref["rc"] == 0 and len(raw) == 1136
    for t in (ref_text, text):
        buf = C.create_string_buffer(1136)
        tb = C.create_string_buffer(t, len(t) + 1)
        H.parse_config(tb, len(t), buf)
        assert buf.raw == raw.replace(b"\\", b"/")
    assert raw[:16] == np.array([4, 4, 800, 600], dtype=np.uint32).tobytes()  # num_pixel_samples, depth, width, height


def test_csv_resampling_matches_the_reference_on_every_table():
    """load_csv_file_to_spectrum's body on every spectra/*.csv (nm and um files, NUL-terminated ones, the magenta table with
    its duplicated rows) on three grids: the host's reader gives the same samples bit for bit."""
    H = pydrt.host_lib()
    files = [f for f in sorted(os.listdir(SPECTRA)) if f.endswith(".csv")]
    for (lo, hi, step) in ((380.0, 720.0, 5.0), (380.0, 720.0, 4.0), (400.0, 700.0, 2.5)):
        n = int(((hi - lo) / step) + 1.0)

        def live():
            R = O.ref_lib()
            R.ref_set_grid(n, lo, step)
            out = {}
            for f in files:
                a = np.zeros(n)
                assert R.ref_csv_to_spectrum(os.path.join(SPECTRA, f).encode(), O._ptr(a)) == 1
                out[f] = RR.digest(a)
            return out
        ref = RR.reference("csv/%g-%g-%g" % (lo, hi, step), live)
        assert sorted(ref) == files
        for f in files:
            b = np.zeros(n)
            assert H.drt_host_csv_to_spectrum(os.path.join(SPECTRA, f).encode(), lo, step, n, O._ptr(b)) == 1
            assert RR.digest(b) == ref[f], (f, lo, step)
