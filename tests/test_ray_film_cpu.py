"""CPU: what the ray films (drt_bind_rays) need no device for -- the table struct in the header, a C compiler's
view of it and pydrt's; the two ray generators of the host library; the drt_render host's DRT_PROJECTION refusals; and, with the
oracle alone in DEVICE arithmetic, the premises the GPU tests' ground truth rests on (tests/ray_film_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import oracle_py as O
import pydrt
import ray_film_cases as R

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")
FIELDS = [("origins", 0), ("dirs", 8), ("weights", 16), ("n_layers", 24), ("flags", 28)]


def test_the_header_declares_the_struct_and_the_calls():
    header = open(os.path.join(REPO, "include", "drt_hip.h")).read()
    body = re.search(r"typedef struct drt_ray_table[^{]*\{(.*?)\}\s*drt_ray_table;", header, re.S).group(1)
    names = re.findall(r"\*?(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in FIELDS]
    assert re.search(r"DRT_PATH_RAYS\s*=\s*4u", header)
    for call in ("drt_bind_rays", "drt_group_bind_rays"):
        assert re.search(r"\bint %s\(" % call, header), call
        assert call in pydrt.HIP_SYMBOLS
    host = open(os.path.join(REPO, "daily-ray-trace_amd", "host", "drt_host.h")).read()
    for call in ("drt_host_rays_equirect", "drt_host_rays_ortho"):
        assert re.search(r"\bint %s\(" % call, host), call


def test_a_c_compiler_and_pydrt_agree_on_the_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "drt_hip.h"\nint main(void)\n{\n    printf("sizeof %zu\\n", sizeof(drt_ray_table));\n'
                   + "".join('    printf("%s %%zu\\n", offsetof(drt_ray_table, %s));\n' % (n, n) for n, _ in FIELDS)
                   + '    printf("path_rays %u\\n", (unsigned)DRT_PATH_RAYS);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["sizeof"]) == 32
    assert [(n, int(out[n])) for n, _ in FIELDS] == FIELDS
    T = pydrt.RayTable
    assert C.sizeof(T) == 32
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == FIELDS
    assert int(out["path_rays"]) == pydrt.PATH_RAYS == 4


# ------------------------------------------------------------------------------------------------
CAMERAS = [((0.0, 0.5, 7.0), (0.0, 0.0, 0.0), 10.0), ((1.5, -1.0, 4.0), (-1.0, 0.5, -1.0), 0.0), ((-2.0, 1.5, 5.0), (1.0, -1.0, 0.0), -25.0),
           ((0.0, 0.0, 30.0), (0.0, 0.0, -20.0), 90.0)]
# exactly orthonormal bases (forward, right, up) for the checks of where each pixel looks: init_camera's `up` of a rolled camera is
# only nearly at right angles to `forward`, as the reference's is
FRAMES = [((0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ((0.6, 0.0, -0.8), (0.8, 0.0, 0.6), (0.0, 1.0, 0.0)),
          ((0.0, 0.6, 0.8), (1.0, 0.0, 0.0), (0.0, 0.8, -0.6))]
SIZES = [(1, 1), (7, 5), (32, 16), (33, 17)]


def _len(v):
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def _frame_camera(frame, position=(0.25, -1.5, 3.0)):
    c = pydrt.Camera()
    for k in range(3):
        c.forward[k], c.right[k], c.up[k], c.aperture_position[k] = frame[0][k], frame[1][k], frame[2][k], position[k]
    return c


@pytest.mark.parametrize("cam", range(len(CAMERAS)))
@pytest.mark.parametrize("w, h", SIZES)
def test_equirect_rays_are_unit_vectors_from_the_cameras_position(cam, w, h):
    pos, tgt, roll = CAMERAS[cam]
    c = pydrt.init_camera(pos, tgt, roll, 70.0, 6.0, 0.3, 0.0, w, h)
    o, d = pydrt.equirect_rays(c, w, h)
    assert o.shape == d.shape == (h, w, 3)
    assert np.all(o == np.array(list(c.aperture_position)))
    assert np.max(np.abs(_len(d) - 1.0)) <= 1e-15
    if w % 2 and h % 2:
        # the centre pixel looks along forward: forward as it stands, normalised once more (two roundings a component at most)
        assert np.max(np.abs(d[h // 2, w // 2] - np.array(list(c.forward)))) <= 1e-15
    # a SceneBundle is taken for its camera
    assert all(np.array_equal(a, b) for a, b in zip(pydrt.equirect_rays(pydrt.SceneBundle(None, c), w, h), (o, d)))


@pytest.mark.parametrize("frame", range(len(FRAMES)))
@pytest.mark.parametrize("w, h", SIZES)
def test_equirect_rays_run_over_longitude_and_latitude(frame, w, h):
    c = _frame_camera(FRAMES[frame])
    forward, right, up = (np.array(v) for v in FRAMES[frame])
    o, d = pydrt.equirect_rays(c, w, h)
    assert np.max(np.abs(_len(d) - 1.0)) <= 1e-15
    if w % 2 and h % 2:
        assert np.max(np.abs(d[h // 2, w // 2] - forward)) <= 1e-15
    # longitude grows with x towards `right`, latitude with y towards `up`; the columns of a row share their latitude
    lat = ((np.arange(h) + 0.5) / h - 0.5) * np.pi
    lon = ((np.arange(w) + 0.5) / w - 0.5) * 2 * np.pi
    assert np.allclose(d @ up, np.sin(lat)[:, None] * np.ones((1, w)), rtol=0, atol=1e-14)
    assert np.allclose(d @ right, np.cos(lat)[:, None] * np.sin(lon)[None, :], rtol=0, atol=1e-14)
    assert np.allclose(d @ forward, np.cos(lat)[:, None] * np.cos(lon)[None, :], rtol=0, atol=1e-14)


@pytest.mark.parametrize("cam", range(len(CAMERAS)))
@pytest.mark.parametrize("w, h, fw", [(1, 1, 1.0), (7, 5, 3.0), (32, 16, 6.5), (33, 17, 0.25)])
def test_ortho_rays_are_parallel_from_one_plane(cam, w, h, fw):
    pos, tgt, roll = CAMERAS[cam]
    c = pydrt.init_camera(pos, tgt, roll, 70.0, 6.0, 0.3, 0.0, w, h)
    o, d = pydrt.ortho_rays(c, w, h, fw)
    forward, right, up, ap = (np.array(list(v)) for v in (c.forward, c.right, c.up, c.aperture_position))
    assert o.shape == d.shape == (h, w, 3)
    assert np.all(d == forward)  # all equal: forward as it stands
    # coplanar: the plane of `right` and `up` through the aperture position (the origins' own size times a few roundings)
    scale = np.max(np.abs(ap)) + max(fw, fw * h / w)
    assert np.max(np.abs((o - ap) @ np.cross(right, up))) <= 1e-14 * scale


@pytest.mark.parametrize("frame", range(len(FRAMES)))
@pytest.mark.parametrize("w, h, fw", [(1, 1, 1.0), (7, 5, 3.0), (32, 16, 6.5), (33, 17, 0.25)])
def test_ortho_origins_are_the_pixel_centres_of_the_rectangle(frame, w, h, fw):
    c = _frame_camera(FRAMES[frame])
    forward, right, up = (np.array(v) for v in FRAMES[frame])
    o, d = pydrt.ortho_rays(c, w, h, fw)
    rel = o - np.array(list(c.aperture_position))
    scale = 3.0 + max(fw, fw * h / w)
    assert np.all(d == forward) and np.max(np.abs(rel @ forward)) <= 1e-14 * scale
    assert np.allclose(rel @ right, (((np.arange(w) + 0.5) / w - 0.5) * fw)[None, :] * np.ones((h, 1)), rtol=0, atol=1e-14 * scale)
    assert np.allclose(rel @ up, (((np.arange(h) + 0.5) / h - 0.5) * fw * h / w)[:, None] * np.ones((1, w)), rtol=0, atol=1e-14 * scale)


def test_the_generators_refuse_what_they_cannot_make():
    c = pydrt.init_camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), 0.0, 60.0, 6.0, 0.3, 0.0, 4, 4)
    for fw in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pydrt.ortho_rays(c, 4, 4, fw)
    L = pydrt.host_lib()
    buf = np.full((4, 4, 3), -7.25)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.drt_host_rays_equirect(C.byref(c), 0, 4, p, p) != 0 and L.drt_host_rays_equirect(C.byref(c), 4, 4, None, p) != 0
    assert L.drt_host_rays_ortho(C.byref(c), 4, 0, 1.0, p, p) != 0 and L.drt_host_rays_ortho(None, 4, 4, 1.0, p, p) != 0
    assert np.all(buf == -7.25)


# ------------------------------------------------------------------------------------------------
def _run_host(tmp_path, env):
    cfg = open(os.path.join(REPO, "config.cfg")).read()
    (tmp_path / "config.cfg").write_text(cfg)
    os.symlink(os.path.join(REPO, "scenes"), tmp_path / "scenes")
    os.symlink(os.path.join(REPO, "spectra"), tmp_path / "spectra")
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full.update(env)
    full["HIP_VISIBLE_DEVICES"] = "-1"
    return subprocess.run([BIN, "config.cfg"], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


@pytest.mark.parametrize("env, named", [
    ({"DRT_PROJECTION": ""}, "DRT_PROJECTION"), ({"DRT_PROJECTION": "fisheye"}, "DRT_PROJECTION"), ({"DRT_PROJECTION": "Equirect"}, "DRT_PROJECTION"),
    ({"DRT_PROJECTION": "equirect "}, "DRT_PROJECTION"), ({"DRT_PROJECTION": "1"}, "DRT_PROJECTION"),
    ({"DRT_PROJECTION": "ortho"}, "DRT_ORTHO_WIDTH"), ({"DRT_PROJECTION": "ortho", "DRT_ORTHO_WIDTH": ""}, "DRT_ORTHO_WIDTH"),
    ({"DRT_PROJECTION": "ortho", "DRT_ORTHO_WIDTH": "0"}, "DRT_ORTHO_WIDTH"), ({"DRT_PROJECTION": "ortho", "DRT_ORTHO_WIDTH": "-2.5"}, "DRT_ORTHO_WIDTH"),
    ({"DRT_PROJECTION": "ortho", "DRT_ORTHO_WIDTH": "nan"}, "DRT_ORTHO_WIDTH"), ({"DRT_PROJECTION": "ortho", "DRT_ORTHO_WIDTH": "inf"}, "DRT_ORTHO_WIDTH"),
    ({"DRT_PROJECTION": "ortho", "DRT_ORTHO_WIDTH": "6m"}, "DRT_ORTHO_WIDTH"),
    ({"DRT_PROJECTION": "equirect", "DRT_ORTHO_WIDTH": "6"}, "DRT_ORTHO_WIDTH"), ({"DRT_ORTHO_WIDTH": "6"}, "DRT_ORTHO_WIDTH"),
    ({"DRT_PROJECTION": "equirect", "DRT_FEATURES": "1"}, "DRT_FEATURES"), ({"DRT_PROJECTION": "ortho", "DRT_ORTHO_WIDTH": "6", "DRT_MATTES": "1"}, "DRT_MATTES"),
    ({"DRT_PROJECTION": "equirect", "DRT_PICK": "1,2"}, "DRT_PICK"),
], ids=lambda v: "+".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_the_host_refuses_a_bad_projection_before_any_device_call(tmp_path, env, named):
    """Exit status nonzero, the variable named on stderr, and no device opened: HIP_VISIBLE_DEVICES hides every device, so a run that got
    as far as the launcher would fail there with the launcher's message instead."""
    r = _run_host(tmp_path, env)
    assert r.returncode != 0
    assert named in r.stderr, r.stderr
    assert "HIP launcher" not in r.stderr and "Rendering" not in r.stdout


@pytest.mark.parametrize("env", [{"DRT_PROJECTION": "equirect"}, {"DRT_PROJECTION": "ortho", "DRT_ORTHO_WIDTH": "6.5"},
                                 {"DRT_PROJECTION": "equirect", "DRT_ADAPTIVE_ERROR": "0.05", "DRT_FEATURES": "0", "DRT_MATTES": "0"}],
                         ids=lambda v: "+".join("%s=%s" % kv for kv in v.items()))
def test_a_good_projection_gets_as_far_as_the_launcher(tmp_path, env):
    r = _run_host(tmp_path, env)
    assert r.returncode != 0 and "DRT_PROJECTION" not in r.stderr and "DRT_ORTHO_WIDTH" not in r.stderr and "HIP launcher" in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------------
# The premises of the GPU tests' ground truth, on the oracle in DEVICE arithmetic.
def _same_film(a, b):
    return all(cases.same_bits(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("name", R.CAMERA_PARITY)
def test_a_centre_scheme_pinhole_gives_every_sample_the_same_ray_and_draws_nothing(name):
    bundle, p = R.load(name)
    assert float(bundle.camera.aperture_radius) == 0.0 and int(p.pixel_scheme) == pydrt.FILM_SAMPLE_CENTER
    w, h = int(p.width), int(p.height)
    s0, s1 = R.centre_rays(bundle, w, h, 0, p), R.centre_rays(bundle, w, h, 1, p)
    table = R.camera_table(name)
    for a, b, t in zip(s0, s1, table):
        assert cases.same_bits(a, b) and cases.same_bits(a, t)
    assert not np.isnan(table[1]).any() and np.all(table[2] > 0.0)  # a pinhole's rays leave the film towards the aperture: forward of it


@pytest.mark.parametrize("name", R.CAMERA_PARITY)
def test_sample_by_sample_accumulation_equals_one_call(name):
    bundle, p = R.load(name)
    p3 = R.params_like(p, spp=3, flags=0)
    once = O.oracle_render_tile(bundle, p3, math_mode=O.MATH_DEVICE)
    by_samples = R.render_by_samples(lambda b, q, film: O.oracle_render_tile(b, q, math_mode=O.MATH_DEVICE, film=film), [bundle], p3, n_layers=1)
    assert _same_film(once, by_samples)
    assert np.any(once[0][:, :-1] != 0.0)


@pytest.mark.parametrize("scene", R.STITCH_SCENES)
def test_every_tile_of_the_stitched_tables_sees_something(scene):
    st = R.stitch(scene)
    o, d, w = st["table"]
    assert o.shape == d.shape == (R.STITCH_H, R.STITCH_W, 3) and w.shape == (R.STITCH_H, R.STITCH_W)
    # three different cameras: the rows' origins and the headings differ from tile to tile
    apertures = [tuple(b.camera.aperture_position) for b in st["cameras"]]
    forwards = [tuple(b.camera.forward) for b in st["cameras"]]
    assert len(set(apertures)) == 3 and len(set(forwards)) == 3
    for k, (b, tp) in enumerate(zip(st["cameras"], st["tile_params"])):
        assert (int(tp.y0), int(tp.tile_h), int(tp.tile_w)) == (R.STITCH_ROWS * k, R.STITCH_ROWS, R.STITCH_W)
        px = O.oracle_render_tile(b, tp, math_mode=O.MATH_DEVICE)[0]
        share = float((px[:, :-1] != 0.0).any(axis=1).mean())
        print("%s tile %d: %.1f %% of the pixels hold light" % (scene, k, 100 * share))
        assert share >= 0.10
        assert not np.isnan(px).any()


def test_the_layer_tables_are_two_cameras():
    ly = R.layers()
    o, d, w = ly["table"]
    assert o.shape == (2, R.STITCH_H, R.STITCH_W, 3) and w.shape == (2, R.STITCH_H, R.STITCH_W)
    assert not np.array_equal(o[0], o[1]) and not np.array_equal(d[0], d[1])
    assert int(ly["params"].spp) == 5


# ------------------------------------------------------------------------------------------------
def test_a_checkpoint_belongs_to_its_projection():
    """The projection is part of what a film was rendered from: a checkpoint written under one is refused under another (the camera
    included), accepted under the same one, and the camera's manifest is what it was without any of this."""
    import tempfile
    H = pydrt.host_lib()
    f64p = C.POINTER(C.c_double)
    H.parse_config.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]
    H.parse_config.restype = None
    H.drt_host_write_outputs.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, f64p, f64p, f64p, C.c_int, C.c_uint32, C.c_uint64]
    H.drt_host_load_checkpoint.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, f64p, f64p, f64p, C.POINTER(C.c_uint32)]
    H.drt_host_checkpoint_error.restype = C.c_char_p
    H.drt_host_checkpoint_projection.argtypes = [C.c_uint32, C.c_double]
    H.drt_host_checkpoint_projection.restype = None
    CAMERA, EQUIRECT, ORTHO = 0, 1, 2
    w, h, S, n = 5, 3, 69, 4
    d = tempfile.mkdtemp(prefix="rf", dir="/tmp")  # (config_arguments' path fields hold 63 characters)
    scene = os.path.join(d, "s.scn")
    open(scene, "w").write("Camera\n")
    text = ("num_pixel_samples 6\nmax_cast_depth 4\noutput_width 5\noutput_height 3\nmin_wl 380.0\nmax_wl 720.0\nwl_interval 5.0\npixel_scheme pixel_random\n"
            "input_scene %s\noutput_spd %s/output.spd\naverage_spd %s/average.spd\nvariance_spd %s/variance.spd\n" % (scene, d, d, d)).encode()
    cfg = C.create_string_buffer(1136)
    H.parse_config(C.create_string_buffer(text, len(text) + 1), len(text), cfg)
    rng = np.random.default_rng(5)
    px = np.zeros((w * h, S + 1))
    px[:, :S] = rng.uniform(0, 5, (w * h, S)) * n
    px[:, S] = n
    av, va = np.ascontiguousarray(px[:, :S] / n), rng.uniform(0, 2, (w * h, S))

    def write(projection, width=0.0):
        H.drt_host_checkpoint_projection(projection, width)
        assert H.drt_host_write_outputs(cfg, w, h, S, 380.0, 5.0, px.ctypes.data_as(f64p), av.ctypes.data_as(f64p), va.ctypes.data_as(f64p), 1, n, 1) == 0
        return open(os.path.join(d, "output.spd.ckpt")).read()

    def load(projection, width=0.0):
        H.drt_host_checkpoint_projection(projection, width)
        a, b, c, done = np.zeros_like(px), np.zeros_like(av), np.zeros_like(va), C.c_uint32(0)
        rc = H.drt_host_load_checkpoint(cfg, w, h, S, 1, a.ctypes.data_as(f64p), b.ctypes.data_as(f64p), c.ctypes.data_as(f64p), C.byref(done))
        return rc == 0 and done.value == n and np.array_equal(a, px), H.drt_host_checkpoint_error().decode()

    try:
        jobs = [(CAMERA, 0.0), (EQUIRECT, 0.0), (ORTHO, 6.5), (ORTHO, 3.0)]
        manifests = []
        for job in jobs:
            manifests.append(write(*job))
            for other in jobs:
                ok, why = load(*other)
                assert ok == (other == job), (job, other, why)
                if not ok:
                    assert "DRT_PROJECTION" in why
        assert len(set(manifests)) == len(jobs)
        # a width given with another projection than ortho is not part of the job
        write(EQUIRECT, 0.0)
        assert load(EQUIRECT, 9.0)[0]
        # the camera's fingerprint is the scene file's own FNV-1a, as before
        hsh = 0xcbf29ce484222325
        for c in open(scene, "rb").read():
            hsh = ((hsh ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        assert ("scene %x\n" % hsh) in manifests[0]
    finally:
        H.drt_host_checkpoint_projection(CAMERA, 0.0)


def test_the_oracles_ray_table_is_the_cameras_film_and_the_scaled_rows_are_not():
    """The oracle's own ray film (drt_oracle_set_ray_table): from the camera's table it is the camera's film, bit for bit, hit log and
    counts included; through two layers it is sample s through camera s % 2, as tests/test_gpu_ray_film.py builds it sample by sample;
    and the table of R.scaled_rows() gives another hit log -- on even rows (d times 2) and on odd rows (d times 0.5) -- so the GPU
    test that binds it checks more than the camera cases do."""
    name = R.SCALED_ROWS
    bundle, p = R.load(name)
    o, d, w = R.camera_table(name)
    cam = O.oracle_render_tile(bundle, p, want_hits=True, math_mode=O.MATH_DEVICE)
    with O.ray_table(o, d, w):
        tab = O.oracle_render_tile(bundle, p, want_hits=True, math_mode=O.MATH_DEVICE)
    for a, b in zip(cam[:3], tab[:3]):
        assert cases.same_bits(a, b), cases.first_difference(a, b)
    assert np.array_equal(cam[3], tab[3]) and cases.stat_counts(cam[4]) == cases.stat_counts(tab[4])
    after = O.oracle_render_tile(bundle, p, want_hits=True, math_mode=O.MATH_DEVICE)  # the table is gone after the block
    assert cases.same_bits(after[0], cam[0])
    ly = R.layers()
    want = R.render_by_samples(lambda b, q, film: O.oracle_render_tile(b, q, math_mode=O.MATH_DEVICE, film=film), ly["cameras"], ly["params"])
    with O.ray_table(*ly["table"]):
        got = O.oracle_render_tile(ly["bundle"], ly["params"], math_mode=O.MATH_DEVICE)
    for a, b in zip(got[:3], want):
        assert cases.same_bits(a, b), cases.first_difference(a, b)
    so, sd, sw = R.scaled_rows()
    W, H = int(p.width), int(p.height)
    assert np.array_equal(sd[0::2], d[0::2] * 2.0) and np.array_equal(sd[1::2], d[1::2] * 0.5) and so is o and sw is w
    with O.ray_table(so, sd, sw):
        sc = O.oracle_render_tile(bundle, p, want_hits=True, math_mode=O.MATH_DEVICE)
    first = lambda log: log[:, 0].reshape(int(p.spp), H, W)[0]
    differ = first(sc[3]) != first(cam[3])
    print("%s: first hits that differ from the camera's: %d on even rows, %d on odd rows" % (name, differ[0::2].sum(), differ[1::2].sum()))
    assert differ[0::2].any() and differ[1::2].any()
    assert not cases.same_bits(sc[0], cam[0])
