"""The inputs of the ray-film tests (drt_bind_rays) and what they must give. Not a test file:
tests/test_ray_film_cpu.py checks with the oracle alone that the ground truth below is sound, tests/test_gpu_ray_film.py runs it on
the device.

The ground truth needs no new oracle. A pinhole camera (aperture_radius = 0) under FILM_SAMPLE_CENTER takes no RNG draw before
cast_ray and gives every sample of a pixel the same ray, so a ray table filled with that camera's rays -- restated on the CPU by
feature_rule.camera_rays -- and weighted with that camera's vignette must reproduce the camera's film bit for bit. Tables stitched
from several cameras, by rows or by layers, are general rays with the same ground truth: each part is some camera's film.

One case has no camera behind it: scaled_rows(), the table with directions that are not of unit length. Its ground truth is the
oracle rendering from the table itself (drt_oracle_set_ray_table), which tests/test_ray_film_cpu.py first holds to the camera's film
on the unscaled table.

Every camera here is forced to aperture_radius = 0 and every params block to FILM_SAMPLE_CENTER. A weight is
rd[0]*f[0] + rd[1]*f[1] + rd[2]*f[2] in that order (v_dot's); the path header stores that value * 1.0."""
import numpy as np

import cases
import feature_rule as F
import pydrt

# the camera-parity cases (tests/cases.py): LDS scans with and without the tail wavelengths in the trace kernel, one light and many,
# another wavelength grid, an open scene most of whose rays escape, and the hierarchy
CAMERA_PARITY = ["plane_light_center", "lights", "gold_mirror", "first_scene", "many_lights", "grid_2p5nm", "spheres_1500"]
PARITY_SPP, PARITY_BATCH = 5, 2  # launches of 2 + 2 + 1 samples

STITCH_W, STITCH_H, STITCH_ROWS, STITCH_SPP = 16, 24, 8, 3
# three cameras per scene (position, target, roll, fov), at different positions and headings; camera k supplies rows 8k .. 8k + 7
STITCH_CAMERAS = {
    "lights": [((0.0, 2.0, 6.0), (0.0, -1.0, 0.0), 10.0, 70.0), ((1.5, -1.0, 4.0), (-1.0, 0.5, -1.0), 0.0, 80.0),
               ((-2.0, 1.5, 5.0), (1.0, -1.0, 0.0), -25.0, 60.0)],
    # (the sphere scene is mostly empty space under one light: each camera looks up at the light so that it falls into its own rows)
    "spheres_1500": [((8.0, 0.0, -10.0), (0.0, 25.0, -12.0), 0.0, 60.0), ((0.0, 10.0, 0.0), (0.0, 25.0, -6.0), 90.0, 50.0),
                     ((-8.0, 2.0, -12.0), (0.0, 25.0, 12.0), 0.0, 60.0)],
}
STITCH_SCENES = sorted(STITCH_CAMERAS)

_loaded, _tables = {}, {}


def params_like(p, **over):
    """a copy of a params block with some fields replaced"""
    kw = dict(width=int(p.width), height=int(p.height), spp=int(p.spp), max_depth=int(p.max_depth), seed=int(p.seed), x0=int(p.x0), y0=int(p.y0),
              tile_w=int(p.tile_w), tile_h=int(p.tile_h), row_stride=int(p.row_stride), first_sample=int(p.first_sample),
              pixel_scheme=int(p.pixel_scheme), mode=int(p.mode), device=int(p.device), batch_spp=int(p.batch_spp), flags=int(p.flags))
    kw.update(over)
    return pydrt.make_params(**kw)


def load(name):
    """(bundle, params) of a camera-parity case, loaded once: a pinhole, the centre scheme, 5 spp in launches of 2, the hit log on"""
    if name not in _loaded:
        bundle, p = cases.load_case(name)
        bundle.camera.aperture_radius = 0.0
        _loaded[name] = (bundle, params_like(p, spp=PARITY_SPP, batch_spp=PARITY_BATCH, pixel_scheme=pydrt.FILM_SAMPLE_CENTER,
                                             flags=pydrt.FLAG_RECORD_HITS))
    return _loaded[name]


def with_camera(bundle, camera):
    """the bundle's scene seen through another camera (the scene's arrays stay the first bundle's)"""
    return pydrt.SceneBundle(bundle.scene, camera, keep=bundle)


def centre_rays(bundle, width, height, sample=0, params=None):
    """(origins [h][w][3], dirs [h][w][3], weights [h][w]) of the bundle's camera for every pixel of the image under the centre scheme.
    With `params` the draws are taken as camera_ray takes them for `sample` (none for a pinhole: the CPU test's premise)."""
    x = np.tile(np.arange(width), height)
    y = np.repeat(np.arange(height), width)
    if params is None:
        px, py, disc = np.full(x.shape, 0.5), np.full(x.shape, 0.5), np.zeros((x.size, 3))
    else:
        px, py, disc = F.sample_draws(bundle, params, x, y, np.full(x.shape, sample))
    ro, rd = F.camera_rays(bundle, x, y, px, py, disc)
    f = [np.float64(v) for v in bundle.camera.forward]
    with np.errstate(all="ignore"):
        w = rd[:, 0] * f[0] + rd[:, 1] * f[1] + rd[:, 2] * f[2]
    return (np.ascontiguousarray(ro.reshape(height, width, 3)), np.ascontiguousarray(rd.reshape(height, width, 3)),
            np.ascontiguousarray(w.reshape(height, width)))


def camera_table(name):
    """the one-layer table of a camera-parity case's own camera, made once and handed out unchanged"""
    if name not in _tables:
        bundle, p = load(name)
        t = centre_rays(bundle, int(p.width), int(p.height))
        for a in t:
            a.setflags(write=False)
        _tables[name] = t
    return _tables[name]


SCALED_ROWS = "lights"  # scanned out of LDS: the reference's own loop, which takes a direction of any length


def scaled_rows(name=SCALED_ROWS):
    """the camera-parity case's own table with the directions of the even rows multiplied by 2 and those of the odd rows by 0.5.
    Such rays are no camera's: the ground truth is the oracle rendering from the same table (oracle_py.ray_table). Under the rule a
    sphere's answer depends on |d| (line_sphere_intersection sets a = 1), so this is another film than the camera's."""
    key = "scaled:" + name
    if key not in _tables:
        o, d, w = camera_table(name)
        f = np.where(np.arange(d.shape[0]) % 2 == 0, 2.0, 0.5)[:, None, None]
        t = (o, np.ascontiguousarray(d * f), w)
        t[1].setflags(write=False)
        _tables[key] = t
    return _tables[key]


def stitch(scene):
    """{"bundle", "params", "cameras": [bundle seen through camera k], "tile_params": [params of rows 8k .. 8k + 7], "table": (o, d, w)}:
    the 16 x 24 image whose rows 8k .. 8k + 7 are camera k's, made once"""
    key = "stitch:" + scene
    if key not in _tables:
        base, p = cases.load_case(scene)
        full = params_like(p, width=STITCH_W, height=STITCH_H, tile_w=STITCH_W, tile_h=STITCH_H, spp=STITCH_SPP, batch_spp=0, flags=0,
                           pixel_scheme=pydrt.FILM_SAMPLE_CENTER)
        cams = [with_camera(base, pydrt.init_camera(pos, tgt, roll, fov, 6.0, 0.3, 0.0, STITCH_W, STITCH_H)) for pos, tgt, roll, fov in STITCH_CAMERAS[scene]]
        o, d, w = (np.zeros((STITCH_H, STITCH_W, 3)), np.zeros((STITCH_H, STITCH_W, 3)), np.zeros((STITCH_H, STITCH_W)))
        tiles = []
        for k, b in enumerate(cams):
            rows = slice(STITCH_ROWS * k, STITCH_ROWS * (k + 1))
            ck = centre_rays(b, STITCH_W, STITCH_H)
            o[rows], d[rows], w[rows] = ck[0][rows], ck[1][rows], ck[2][rows]
            tiles.append(params_like(full, y0=STITCH_ROWS * k, tile_h=STITCH_ROWS))
        for a in (o, d, w):
            a.setflags(write=False)
        _tables[key] = {"bundle": cams[0], "params": full, "cameras": cams, "tile_params": tiles, "table": (o, d, w)}
    return _tables[key]


def layers(scene="lights"):
    """two of the stitched scene's cameras as layers 0 and 1 of a whole-image table: {"bundle", "params" (5 spp), "cameras",
    "table": (o [2][h][w][3], d, w [2][h][w])}"""
    key = "layers:" + scene
    if key not in _tables:
        st = stitch(scene)
        cams = st["cameras"][:2]
        parts = [centre_rays(b, STITCH_W, STITCH_H) for b in cams]
        table = tuple(np.ascontiguousarray(np.stack([parts[0][i], parts[1][i]])) for i in range(3))
        for a in table:
            a.setflags(write=False)
        _tables[key] = {"bundle": cams[0], "params": params_like(st["params"], spp=PARITY_SPP, batch_spp=PARITY_BATCH), "cameras": cams, "table": table}
    return _tables[key]


def render_by_samples(render, cameras, params, n_layers=2):
    """the film of samples [0, spp) rendered one call at a time, sample s through cameras[s % n_layers], each call accumulating into
    the film the last one left. render(bundle, params, film) -> (pixels, avgs, vars, ...)"""
    film = None
    for s in range(int(params.spp)):
        out = render(cameras[s % n_layers], params_like(params, first_sample=s, spp=1), film)
        film = out[:3]
    return film
