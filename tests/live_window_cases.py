"""Cases of the live-window tests (tests/test_live_window_cpu.py, tests/test_gpu_live_window.py): the shipped scenes under five cameras
each, made from the scene's own camera by rigid moves, and the scenes for which the rule must answer "the whole tile" or "empty"."""
import ctypes as C
import math

import numpy as np

import cases
import pydrt

SCENES = ("cornell_plane_light.scn", "cornell_gold_mirror.scn", "cornell_large_box.scn", "init_cornell.scn", "cornell_downward.scn",
          "first_scene.scn")
SIZES = ((96, 96), (64, 48))
CAMERAS = ("shipped", "rolled30", "off_axis", "twice_distance", "inside")


def _v(a):
    return np.array([a[0], a[1], a[2]], dtype=np.float64)


def _unit(a):
    return a / math.sqrt(float(a @ a))


def scene_bounds(bundle):
    """(lo, hi) of what the scene's surfaces span: rectangles' corners, spheres' centre +- radius"""
    pts = []
    for i in range(int(bundle.scene.num_surfaces)):
        s = bundle.scene.surfaces[i]
        p = _v(s.position)
        if s.type == pydrt.GEO_SPHERE:
            pts += [p - abs(s.radius), p + abs(s.radius)]
        elif s.type == pydrt.GEO_PLANE:
            u, v = _v(s.u), _v(s.v)
            pts += [p, p + u, p + v, p + u + v]
    pts = np.array(pts)
    return pts.min(axis=0), pts.max(axis=0)


def camera_frame(cam, w, h):
    """(position = the film's centre, forward, right, up, aperture distance) of a Camera"""
    f, r, u = _v(cam.forward), _v(cam.right), _v(cam.up)
    pos = _v(cam.film_bottom_left) + 0.5 * w * cam.pixel_width * r + 0.5 * h * cam.pixel_height * u
    return pos, f, r, u, float((_v(cam.aperture_position) - pos) @ f)


def make_camera(base, w, h, pos, f, r, u):
    """`base` moved rigidly: the same film, pinhole distance and lens, at `pos` with the orthonormal frame (f, r, u)"""
    _, _, _, _, ad = camera_frame(base, w, h)
    cam = pydrt.Camera.from_buffer_copy(base)
    bl = pos - 0.5 * w * base.pixel_width * r - 0.5 * h * base.pixel_height * u
    ap = pos + ad * f
    for k in range(3):
        cam.forward[k], cam.right[k], cam.up[k] = f[k], r[k], u[k]
        cam.film_bottom_left[k], cam.aperture_position[k] = bl[k], ap[k]
    return cam


def look(f, u_hint):
    """an orthonormal frame for forward f, as init_camera makes it: right = f x up"""
    f = _unit(f)
    r = _unit(np.cross(f, u_hint))
    return f, r, np.cross(r, f)


def camera_variant(bundle, w, h, which):
    cam = bundle.camera
    pos, f, r, u, ad = camera_frame(cam, w, h)
    lo, hi = scene_bounds(bundle)
    centre = 0.5 * (lo + hi)
    if which == "shipped":
        return pydrt.Camera.from_buffer_copy(cam)
    if which == "rolled30":
        a = math.radians(30.0)
        return make_camera(cam, w, h, pos, f, math.cos(a) * r + math.sin(a) * u, math.cos(a) * u - math.sin(a) * r)
    if which == "off_axis":
        return make_camera(cam, w, h, pos, *look(f + 0.25 * r + 0.15 * u, u))
    if which == "twice_distance":
        return make_camera(cam, w, h, pos - f * float((centre - pos) @ f), f, r, u)
    if which == "inside":
        return make_camera(cam, w, h, centre - ad * f, f, r, u)  # the pinhole at the middle of the scene
    if which == "sideways":  # from where it stands, looking along its own right: some of the scene is behind the pinhole
        return make_camera(cam, w, h, pos, *look(r, u))
    if which == "off_screen":  # far away, the scene in front of the pinhole but outside the 90 degree field of view
        far = centre - f * 10.0 * float(np.max(hi - lo))
        return make_camera(cam, w, h, far, *look(f + 1.6 * r, u))
    raise KeyError(which)


def with_camera(bundle, cam):
    return pydrt.SceneBundle(bundle.scene, cam, keep=bundle)


_loaded = {}


def load(scene, w, h, which="shipped"):
    """the scene at w x h under camera `which`, as a SceneBundle"""
    key = (scene, w, h)
    if key not in _loaded:
        _loaded[key] = pydrt.load_scene(cases.scene_path(scene), w, h)
    return with_camera(_loaded[key], camera_variant(_loaded[key], w, h, which))


def with_materials(bundle, edit):
    """a copy of the bundle whose materials array `edit(materials, scene)` has changed"""
    mats = bundle.materials()
    sc = pydrt.Scene.from_buffer_copy(bundle.scene)
    edit(mats, sc)
    sc.materials = C.cast(mats, C.POINTER(pydrt.Material))
    return pydrt.SceneBundle(sc, bundle.camera, keep=(bundle, mats))


def corner_ray_tables(cam, w, h):
    """(origins, dirs), each [5][h][w][3]: every pixel's four film-corner rays and its centre ray through the pinhole, as camera_ray
    makes them from the draws (0, 0), (1, 0), (0, 1), (1, 1), (0.5, 0.5)"""
    r, u, bl, ap = _v(cam.right), _v(cam.up), _v(cam.film_bottom_left), _v(cam.aperture_position)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    o, d = np.empty((5, h, w, 3)), np.empty((5, h, w, 3))
    for l, (px, py) in enumerate(((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.5, 0.5))):
        fx, fy = (xs + px) * cam.pixel_width, (ys + py) * cam.pixel_height
        o[l] = fx[..., None] * r + fy[..., None] * u + bl
        t = ap - o[l]
        d[l] = t / np.sqrt((t * t).sum(axis=-1))[..., None]
    return o, d


def outside_mask(win, params):
    """[tile_h][tile_w] bool: the tile pixels outside the window (x_lo, x_hi, y_lo, y_hi)"""
    x = int(params.x0) + np.arange(int(params.tile_w))
    y = int(params.y0) + np.arange(int(params.tile_h)) * max(1, int(params.row_stride))
    inside = ((y >= win[2]) & (y < win[3]))[:, None] & ((x >= win[0]) & (x < win[1]))[None, :]
    return ~inside


def whole_tile(params):
    s = max(1, int(params.row_stride))
    return (int(params.x0), int(params.x0 + params.tile_w), int(params.y0), int(params.y0 + (params.tile_h - 1) * s + 1))
