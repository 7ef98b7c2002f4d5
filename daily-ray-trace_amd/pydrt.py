"""ctypes bindings of the product: libdrt_hip.so (HIP launcher, include/drt_hip.h) and
libdrt_host.so (POSIX C host: .scn / CSV / camera, host/drt_host.h).

Used by tests/, bench.py and __graft_entry__.py. Python is plumbing only: every compute call
goes through the C-ABI. Nothing here touches oracle/; there is no CPU fallback -- if the HIP
library is missing, `hip_lib()` raises.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

DRT_MAX_BDSFS = 16
GEO_POINT, GEO_SPHERE, GEO_PLANE = 1, 2, 3
FILM_SAMPLE_CENTER, FILM_SAMPLE_RANDOM = 1, 2
MODE_SPECTRAL, MODE_XYZ = 0, 1
FLAG_RECORD_HITS = 1
BATCH_RESIDENT = 0xFFFFFFFF  # make_params(batch_spp=...): launches sized for a context kept across frames
FLAG_FILM_ZERO = 2
PATH_BVH, PATH_TRACE_TAIL, PATH_RAYS, PATH_RAY_STASH = 1, 2, 4, 8  # Stats.path_flags

# names and order of include/bdsf_list.h
BDSF_NAMES = ["bp_diffuse_bdsf", "bp_glossy_bdsf", "mirror_bdsf", "fs_conductor_bdsf",
              "fs_dielectric_reflectance_bdsf", "fs_dielectric_transmittance_bdsf", "ct_conductor_bdsf"]
DIRF_NAMES = ["cos_weighted_sample_hemisphere", "uniform_sample_hemisphere", "sample_specular_direction",
              "sample_transmit_direction", "sample_reflect_or_transmit_direction", "sample_ct_direction"]
BDSF = {n: i for i, n in enumerate(BDSF_NAMES)}
DIRF = {n: i for i, n in enumerate(DIRF_NAMES)}

f64x3 = C.c_double * 3


class Surface(C.Structure):
    _fields_ = [("type", C.c_uint32), ("material", C.c_uint32), ("position", f64x3), ("radius", C.c_double),
                ("normal", f64x3), ("u", f64x3), ("v", f64x3)]


class Material(C.Structure):
    _fields_ = [("is_black_body", C.c_uint32), ("is_emissive", C.c_uint32), ("shininess", C.c_double),
                ("roughness", C.c_double), ("emission_spd", C.c_int32), ("diffuse_spd", C.c_int32),
                ("glossy_spd", C.c_int32), ("mirror_spd", C.c_int32), ("refract_spd", C.c_int32),
                ("extinct_spd", C.c_int32), ("num_bdsfs", C.c_uint32), ("bdsfs", C.c_uint32 * DRT_MAX_BDSFS),
                ("dir_func", C.c_uint32)]


class Scene(C.Structure):
    _fields_ = [("num_surfaces", C.c_uint32), ("surfaces", C.POINTER(Surface)), ("num_materials", C.c_uint32),
                ("materials", C.POINTER(Material)), ("base_material", C.c_uint32), ("escape_material", C.c_uint32),
                ("num_spds", C.c_uint32), ("num_wavelengths", C.c_uint32), ("spds", C.POINTER(C.c_double)),
                ("min_wavelength", C.c_double), ("wavelength_interval", C.c_double), ("cmf_rw", C.c_uint32),
                ("cmf_x", C.c_uint32), ("cmf_y", C.c_uint32), ("cmf_z", C.c_uint32)]


class Camera(C.Structure):
    _fields_ = [("forward", f64x3), ("right", f64x3), ("up", f64x3), ("aperture_position", f64x3),
                ("aperture_radius", C.c_double), ("focal_depth", C.c_double), ("focal_length", C.c_double),
                ("film_bottom_left", f64x3), ("pixel_width", C.c_double), ("pixel_height", C.c_double)]


class Params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32),
                ("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("row_stride", C.c_uint32), ("spp", C.c_uint32),
                ("first_sample", C.c_uint32), ("max_depth", C.c_uint32), ("pixel_scheme", C.c_uint32),
                ("seed", C.c_uint64), ("mode", C.c_uint32), ("device", C.c_int32), ("batch_spp", C.c_uint32),
                ("flags", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("closest_hit_scans", C.c_uint64), ("shaded_vertices", C.c_uint64),
                ("shadow_scans", C.c_uint64), ("rng_draws", C.c_uint64), ("trace_ms", C.c_double),
                ("shade_ms", C.c_double), ("total_ms", C.c_double), ("record_pool_blocks", C.c_uint64),
                ("record_pool_peak", C.c_uint64), ("record_block_bytes", C.c_uint32), ("redone_launches", C.c_uint32),
                ("launches", C.c_uint32), ("path_flags", C.c_uint32), ("min_sample_ms", C.c_double), ("max_sample_ms", C.c_double),
                ("avg_sample_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Adaptive(C.Structure):
    """drt_adaptive (include/drt_hip.h): the inputs of an adaptive render and, after it, rounds / pixels_at_max / paths."""
    _fields_ = [("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("step", C.c_uint32), ("flags", C.c_uint32),
                ("rel_error", C.c_double), ("floor", C.c_double), ("rounds", C.c_uint32), ("pixels_at_max", C.c_uint32),
                ("paths", C.c_uint64)]


def make_adaptive(min_spp, max_spp, step, rel_error, floor=0.0):
    a = Adaptive()
    a.min_spp, a.max_spp, a.step, a.flags = min_spp, max_spp, step, 0
    a.rel_error, a.floor = rel_error, floor
    return a


MAP_DEVICE, MAP_ADD = 1, 2  # DRT_MAP_DEVICE, DRT_MAP_ADD


class SampleMap(C.Structure):
    """drt_sample_map (include/drt_hip.h): the targets and flags of a sample-map render and, after it, its report."""
    _fields_ = [("targets", C.c_void_p), ("flags", C.c_uint32), ("rounds", C.c_uint32), ("pixels_rendered", C.c_uint32),
                ("pixels_above", C.c_uint32), ("max_count", C.c_uint32), ("paths", C.c_uint64)]


def _map_report(m):
    return {"rounds": m.rounds, "paths": m.paths, "pixels_rendered": m.pixels_rendered, "pixels_above": m.pixels_above,
            "max_count": m.max_count}


def _map_u32(targets, tile_w, tile_h, name):
    """a host map as a contiguous uint32 array [tile_h * tile_w]: any integer dtype, every value in [0, 2^32), (tile_h, tile_w) or flat"""
    a = np.asarray(targets)
    if a.dtype.kind not in "iu":
        raise ValueError("%s: the targets are integers, not %s" % (name, a.dtype))
    if a.shape != (tile_h, tile_w) and a.shape != (tile_h * tile_w,):
        raise ValueError("%s: targets of shape (%d, %d) or (%d,), not %s" % (name, tile_h, tile_w, tile_h * tile_w, a.shape))
    if a.size and a.dtype != np.uint32:
        lo, hi = int(a.min()), int(a.max())
        if lo < 0:
            raise ValueError("%s: a target is negative (%d)" % (name, lo))
        if hi > 0xFFFFFFFF:
            raise ValueError("%s: a target is above 2^32 - 1 (%d)" % (name, hi))
    return np.ascontiguousarray(a.reshape(-1), dtype=np.uint32)


def region_map(tile_w, tile_h, base, regions):
    """A sample map [tile_h][tile_w] (uint32): `base` everywhere, and inside every region (x, y, w, h, spp) -- clipped to the tile -- the
    largest spp of the regions that cover the pixel, where that is above base."""
    tile_w, tile_h, base = int(tile_w), int(tile_h), int(base)
    if tile_w < 1 or tile_h < 1 or not 0 <= base <= 0xFFFFFFFF:
        raise ValueError("region_map: a tile of at least one pixel and a base in [0, 2^32)")
    m = np.full((tile_h, tile_w), base, dtype=np.uint32)
    for x, y, w, h, spp in regions:
        x, y, w, h, spp = int(x), int(y), int(w), int(h), int(spp)
        if w < 0 or h < 0 or not 0 <= spp <= 0xFFFFFFFF:
            raise ValueError("region_map: a region's size is not negative and its spp is in [0, 2^32)")
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, tile_w), min(y + h, tile_h)
        if x1 > x0 and y1 > y0:
            m[y0:y1, x0:x1] = np.maximum(m[y0:y1, x0:x1], np.uint32(spp))
    return m


def coverage_map(coverage, base, extra):
    """A sample map of the shape of `coverage` (a read_matte buffer, values in [0, 1]): base + ceil(extra * coverage), uint32."""
    c = np.asarray(coverage, dtype=np.float64)
    base, extra = int(base), int(extra)
    if base < 0 or extra < 0 or not np.all((c >= 0.0) & (c <= 1.0)):
        raise ValueError("coverage_map: base and extra are not negative and the coverage lies in [0, 1]")
    m = np.ceil(np.float64(extra) * c) + np.float64(base)
    if m.size and m.max() > 0xFFFFFFFF:
        raise ValueError("coverage_map: a target is above 2^32 - 1")
    return m.astype(np.uint32)


class Denoise(C.Structure):
    """drt_denoise (include/drt_hip.h): the inputs of the variance-guided denoiser and, after it, unusable / kernel_ms."""
    _fields_ = [("radius", C.c_uint32), ("patch", C.c_uint32), ("flags", C.c_uint32), ("unusable", C.c_uint32),
                ("k", C.c_double), ("alpha", C.c_double), ("kernel_ms", C.c_double)]


def make_denoise(radius=5, patch=1, k=1.0, alpha=1.0):
    d = Denoise()
    d.radius, d.patch, d.flags, d.unusable = radius, patch, 0, 0
    d.k, d.alpha, d.kernel_ms = k, alpha, 0.0
    return d


FEATURE_CHANNELS = 8  # DRT_FEATURE_CHANNELS: normal x y z, depth, coverage, albedo X Y Z
FEATURE_NORMAL, FEATURE_DEPTH, FEATURE_COVERAGE = 0, 1, 2  # read_feature_bgra(which)


class Features(C.Structure):
    """drt_features (include/drt_hip.h): the inputs of a first-hit feature pass and, after it, empty_pixels / rays / kernel_ms."""
    _fields_ = [("n_samples", C.c_uint32), ("first_sample", C.c_uint32), ("flags", C.c_uint32), ("empty_pixels", C.c_uint32),
                ("rays", C.c_uint64), ("kernel_ms", C.c_double)]


def make_features(n_samples=0, first_sample=0):
    f = Features()
    f.n_samples, f.first_sample, f.flags, f.empty_pixels = n_samples, first_sample, 0, 0
    f.rays, f.kernel_ms = 0, 0.0
    return f


MATTE_SLOTS, MATTE_LAYERS, MATTE_ID_MISS = 6, 2, -1  # DRT_MATTE_SLOTS, DRT_MATTE_LAYERS, DRT_MATTE_ID_MISS
MATTE_SURFACE, MATTE_MATERIAL = 0, 1  # the layers


class Mattes(C.Structure):
    """drt_mattes (include/drt_hip.h): the inputs of an ID-matte pass and, after it, empty_pixels / overflow_pixels / rays / kernel_ms."""
    _fields_ = [("n_samples", C.c_uint32), ("first_sample", C.c_uint32), ("flags", C.c_uint32), ("empty_pixels", C.c_uint32),
                ("overflow_pixels", C.c_uint32 * 2), ("rays", C.c_uint64), ("kernel_ms", C.c_double)]


def make_mattes(n_samples=0, first_sample=0):
    m = Mattes()
    m.n_samples, m.first_sample, m.flags, m.empty_pixels = n_samples, first_sample, 0, 0
    m.overflow_pixels[0] = m.overflow_pixels[1] = 0
    m.rays, m.kernel_ms = 0, 0.0
    return m


RAYS_DEVICE = 1  # DRT_RAYS_DEVICE


class RayHit(C.Structure):
    """drt_ray_hit (include/drt_hip.h): a closest hit as find_ray_intersection gives it, plus the distance. 104 bytes."""
    _fields_ = [("position", f64x3), ("normal", f64x3), ("out", f64x3), ("on_dot", C.c_double), ("distance", C.c_double),
                ("index", C.c_int32), ("surface_material", C.c_uint32), ("incident_material", C.c_uint32),
                ("transmit_material", C.c_uint32)]


# the same layout as a numpy record: what cast_rays / cast_pixels return in host mode
RAY_HIT_DTYPE = np.dtype([("position", "<f8", 3), ("normal", "<f8", 3), ("out", "<f8", 3), ("on_dot", "<f8"), ("distance", "<f8"),
                          ("index", "<i4"), ("surface_material", "<u4"), ("incident_material", "<u4"), ("transmit_material", "<u4")])
assert RAY_HIT_DTYPE.itemsize == C.sizeof(RayHit) == 104


class RayTable(C.Structure):
    """drt_ray_table (include/drt_hip.h): the first rays of a ray film, [n_layers][height][width] over the whole image. 32 bytes."""
    _fields_ = [("origins", C.c_void_p), ("dirs", C.c_void_p), ("weights", C.c_void_p), ("n_layers", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(RayTable) == 32


def _ray_table(origins, dirs, weights, width, height, device):
    """(RayTable, what must stay referenced) from numpy arrays [L][h][w][3] / [h][w][3] (host mode) or float64 torch tensors of those
    shapes on cuda:<device> (device mode); weights [L][h][w] / [h][w] or None."""
    t = RayTable()
    if _is_tensor(origins) or _is_tensor(dirs) or _is_tensor(weights):
        torch = sys.modules["torch"]
        arrs = [origins, dirs] + ([weights] if weights is not None else [])
        for a, name in zip(arrs, ("origins", "dirs", "weights")):
            if not _is_tensor(a) or a.dtype != torch.float64 or not a.is_contiguous():
                raise ValueError("%s: a contiguous float64 tensor (device mode takes tensors only)" % name)
            if a.device.type != "cuda" or a.device.index != device:
                raise ValueError("%s: a tensor on the context's device (cuda:%d)" % (name, device))
        shape = lambda a: tuple(a.shape)
        ptr = lambda a: a.data_ptr()
        t.flags = RAYS_DEVICE
    else:
        arrs = [np.ascontiguousarray(origins, dtype=np.float64), np.ascontiguousarray(dirs, dtype=np.float64)]
        if weights is not None:
            arrs.append(np.ascontiguousarray(weights, dtype=np.float64))
        shape = lambda a: a.shape
        ptr = lambda a: a.ctypes.data
        t.flags = 0
    o = shape(arrs[0])
    if len(o) == 3:
        o = (1,) + o
    if len(o) != 4 or o[0] < 1 or o[1:] != (height, width, 3):
        raise ValueError("origins: [n_layers][%d][%d][3] or [%d][%d][3]" % (height, width, height, width))
    d = shape(arrs[1])
    if (d if len(d) == 4 else (1,) + d) != o:
        raise ValueError("dirs: the shape of origins")
    if weights is not None:
        w = shape(arrs[2])
        if (w if len(w) == 3 else (1,) + w) != o[:3]:
            raise ValueError("weights: [n_layers][%d][%d] or [%d][%d]" % (height, width, height, width))
    t.origins, t.dirs = ptr(arrs[0]), ptr(arrs[1])
    t.weights = ptr(arrs[2]) if weights is not None else None
    t.n_layers = o[0]
    return t, arrs


SURFACES_DEVICE, SURFACES_REBUILD = 1, 2  # DRT_SURFACES_*
SPECTRA_DEVICE = 1  # DRT_SPECTRA_DEVICE
SURFACE_ROW = 14  # a drt_surface as doubles: word 0 holds type and material, then position, radius, normal, u, v


class UpdateReport(C.Structure):
    """drt_update_report (include/drt_hip.h). 24 bytes."""
    _fields_ = [("updates", C.c_uint32), ("refits_since_build", C.c_uint32), ("extent", C.c_double), ("kernel_ms", C.c_double)]


assert C.sizeof(Surface) == 8 * SURFACE_ROW == 112 and C.sizeof(UpdateReport) == 24


class HierarchyReport(C.Structure):
    """drt_hierarchy_report (include/drt_hip.h). 32 bytes."""
    _fields_ = [("nodes", C.c_uint32), ("leaf_surfaces", C.c_uint32), ("depth", C.c_uint32), ("device_builds", C.c_uint32),
                ("built_by", C.c_uint32), ("pad", C.c_uint32), ("kernel_ms", C.c_double)]


# a BvhNode (csrc/drt_kernels.h): the two children's f32 boxes, the traversal's references to them, and their kinds. 64 bytes.
BVH_NODE = np.dtype([("lo", "<f4", (2, 3)), ("hi", "<f4", (2, 3)), ("child", "<i4", (2,)), ("count", "<i4", (2,))])
assert C.sizeof(HierarchyReport) == 32 and BVH_NODE.itemsize == 64


def surface_rows(bundle_or_surfaces):
    """[n][14] float64: the bytes of the scene's drt_surface records viewed as doubles (word 0 holds type and material, so it is
    no number to compute with). Takes a SceneBundle or a ctypes Surface array; a copy."""
    if hasattr(bundle_or_surfaces, "scene"):
        sc = bundle_or_surfaces.scene
        n, src = int(sc.num_surfaces), sc.surfaces
    else:
        n, src = len(bundle_or_surfaces), bundle_or_surfaces
    rows = np.empty((n, SURFACE_ROW), dtype=np.float64)
    if n:
        C.memmove(rows.ctypes.data, src, n * C.sizeof(Surface))
    return rows


def surfaces_from_rows(rows):
    """the inverse of surface_rows: a ctypes Surface array with the rows' bytes"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != SURFACE_ROW:
        raise ValueError("rows: an [n][%d] float64 array" % SURFACE_ROW)
    sa = (Surface * max(1, rows.shape[0]))()
    if rows.shape[0]:
        C.memmove(sa, rows.ctypes.data, rows.shape[0] * C.sizeof(Surface))
    return sa


def _update_args(surfaces, device):
    """(pointer, count, flags, what must stay referenced) of update_surfaces' three input forms"""
    if _is_tensor(surfaces):
        torch = sys.modules["torch"]
        t = surfaces
        if t.dtype != torch.float64 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != SURFACE_ROW:
            raise ValueError("surfaces: a contiguous [n][%d] float64 tensor" % SURFACE_ROW)
        if t.device.type != "cuda" or t.device.index != device:
            raise ValueError("surfaces: a tensor on the context's device (cuda:%d)" % device)
        return t.data_ptr(), int(t.shape[0]), SURFACES_DEVICE, t
    if isinstance(surfaces, np.ndarray):
        rows = np.ascontiguousarray(surfaces, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != SURFACE_ROW:
            raise ValueError("surfaces: an [n][%d] float64 array" % SURFACE_ROW)
        return rows.ctypes.data, int(rows.shape[0]), 0, rows
    return C.cast(surfaces, C.c_void_p).value, len(surfaces), 0, surfaces


def _spectra_args(rows, S, device):
    """(pointer, count, flags, what must stay referenced) of update_spectra's two input forms"""
    if _is_tensor(rows):
        torch = sys.modules["torch"]
        t = rows
        if t.dtype != torch.float64 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != S:
            raise ValueError("rows: a contiguous [n][%d] float64 tensor" % S)
        if t.device.type != "cuda" or t.device.index != device:
            raise ValueError("rows: a tensor on the context's device (cuda:%d)" % device)
        return t.data_ptr(), int(t.shape[0]), SPECTRA_DEVICE, t
    a = np.ascontiguousarray(rows, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != S:
        raise ValueError("rows: an [n][%d] float64 array" % S)
    return a.ctypes.data, int(a.shape[0]), 0, a


def _materials_args(materials):
    """(pointer, count, what must stay referenced): a ctypes Material array, or a sequence of Material"""
    if not isinstance(materials, C.Array):
        materials = (Material * max(1, len(materials)))(*materials) if len(materials) else (Material * 0)()
    return C.cast(materials, C.c_void_p).value, len(materials), materials


def turntable_camera(bundle, width, height, k, n):
    """drt_host_turntable_camera (host/drt_host.h): the camera of frame k of an n-frame turntable about the target of a LOADED scene's
    camera (load_scene / load_scene_text); k = 0 is the scene's camera bit for bit."""
    if bundle._handle is None:
        raise ValueError("turntable_camera: a scene loaded through the host library (it keeps the camera's position and target)")
    cam = Camera()
    if host_lib().drt_host_turntable_camera(bundle._handle, width, height, k, n, C.byref(cam)) != 0:
        raise ValueError("turntable_camera: n of at least 1 and an image of at least one pixel")
    return cam


def _camera_of(bundle_or_camera):
    return bundle_or_camera.camera if hasattr(bundle_or_camera, "camera") else bundle_or_camera


def equirect_rays(camera, width, height):
    """drt_host_rays_equirect (host/drt_host.h): (origins, dirs), each [height][width][3], of an equirectangular capture about the
    camera's aperture position. `camera`: a Camera or a SceneBundle."""
    cam = _camera_of(camera)
    o, d = np.empty((height, width, 3)), np.empty((height, width, 3))
    if host_lib().drt_host_rays_equirect(C.byref(cam), width, height, _ptr(o, C.c_double), _ptr(d, C.c_double)) != 0:
        raise ValueError("equirect_rays: an image of at least one pixel")
    return o, d


def ortho_rays(camera, width, height, film_width):
    """drt_host_rays_ortho (host/drt_host.h): (origins, dirs), each [height][width][3]: parallel rays along the camera's forward from a
    rectangle film_width wide through its aperture position."""
    cam = _camera_of(camera)
    o, d = np.empty((height, width, 3)), np.empty((height, width, 3))
    if host_lib().drt_host_rays_ortho(C.byref(cam), width, height, float(film_width), _ptr(o, C.c_double), _ptr(d, C.c_double)) != 0:
        raise ValueError("ortho_rays: an image of at least one pixel and a finite film_width above 0")
    return o, d


def _is_tensor(a):
    return "torch" in sys.modules and isinstance(a, sys.modules["torch"].Tensor)


def _rays_f64(a, name):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s: an [n][3] array" % name)
    return a


def _rays_tensor(t, name, device):
    torch = sys.modules["torch"]
    if t.dtype != torch.float64 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("%s: a contiguous [n][3] float64 tensor" % name)
    if t.device.type != "cuda" or t.device.index != device:
        raise ValueError("%s: a tensor on the context's device (cuda:%d)" % (name, device))
    return t


def _pixels_u32(xy, samples):
    xy = np.ascontiguousarray(xy, dtype=np.uint32)
    samples = np.ascontiguousarray(samples, dtype=np.uint32).reshape(-1)
    if xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] != samples.shape[0]:
        raise ValueError("xy: an [n][2] array, samples: [n]")
    return xy, samples


def _mattes_report(m):
    return {"empty_pixels": m.empty_pixels, "overflow_pixels": (m.overflow_pixels[0], m.overflow_pixels[1]), "rays": m.rays,
            "kernel_ms": m.kernel_ms}


def make_params(width, height, spp, max_depth, seed=1, x0=0, y0=0, tile_w=None, tile_h=None, row_stride=1,
                first_sample=0, pixel_scheme=FILM_SAMPLE_RANDOM, mode=MODE_SPECTRAL, device=0, batch_spp=0, flags=0):
    p = Params()
    p.width, p.height = width, height
    p.x0, p.y0 = x0, y0
    p.tile_w = width if tile_w is None else tile_w
    p.tile_h = height if tile_h is None else tile_h
    p.row_stride = row_stride
    p.spp, p.first_sample, p.max_depth, p.pixel_scheme = spp, first_sample, max_depth, pixel_scheme
    p.seed, p.mode, p.device, p.batch_spp, p.flags = seed, mode, device, batch_spp, flags
    return p


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


# ------------------------------------------------------------------------------------------------
# libdrt_host.so

_host = None


def host_lib():
    global _host
    if _host is None:
        path = os.path.join(HERE, "libdrt_host.so")
        if not os.path.exists(path):
            raise RuntimeError("libdrt_host.so is not built: run __graft_entry__.build() / make -C daily-ray-trace_amd host")
        L = C.CDLL(path)
        L.drt_host_load_scene.restype = C.c_void_p
        L.drt_host_load_scene.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_double,
                                          C.c_double, C.c_double]
        L.drt_host_load_scene_text.restype = C.c_void_p
        L.drt_host_load_scene_text.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                               C.c_double, C.c_double, C.c_double]
        L.drt_host_free_scene.argtypes = [C.c_void_p]
        L.drt_host_scene_data.restype = C.POINTER(Scene)
        L.drt_host_scene_data.argtypes = [C.c_void_p]
        L.drt_host_camera_data.restype = C.POINTER(Camera)
        L.drt_host_camera_data.argtypes = [C.c_void_p]
        L.drt_host_material_name.restype = C.c_char_p
        L.drt_host_material_name.argtypes = [C.c_void_p, C.c_uint32]
        L.drt_host_surface_name.restype = C.c_char_p
        L.drt_host_surface_name.argtypes = [C.c_void_p, C.c_uint32]
        L.drt_host_last_error.restype = C.c_char_p
        L.drt_host_csv_to_spectrum.restype = C.c_uint32
        L.drt_host_csv_to_spectrum.argtypes = [C.c_char_p, C.c_double, C.c_double, C.c_uint32, C.POINTER(C.c_double)]
        L.drt_host_rgb_to_spectrum.argtypes = [C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.drt_host_blackbody_spectrum.argtypes = [C.c_double, C.c_double, C.c_uint32, C.c_double, C.POINTER(C.c_double)]
        L.drt_host_init_camera.argtypes = [C.POINTER(Camera), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                           C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_uint32]
        f64p = C.POINTER(C.c_double)
        L.drt_host_rays_equirect.argtypes = [C.POINTER(Camera), C.c_uint32, C.c_uint32, f64p, f64p]
        L.drt_host_rays_ortho.argtypes = [C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_double, f64p, f64p]
        L.drt_host_turntable_camera.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Camera)]
        _host = L
    return _host


class SceneBundle:
    """A scene + camera pair ready for the C-ABI. Keeps every backing array alive."""

    def __init__(self, scene, camera, keep=None, handle=None):
        self.scene = scene
        self.camera = camera
        self._keep = keep
        self._handle = handle

    @property
    def S(self):
        return int(self.scene.num_wavelengths)

    def spds(self):
        n = int(self.scene.num_spds) * self.S
        return np.ctypeslib.as_array(self.scene.spds, shape=(n,)).reshape(int(self.scene.num_spds), self.S).copy()

    def materials(self):
        """a copy of the scene's Material array"""
        n = int(self.scene.num_materials)
        out = (Material * n)()
        if n:
            C.memmove(out, self.scene.materials, n * C.sizeof(Material))
        return out

    def material_names(self):
        if self._handle is None:
            return [""] * int(self.scene.num_materials)
        return [host_lib().drt_host_material_name(self._handle, i).decode() for i in range(int(self.scene.num_materials))]

    def surface_names(self):
        if self._handle is None:
            return [""] * int(self.scene.num_surfaces)
        return [host_lib().drt_host_surface_name(self._handle, i).decode() for i in range(int(self.scene.num_surfaces))]

    def __del__(self):
        try:
            if self._handle is not None and _host is not None:
                _host.drt_host_free_scene(self._handle)
                self._handle = None
        except Exception:
            pass


def load_scene(scene_path, width, height, spectra_dir=None, min_wl=380.0, max_wl=720.0, wl_interval=5.0):
    """parse .scn + build scene/camera through the C host (host/drt_scene.c)."""
    L = host_lib()
    spectra_dir = spectra_dir or os.path.join(REPO, "spectra")
    h = L.drt_host_load_scene(scene_path.encode(), spectra_dir.encode(), None, width, height, min_wl, max_wl, wl_interval)
    if not h:
        raise RuntimeError("drt_host_load_scene: " + L.drt_host_last_error().decode())
    return SceneBundle(L.drt_host_scene_data(h).contents, L.drt_host_camera_data(h).contents, handle=h)


def load_scene_text(text, width, height, spectra_dir=None, min_wl=380.0, max_wl=720.0, wl_interval=5.0):
    L = host_lib()
    spectra_dir = spectra_dir or os.path.join(REPO, "spectra")
    b = text.encode()
    h = L.drt_host_load_scene_text(b, len(b), spectra_dir.encode(), None, width, height, min_wl, max_wl, wl_interval)
    if not h:
        raise RuntimeError("drt_host_load_scene_text: " + L.drt_host_last_error().decode())
    return SceneBundle(L.drt_host_scene_data(h).contents, L.drt_host_camera_data(h).contents, handle=h)


def init_camera(position, target, roll, fov, fdepth, flength, aperture, width, height):
    cam = Camera()
    pos = (C.c_double * 3)(*position)
    tgt = (C.c_double * 3)(*target)
    host_lib().drt_host_init_camera(C.byref(cam), pos, tgt, roll, fov, fdepth, flength, aperture, width, height)
    return cam


def build_scene(surfaces, materials, spds, base_material, escape_material, camera, min_wl=380.0, wl_interval=5.0,
                cmf=(0, 1, 2, 3)):
    """Assemble a Scene from Python data (synthetic scenes).

    surfaces: list of dicts {type, material, position, radius?, normal?, u?, v?}
    materials: list of dicts with Material field names (bdsfs as list of ids)
    spds: float64 array [n_spd][S]
    """
    spds = np.ascontiguousarray(spds, dtype=np.float64)
    sa = (Surface * max(1, len(surfaces)))()
    for i, s in enumerate(surfaces):
        sa[i].type = s["type"]
        sa[i].material = s["material"]
        sa[i].position = f64x3(*s["position"])
        sa[i].radius = float(s.get("radius", 0.0))
        for k in ("normal", "u", "v"):
            if k in s:
                setattr(sa[i], k, f64x3(*s[k]))
    ma = (Material * max(1, len(materials)))()
    for i, m in enumerate(materials):
        for k in ("emission_spd", "diffuse_spd", "glossy_spd", "mirror_spd", "refract_spd", "extinct_spd"):
            setattr(ma[i], k, int(m.get(k, -1)))
        ma[i].is_black_body = int(m.get("is_black_body", 0))
        ma[i].is_emissive = int(m.get("is_emissive", 0))
        ma[i].shininess = float(m.get("shininess", 0.0))
        ma[i].roughness = float(m.get("roughness", 0.0))
        b = m.get("bdsfs", [])
        ma[i].num_bdsfs = len(b)
        for j, v in enumerate(b):
            ma[i].bdsfs[j] = v
        ma[i].dir_func = int(m.get("dir_func", 0))
    sc = Scene()
    sc.num_surfaces = len(surfaces)
    sc.surfaces = C.cast(sa, C.POINTER(Surface))
    sc.num_materials = len(materials)
    sc.materials = C.cast(ma, C.POINTER(Material))
    sc.base_material, sc.escape_material = base_material, escape_material
    sc.num_spds, sc.num_wavelengths = spds.shape
    sc.spds = _ptr(spds, C.c_double)
    sc.min_wavelength, sc.wavelength_interval = min_wl, wl_interval
    sc.cmf_rw, sc.cmf_x, sc.cmf_y, sc.cmf_z = cmf
    return SceneBundle(sc, camera, keep=(sa, ma, spds))


def plane_from_points(o, pu, pv):
    """create_plane_from_points: returns (u, v, n) for a surface dict."""
    o, pu, pv = (np.asarray(a, dtype=np.float64) for a in (o, pu, pv))
    u, v = pu - o, pv - o
    n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
    n = n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    return u, v, n


# ------------------------------------------------------------------------------------------------
# libdrt_hip.so

_hip = None


def _share_torch_hip_runtime():
    """One HIP runtime per process. A PyTorch-ROCm wheel carries its own libamdhip64.so (soname libamdhip64.so.7, like
    /opt/rocm's) and loads it by file name; if libdrt_hip.so has pulled in /opt/rocm's copy first, the process ends up with
    two runtimes and the second one finds no GPU ("No HIP GPUs are available"). So when such a wheel is installed, its copy
    is loaded first -- without importing torch -- and libdrt_hip.so binds to it by soname; `import torch` later finds the
    same file already mapped. DRT_NO_TORCH_RUNTIME=1 turns this off (then never import torch after the first render)."""
    if os.environ.get("DRT_NO_TORCH_RUNTIME") or "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def hip_lib():
    global _hip
    if _hip is None:
        path = os.environ.get("DRT_HIP_LIB") or os.path.join(HERE, "libdrt_hip.so")  # DRT_HIP_LIB: A/B builds when profiling
        if not os.path.exists(path):
            raise RuntimeError("libdrt_hip.so is not built (no fallback exists): run __graft_entry__.build()")
        _share_torch_hip_runtime()
        L = C.CDLL(path)
        L.drt_last_error.restype = C.c_char_p
        L.drt_device_count.restype = C.c_int
        L.drt_create.restype = C.c_void_p
        L.drt_create.argtypes = [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params)]
        L.drt_destroy.argtypes = [C.c_void_p]
        L.drt_bind_film.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.drt_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.drt_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.drt_synchronize.argtypes = [C.c_void_p]
        L.drt_reset_film.argtypes = [C.c_void_p]
        L.drt_film_device_ptrs.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.drt_read_film.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.drt_read_xyz.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.drt_read_bgra.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint8)]
        L.drt_group_read_bgra.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint8)]
        f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        L.drt_group_create.restype = C.c_void_p
        L.drt_group_create.argtypes = [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params), i32p, C.c_uint32]
        L.drt_group_destroy.argtypes = [C.c_void_p]
        L.drt_group_destroy.restype = None
        L.drt_group_size.argtypes = [C.c_void_p]
        L.drt_group_size.restype = C.c_uint32
        L.drt_group_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.drt_group_synchronize.argtypes = [C.c_void_p]
        L.drt_group_read_film.argtypes = [C.c_void_p, f64p, f64p, f64p]
        L.drt_group_write_film.argtypes = [C.c_void_p, f64p, f64p, f64p]
        L.drt_group_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.drt_render_tile_multi.argtypes = [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params), i32p, C.c_uint32, f64p, f64p, f64p,
                                            C.POINTER(Stats)]
        L.drt_write_film.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.drt_read_hit_indices.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_uint64]
        L.drt_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.drt_render_adaptive.argtypes = [C.c_void_p, C.POINTER(Adaptive)]
        L.drt_read_sample_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.drt_read_active_list.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
        L.drt_group_render_adaptive.argtypes = [C.c_void_p, C.POINTER(Adaptive)]
        L.drt_group_read_sample_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.drt_render_adaptive_continue.argtypes = [C.c_void_p, C.POINTER(Adaptive), C.c_uint32, C.POINTER(C.c_uint32)]
        L.drt_group_render_adaptive_continue.argtypes = [C.c_void_p, C.POINTER(Adaptive), C.c_uint32, C.POINTER(C.c_uint32)]
        if hasattr(L, "drt_render_sample_map"):  # (as drt_selftest_path_ids below)
            L.drt_render_sample_map.argtypes = [C.c_void_p, C.POINTER(SampleMap)]
            L.drt_group_render_sample_map.argtypes = [C.c_void_p, C.POINTER(SampleMap)]
        if hasattr(L, "drt_denoise_film"):  # (as drt_selftest_path_ids below)
            L.drt_denoise_film.argtypes = [C.c_void_p, C.POINTER(Denoise)]
            L.drt_read_denoised.argtypes = [C.c_void_p, f64p, f64p]
            L.drt_read_denoised_bgra.argtypes = [C.c_void_p, C.POINTER(C.c_uint8)]
            L.drt_denoise_buffers.argtypes = [C.POINTER(Scene), C.POINTER(Params), C.POINTER(Denoise), f64p, f64p, f64p, f64p, f64p]
            L.drt_group_denoise.argtypes = [C.c_void_p, C.POINTER(Denoise), f64p, f64p]
        if hasattr(L, "drt_render_features"):  # (as drt_selftest_path_ids below)
            L.drt_render_features.argtypes = [C.c_void_p, C.POINTER(Features)]
            L.drt_read_features.argtypes = [C.c_void_p, f64p, f64p, i32p]
            L.drt_read_feature_bgra.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_uint8)]
            L.drt_group_render_features.argtypes = [C.c_void_p, C.POINTER(Features), f64p, f64p, i32p]
        if hasattr(L, "drt_cast_rays"):
            vp = C.c_void_p  # host or device memory
            L.drt_cast_rays.argtypes = [C.c_void_p, vp, vp, C.c_uint64, vp, C.c_uint32]
            L.drt_test_visibility.argtypes = [C.c_void_p, vp, vp, C.c_uint64, vp, C.c_uint32]
            L.drt_cast_pixels.argtypes = [C.c_void_p, vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32]
            L.drt_group_cast_rays.argtypes = [C.c_void_p, vp, vp, C.c_uint64, vp]
            L.drt_group_test_visibility.argtypes = [C.c_void_p, vp, vp, C.c_uint64, vp]
            L.drt_group_cast_pixels.argtypes = [C.c_void_p, vp, vp, C.c_uint64, vp, vp, vp]
        if hasattr(L, "drt_render_mattes"):
            u32p = C.POINTER(C.c_uint32)
            L.drt_render_mattes.argtypes = [C.c_void_p, C.POINTER(Mattes)]
            L.drt_read_mattes.argtypes = [C.c_void_p, i32p, u32p, u32p]
            L.drt_read_matte.argtypes = [C.c_void_p, C.c_int, i32p, C.c_uint32, f64p]
            L.drt_read_matte_bgra.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint8)]
            L.drt_group_render_mattes.argtypes = [C.c_void_p, C.POINTER(Mattes), i32p, u32p, u32p]
        L.drt_batch_spp.restype = C.c_uint32
        if hasattr(L, "drt_bind_rays"):
            L.drt_bind_rays.argtypes = [C.c_void_p, C.POINTER(RayTable)]
            L.drt_group_bind_rays.argtypes = [C.c_void_p, C.POINTER(RayTable)]
        L.drt_batch_spp.argtypes = [C.c_void_p]
        if hasattr(L, "drt_shade_instantiation"):  # (an older build named by DRT_HIP_LIB for an A/B run has none; build() checks HIP_SYMBOLS)
            L.drt_shade_instantiation.argtypes = [C.c_void_p]
            L.drt_shade_instantiation.restype = C.c_int
        if hasattr(L, "drt_shade_closed_lds"):
            L.drt_shade_closed_lds.argtypes = [C.c_void_p]
            L.drt_shade_closed_lds.restype = C.c_int
        if hasattr(L, "drt_shade_closed_waves"):
            L.drt_shade_closed_waves.argtypes = [C.c_void_p]
            L.drt_shade_closed_waves.restype = C.c_int
        if hasattr(L, "drt_update_surfaces"):
            L.drt_set_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
            L.drt_update_surfaces.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
            L.drt_get_update_report.argtypes = [C.c_void_p, C.POINTER(UpdateReport)]
            L.drt_group_set_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
            L.drt_group_update_surfaces.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
            L.drt_group_reset_film.argtypes = [C.c_void_p]
        if hasattr(L, "drt_update_spectra"):
            L.drt_update_spectra.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
            L.drt_update_materials.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
            L.drt_group_update_spectra.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
            L.drt_group_update_materials.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        if hasattr(L, "drt_bind_depth_cuts"):  # (as drt_selftest_path_ids below)
            u32p, vpp = C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)
            L.drt_bind_depth_cuts.argtypes = [C.c_void_p, u32p, C.c_uint32]
            L.drt_read_depth_film.argtypes = [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
            L.drt_depth_film_device_ptrs.argtypes = [C.c_void_p, C.c_uint32, vpp, vpp, vpp]
            L.drt_read_depth_xyz.argtypes = [C.c_void_p, C.c_uint32, f64p]
            L.drt_read_depth_bgra.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint8)]
            L.drt_group_bind_depth_cuts.argtypes = [C.c_void_p, u32p, C.c_uint32]
            L.drt_group_read_depth_film.argtypes = [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
        if hasattr(L, "drt_bind_sensor"):  # (as drt_selftest_path_ids below)
            vpp = C.POINTER(C.c_void_p)
            L.drt_bind_sensor.argtypes = [C.c_void_p, f64p, C.c_uint32]
            L.drt_read_sensor_film.argtypes = [C.c_void_p, f64p, f64p, f64p]
            L.drt_sensor_film_device_ptrs.argtypes = [C.c_void_p, vpp, vpp, vpp]
            L.drt_read_sensor_bgra.argtypes = [C.c_void_p, C.c_int, f64p, C.POINTER(C.c_uint8)]
            L.drt_group_bind_sensor.argtypes = [C.c_void_p, f64p, C.c_uint32]
            L.drt_group_read_sensor_film.argtypes = [C.c_void_p, f64p, f64p, f64p]
        if hasattr(L, "drt_bind_buckets"):  # (as drt_selftest_path_ids below)
            vpp, u8p = C.POINTER(C.c_void_p), C.POINTER(C.c_uint8)
            L.drt_bind_buckets.argtypes = [C.c_void_p, C.c_uint32]
            L.drt_read_bucket_film.argtypes = [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
            L.drt_bucket_film_device_ptrs.argtypes = [C.c_void_p, C.c_uint32, vpp, vpp, vpp]
            L.drt_resolve_buckets.argtypes = [C.c_void_p, C.c_uint32]
            L.drt_read_bucket_resolve.argtypes = [C.c_void_p, f64p, f64p]
            L.drt_bucket_resolve_device_ptrs.argtypes = [C.c_void_p, vpp, vpp]
            L.drt_read_bucket_resolve_xyz.argtypes = [C.c_void_p, f64p]
            L.drt_read_bucket_resolve_bgra.argtypes = [C.c_void_p, u8p]
            L.drt_group_bind_buckets.argtypes = [C.c_void_p, C.c_uint32]
            L.drt_group_read_bucket_film.argtypes = [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
            L.drt_group_resolve_buckets.argtypes = [C.c_void_p, C.c_uint32]
            L.drt_group_read_bucket_resolve.argtypes = [C.c_void_p, f64p, f64p]
        if hasattr(L, "drt_bind_lobes"):  # (as drt_selftest_path_ids below)
            vpp, u8p, mapp = C.POINTER(C.c_void_p), C.POINTER(C.c_uint8), C.POINTER(LobeMap)
            L.drt_bind_lobes.argtypes = [C.c_void_p, C.c_uint32, mapp]
            L.drt_read_lobe_film.argtypes = [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
            L.drt_lobe_film_device_ptrs.argtypes = [C.c_void_p, C.c_uint32, vpp, vpp, vpp]
            L.drt_read_lobe_xyz.argtypes = [C.c_void_p, C.c_uint32, f64p]
            L.drt_read_lobe_bgra.argtypes = [C.c_void_p, C.c_uint32, C.c_int, u8p]
            L.drt_group_bind_lobes.argtypes = [C.c_void_p, C.c_uint32, mapp]
            L.drt_group_read_lobe_film.argtypes = [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
        if hasattr(L, "drt_rebuild_hierarchy"):
            L.drt_rebuild_hierarchy.argtypes = [C.c_void_p, C.c_uint32]
            L.drt_group_rebuild_hierarchy.argtypes = [C.c_void_p, C.c_uint32]
            L.drt_get_hierarchy_report.argtypes = [C.c_void_p, C.POINTER(HierarchyReport)]
            L.drt_read_hierarchy.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]
        if hasattr(L, "drt_live_window_of"):  # (as drt_selftest_path_ids below)
            L.drt_live_window_of.argtypes = [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params), C.POINTER(C.c_uint32)]
            L.drt_live_window.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.drt_render_tile.argtypes = [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(Stats)]
        L.drt_selftest_arith.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), C.c_uint64]
        if hasattr(L, "drt_selftest_path_ids"):  # (an older build named by DRT_HIP_LIB for an A/B run has none; build() checks HIP_SYMBOLS)
            L.drt_selftest_path_ids.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.POINTER(C.c_uint64)]
        L.drt_bvh_stats.argtypes = [C.POINTER(Scene)] + [C.POINTER(C.c_uint32)] * 4
        L.drt_selftest_unit.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.c_uint32,
                                        C.c_uint64]
        L.drt_selftest_material.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.c_uint32,
                                            C.c_uint64]
        if hasattr(L, "drt_selftest_build_sort"):  # (as drt_selftest_path_ids above)
            u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
            L.drt_selftest_build_sort.argtypes = [C.c_int, u64p, C.c_uint32, u64p, u32p]
            L.drt_selftest_build_topology.argtypes = [C.c_int, u64p, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), u32p, u32p]
        if hasattr(L, "drt_selftest_live_resources"):  # (as drt_selftest_path_ids above)
            L.drt_selftest_live_resources.argtypes = [C.POINTER(C.c_uint64)]
        if hasattr(L, "drt_selftest_division"):  # (as drt_selftest_path_ids above)
            L.drt_selftest_division.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.c_uint32,
                                                C.c_uint64]
        _hip = L
    return _hip


SHADE_INSTANTIATIONS = ("general", "simple", "closed")  # DRT_SHADE_GENERAL, DRT_SHADE_SIMPLE, DRT_SHADE_CLOSED

HIP_SYMBOLS = ["drt_shade_instantiation", "drt_shade_closed_lds", "drt_shade_closed_waves",
               "drt_last_error", "drt_device_count", "drt_create", "drt_destroy", "drt_bind_film", "drt_set_stream",
               "drt_render", "drt_synchronize", "drt_reset_film", "drt_film_device_ptrs", "drt_read_film", "drt_write_film",
               "drt_read_xyz", "drt_read_bgra", "drt_read_hit_indices", "drt_get_stats", "drt_batch_spp", "drt_render_tile", "drt_selftest_arith",
               "drt_selftest_unit", "drt_selftest_material", "drt_selftest_path_ids", "drt_bvh_stats",
               "drt_selftest_build_sort", "drt_selftest_build_topology", "drt_selftest_live_resources",
               "drt_group_create", "drt_group_destroy", "drt_group_size", "drt_group_render", "drt_group_synchronize",
               "drt_group_read_film", "drt_group_write_film", "drt_group_read_bgra", "drt_group_get_stats", "drt_render_tile_multi",
               "drt_render_adaptive", "drt_read_sample_counts", "drt_group_render_adaptive", "drt_group_read_sample_counts",
               "drt_read_active_list", "drt_render_adaptive_continue", "drt_group_render_adaptive_continue",
               "drt_denoise_film", "drt_read_denoised", "drt_read_denoised_bgra", "drt_denoise_buffers", "drt_group_denoise",
               "drt_render_features", "drt_read_features", "drt_read_feature_bgra", "drt_group_render_features",
               "drt_render_mattes", "drt_read_mattes", "drt_read_matte", "drt_read_matte_bgra", "drt_group_render_mattes",
               "drt_cast_rays", "drt_test_visibility", "drt_cast_pixels", "drt_group_cast_rays", "drt_group_test_visibility",
               "drt_group_cast_pixels", "drt_bind_rays", "drt_group_bind_rays",
               "drt_set_camera", "drt_update_surfaces", "drt_get_update_report", "drt_group_set_camera", "drt_group_update_surfaces",
               "drt_group_reset_film",
               "drt_rebuild_hierarchy", "drt_group_rebuild_hierarchy", "drt_get_hierarchy_report", "drt_read_hierarchy",
               "drt_update_spectra", "drt_update_materials", "drt_group_update_spectra", "drt_group_update_materials",
               "drt_bind_depth_cuts", "drt_read_depth_film", "drt_depth_film_device_ptrs", "drt_read_depth_xyz", "drt_read_depth_bgra",
               "drt_group_bind_depth_cuts", "drt_group_read_depth_film",
               "drt_bind_sensor", "drt_read_sensor_film", "drt_sensor_film_device_ptrs", "drt_read_sensor_bgra",
               "drt_group_bind_sensor", "drt_group_read_sensor_film",
               "drt_bind_buckets", "drt_read_bucket_film", "drt_bucket_film_device_ptrs", "drt_resolve_buckets", "drt_read_bucket_resolve",
               "drt_bucket_resolve_device_ptrs", "drt_read_bucket_resolve_xyz", "drt_read_bucket_resolve_bgra",
               "drt_group_bind_buckets", "drt_group_read_bucket_film", "drt_group_resolve_buckets", "drt_group_read_bucket_resolve",
               "drt_bind_lobes", "drt_read_lobe_film", "drt_lobe_film_device_ptrs", "drt_read_lobe_xyz", "drt_read_lobe_bgra",
               "drt_group_bind_lobes", "drt_group_read_lobe_film",
               "drt_render_sample_map", "drt_group_render_sample_map",
               "drt_live_window_of", "drt_live_window", "drt_selftest_division"]

MAX_DEPTH_CUTS = 8  # DRT_MAX_DEPTH_CUTS


def _depth_array(depths):
    """the (uint32 array or None, count) of drt_bind_depth_cuts: None or an empty sequence unbinds"""
    depths = [] if depths is None else [int(d) for d in depths]
    if any(d < 0 or d > 0xFFFFFFFF for d in depths):
        raise ValueError("bind_depth_cuts: depths are unsigned 32-bit numbers")
    return ((C.c_uint32 * len(depths))(*depths) if depths else None), len(depths)


MAX_SENSOR_CHANNELS = 8  # DRT_MAX_SENSOR_CHANNELS


def _sensor_curves(curves, S):
    """the (float64 array [n][S] or None, n) of drt_bind_sensor: None or no rows unbinds. The count and the values are the library's
    to refuse (drt_last_error says which); the shape is checked here, because the library cannot see it."""
    if curves is None:
        return None, 0
    a = np.ascontiguousarray(curves, dtype=np.float64)
    if a.ndim == 1 and a.size == 0:
        return None, 0
    if a.ndim != 2 or a.shape[1] != S:
        raise ValueError("bind_sensor: curves of shape %s, need [n][%d] (one value per wavelength of the render's grid)" % (a.shape, S))
    if a.shape[0] == 0:
        return None, 0
    return a, int(a.shape[0])


def _sensor_matrix(matrix, n):
    m = np.ascontiguousarray(matrix, dtype=np.float64)
    if m.shape != (3, n):
        raise ValueError("read_sensor_bgra: a matrix of shape %s, need (3, %d): the bound channels to R, G, B" % (m.shape, n))
    return m


MAX_BUCKETS = 8  # DRT_MAX_BUCKETS


def _u32(value, what):
    """an unsigned 32-bit argument: what ctypes would wrap around silently is refused here; the range proper is the library's to refuse"""
    v = int(value)
    if v < 0 or v > 0xFFFFFFFF:
        raise ValueError("%s = %d: an unsigned 32-bit number" % (what, v))
    return v


def bucket_pair(means):
    """The half-buffer pair dual-buffer denoisers take, from bucket means [n][...] (n >= 2): the plain mean of the even buckets
    (0, 2, ...) and of the odd ones (1, 3, ...), each summed in bucket order and divided by its count. Pure numpy."""
    m = np.asarray(means, dtype=np.float64)
    if m.ndim < 1 or m.shape[0] < 2:
        raise ValueError("bucket_pair: means of shape %s, need [n][...] with n >= 2 buckets" % (m.shape,))
    out = []
    for half in (m[0::2], m[1::2]):
        acc = half[0].copy()
        for k in range(1, half.shape[0]):
            acc = acc + half[k]
        out.append(acc / float(half.shape[0]))
    return out[0], out[1]


MAX_LOBE_FILMS = 8  # DRT_MAX_LOBE_FILMS
LOBE_NONE = 0xFF    # DRT_LOBE_NONE


class LobeMap(C.Structure):
    """drt_lobe_map"""
    _fields_ = [("emission", C.c_uint8), ("direct", C.c_uint8 * len(BDSF_NAMES)), ("indirect", C.c_uint8 * len(BDSF_NAMES)), ("pad_", C.c_uint8)]


def _lobe_film(value, what):
    v = int(value)
    if v != LOBE_NONE and not 0 <= v < MAX_LOBE_FILMS:
        raise ValueError("%s = %d: a film 0 .. %d or LOBE_NONE" % (what, v, MAX_LOBE_FILMS - 1))
    return v


def _lobe_row(row, default, what):
    out = [default] * len(BDSF_NAMES)
    for name, film in dict(row or {}).items():
        key = name if name in BDSF else str(name) + "_bdsf"
        if key not in BDSF:
            raise ValueError("%s: unknown scattering function %r (one of %s)" % (what, name, ", ".join(BDSF_NAMES)))
        out[BDSF[key]] = _lobe_film(film, "%s[%s]" % (what, name))
    return out


def lobe_map(emission=None, direct=None, indirect=None, default=LOBE_NONE):
    """A drt_lobe_map: the film of emission seen by the camera ray, and {function name: film} for the light sampled at the first vertex
    (direct) and for everything behind it (indirect). Names are those of BDSF_NAMES, with or without the _bdsf ending; what is not
    named goes to `default`. The film count a map needs is lobe_map_films(map)."""
    default = _lobe_film(default, "lobe_map: default")
    m = LobeMap()
    m.emission = default if emission is None else _lobe_film(emission, "lobe_map: emission")
    for k, v in enumerate(_lobe_row(direct, default, "lobe_map: direct")):
        m.direct[k] = v
    for k, v in enumerate(_lobe_row(indirect, default, "lobe_map: indirect")):
        m.indirect[k] = v
    return m


def lobe_map_entries(m):
    """the 15 entries of a map: emission, direct[7], indirect[7]"""
    return [int(m.emission)] + [int(v) for v in m.direct] + [int(v) for v in m.indirect]


def lobe_map_films(m):
    """the smallest film count the map can be bound with: its highest film + 1 (at least 1)"""
    used = [v for v in lobe_map_entries(m) if v != LOBE_NONE]
    return max(used) + 1 if used else 1


def _lobe_presets():
    both = lambda films: dict(direct=films, indirect=films)
    functions = lobe_map(emission=0, **both({n: 1 + i for i, n in enumerate(BDSF_NAMES)}))
    d = {"bp_diffuse_bdsf": 1, "bp_glossy_bdsf": 3, "ct_conductor_bdsf": 3, "mirror_bdsf": 5, "fs_conductor_bdsf": 5,
         "fs_dielectric_reflectance_bdsf": 5, "fs_dielectric_transmittance_bdsf": 6}
    i = {"bp_diffuse_bdsf": 2, "bp_glossy_bdsf": 4, "ct_conductor_bdsf": 4, "mirror_bdsf": 5, "fs_conductor_bdsf": 5,
         "fs_dielectric_reflectance_bdsf": 5, "fs_dielectric_transmittance_bdsf": 6}
    return {"functions": (functions, ["emission"] + [n[:-len("_bdsf")] for n in BDSF_NAMES]),
            "standard": (lobe_map(emission=0, direct=d, indirect=i),
                         ["emission", "diffuse_direct", "diffuse_indirect", "glossy_direct", "glossy_indirect", "specular", "transmission"])}


# name -> (map, film names): "functions" is emission plus one film per scattering function, direct and indirect together;
# "standard" the usual layer set -- emission, diffuse and glossy each direct and indirect, specular, transmission
LOBE_PRESETS = _lobe_presets()


def _lobe_bind_args(map_or_preset, n):
    """(n, map) for a bind: a preset's name, a LobeMap (n: its highest film + 1 unless given), or None / 0 to unbind"""
    if map_or_preset is None or (isinstance(map_or_preset, int) and map_or_preset == 0):
        return 0, None
    if isinstance(map_or_preset, str):
        if map_or_preset not in LOBE_PRESETS:
            raise ValueError("bind_lobes: unknown preset %r (one of %s)" % (map_or_preset, ", ".join(sorted(LOBE_PRESETS))))
        m, names = LOBE_PRESETS[map_or_preset]
        return (len(names) if n is None else _u32(n, "bind_lobes: n")), m
    if not isinstance(map_or_preset, LobeMap):
        raise TypeError("bind_lobes: a preset's name, a pydrt.lobe_map(...) or None, not %s" % type(map_or_preset).__name__)
    return (lobe_map_films(map_or_preset) if n is None else _u32(n, "bind_lobes: n")), map_or_preset


def observer_curves(bundle):
    """The CIE observer as sensor curves [3][S]: row k is cmf_k[s] * rw[s], one multiply each -- the weights drt_read_xyz gives a
    wavelength before its normalisation."""
    spds = bundle.spds()
    sc = bundle.scene
    rw = spds[int(sc.cmf_rw)]
    return np.stack([spds[int(sc.cmf_x)] * rw, spds[int(sc.cmf_y)] * rw, spds[int(sc.cmf_z)] * rw])


def depth_layers(means):
    """Cumulative cut means [n_cuts][...] (cut k = everything up to depth d_k, ascending) as per-bounce layers: layer 0 is cut 0, layer
    k is cut k minus cut k - 1, what the loop iterations d_(k-1) .. d_k - 1 add. Pure numpy; the layers sum back to the last cut up to
    rounding."""
    m = np.asarray(means, dtype=np.float64)
    if m.ndim < 1 or m.shape[0] < 1:
        raise ValueError("depth_layers: at least one cut")
    out = m.copy()
    out[1:] = m[1:] - m[:-1]
    return out


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, hip_lib().drt_last_error().decode()))


def live_window_of(bundle, params, camera=None):
    """(x_lo, x_hi, y_lo, y_hi) in image pixels: drt_live_window_of, the rectangle outside which no camera ray reaches the scene.
    Host only (no GPU). camera: another one than the bundle's."""
    out = (C.c_uint32 * 4)()
    cam = bundle.camera if camera is None else camera
    _check(hip_lib().drt_live_window_of(C.byref(bundle.scene), C.byref(cam), C.byref(params), out), "drt_live_window_of")
    return tuple(int(v) for v in out)


class Renderer:
    """Session form of the C-ABI: scene resident on the device, film accumulated on the device."""

    def __init__(self, bundle, params):
        self.L = hip_lib()
        self.bundle = bundle
        self.params = params
        self.S = bundle.S
        self.n_pixels = int(params.tile_w) * int(params.tile_h)
        self.ctx = self.L.drt_create(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(params))
        if not self.ctx:
            raise RuntimeError("drt_create failed: " + self.L.drt_last_error().decode())

    def close(self):
        if self.ctx:
            self.L.drt_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def live_window(self):
        """(x_lo, x_hi, y_lo, y_hi) in image pixels: the context's live window as it stands (drt_live_window)"""
        out = (C.c_uint32 * 4)()
        _check(self.L.drt_live_window(self.ctx, out), "drt_live_window")
        return tuple(int(v) for v in out)

    def bind_film(self, d_pixels, d_avgs, d_vars):
        _check(self.L.drt_bind_film(self.ctx, d_pixels, d_avgs, d_vars), "drt_bind_film")

    def set_stream(self, stream_handle):
        _check(self.L.drt_set_stream(self.ctx, stream_handle), "drt_set_stream")

    def render(self, first_sample=None, num_samples=None):
        fs = int(self.params.first_sample) if first_sample is None else first_sample
        ns = int(self.params.spp) if num_samples is None else num_samples
        _check(self.L.drt_render(self.ctx, fs, ns), "drt_render")

    def synchronize(self):
        _check(self.L.drt_synchronize(self.ctx), "drt_synchronize")

    def reset_film(self):
        _check(self.L.drt_reset_film(self.ctx), "drt_reset_film")

    def film_device_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self.L.drt_film_device_ptrs(self.ctx, C.byref(a), C.byref(b), C.byref(c)), "drt_film_device_ptrs")
        return a.value, b.value, c.value

    def read_xyz_film(self):
        """XYZ film mode: the raw [n][8] accumulators (X, Y, Z, filter sum, tail X, Y, Z, 0)."""
        acc = np.empty((self.n_pixels, 8), dtype=np.float64)
        _check(self.L.drt_read_film(self.ctx, _ptr(acc, C.c_double), None, None), "drt_read_film")
        return acc

    def write_xyz_film(self, acc):
        acc = np.ascontiguousarray(acc, dtype=np.float64)
        _check(self.L.drt_write_film(self.ctx, _ptr(acc, C.c_double), None, None), "drt_write_film")

    def read_film(self):
        px = np.empty((self.n_pixels, self.S + 1), dtype=np.float64)
        av = np.empty((self.n_pixels, self.S), dtype=np.float64)
        va = np.empty((self.n_pixels, self.S), dtype=np.float64)
        _check(self.L.drt_read_film(self.ctx, _ptr(px, C.c_double), _ptr(av, C.c_double), _ptr(va, C.c_double)), "drt_read_film")
        return px, av, va

    def write_film(self, px, av, va):
        px, av, va = (np.ascontiguousarray(a, dtype=np.float64) for a in (px, av, va))
        _check(self.L.drt_write_film(self.ctx, _ptr(px, C.c_double), _ptr(av, C.c_double), _ptr(va, C.c_double)), "drt_write_film")

    def read_xyz(self):
        xyz = np.empty((self.n_pixels, 3), dtype=np.float64)
        _check(self.L.drt_read_xyz(self.ctx, _ptr(xyz, C.c_double)), "drt_read_xyz")
        return xyz

    def read_bgra(self, which=0):
        """BMP pixel bytes [n][4] = B, G, R, 255 of the sum (0), mean (1) or normalised variance (2) film."""
        out = np.empty((self.n_pixels, 4), dtype=np.uint8)
        _check(self.L.drt_read_bgra(self.ctx, int(which), _ptr(out, C.c_uint8)), "drt_read_bgra")
        return out

    def bind_depth_cuts(self, depths):
        """drt_bind_depth_cuts: one cut film per depth (ascending, each in 1..max_depth, at most MAX_DEPTH_CUTS) beside the main film,
        on a film without samples. None or an empty sequence unbinds."""
        arr, n = _depth_array(depths)
        _check(self.L.drt_bind_depth_cuts(self.ctx, arr, n), "drt_bind_depth_cuts")

    def read_depth_film(self, cut):
        """(pixels, means, variances) of cut film `cut`, laid out as read_film's"""
        px = np.empty((self.n_pixels, self.S + 1), dtype=np.float64)
        av = np.empty((self.n_pixels, self.S), dtype=np.float64)
        va = np.empty((self.n_pixels, self.S), dtype=np.float64)
        _check(self.L.drt_read_depth_film(self.ctx, int(cut), _ptr(px, C.c_double), _ptr(av, C.c_double), _ptr(va, C.c_double)), "drt_read_depth_film")
        return px, av, va

    def depth_film_device_ptrs(self, cut):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self.L.drt_depth_film_device_ptrs(self.ctx, int(cut), C.byref(a), C.byref(b), C.byref(c)), "drt_depth_film_device_ptrs")
        return a.value, b.value, c.value

    def read_depth_xyz(self, cut):
        xyz = np.empty((self.n_pixels, 3), dtype=np.float64)
        _check(self.L.drt_read_depth_xyz(self.ctx, int(cut), _ptr(xyz, C.c_double)), "drt_read_depth_xyz")
        return xyz

    def read_depth_bgra(self, cut, which=0):
        """read_bgra of cut film `cut`"""
        out = np.empty((self.n_pixels, 4), dtype=np.uint8)
        _check(self.L.drt_read_depth_bgra(self.ctx, int(cut), int(which), _ptr(out, C.c_uint8)), "drt_read_depth_bgra")
        return out

    def bind_buckets(self, n):
        """drt_bind_buckets: n films (at most MAX_BUCKETS) beside the main film, sample m in film m % n as its sample m // n, on a film
        that holds no samples; 0 or None unbinds"""
        n = _u32(0 if n is None else n, "bind_buckets: n")
        _check(self.L.drt_bind_buckets(self.ctx, n), "drt_bind_buckets")
        self.n_buckets = n

    def read_bucket_film(self, b):
        """(pixels [P][S+1], means [P][S], variances [P][S]) of bucket b's film"""
        b = _u32(b, "read_bucket_film: b")
        if not getattr(self, "n_buckets", 0) or b >= self.n_buckets:
            _check(self.L.drt_read_bucket_film(self.ctx, b, None, None, None), "drt_read_bucket_film")  # (says which, touches nothing)
        S, n = self.S, self.n_pixels
        px, av, va = np.empty((n, S + 1)), np.empty((n, S)), np.empty((n, S))
        _check(self.L.drt_read_bucket_film(self.ctx, b, _ptr(px, C.c_double), _ptr(av, C.c_double), _ptr(va, C.c_double)), "drt_read_bucket_film")
        return px, av, va

    def bucket_film_device_ptrs(self, b):
        a, bb, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self.L.drt_bucket_film_device_ptrs(self.ctx, _u32(b, "bucket_film_device_ptrs: b"), C.byref(a), C.byref(bb), C.byref(c)),
               "drt_bucket_film_device_ptrs")
        return a.value, bb.value, c.value

    def resolve_buckets(self, trim=None):
        """drt_resolve_buckets: the trimmed mean of the sorted bucket means and the squared standard error across buckets, on the device.
        trim None: the median's, (n - 1) // 2"""
        n = getattr(self, "n_buckets", 0)
        t = max(n - 1, 0) // 2 if trim is None else _u32(trim, "resolve_buckets: trim")
        _check(self.L.drt_resolve_buckets(self.ctx, t), "drt_resolve_buckets")

    def read_bucket_resolve(self):
        """(estimate [P][S], error [P][S]) of the last resolve_buckets"""
        _check(self.L.drt_read_bucket_resolve(self.ctx, None, None), "drt_read_bucket_resolve")  # (refused before anything is allocated)
        S, n = self.S, self.n_pixels
        est, err = np.empty((n, S)), np.empty((n, S))
        _check(self.L.drt_read_bucket_resolve(self.ctx, _ptr(est, C.c_double), _ptr(err, C.c_double)), "drt_read_bucket_resolve")
        return est, err

    def bucket_resolve_device_ptrs(self):
        a, b = C.c_void_p(), C.c_void_p()
        _check(self.L.drt_bucket_resolve_device_ptrs(self.ctx, C.byref(a), C.byref(b)), "drt_bucket_resolve_device_ptrs")
        return a.value, b.value

    def read_bucket_resolve_xyz(self):
        """[P][3]: drt_read_xyz's conversion of the estimate"""
        out = np.empty((self.n_pixels, 3))
        _check(self.L.drt_read_bucket_resolve_xyz(self.ctx, _ptr(out, C.c_double)), "drt_read_bucket_resolve_xyz")
        return out

    def read_bucket_resolve_bgra(self):
        """BMP pixel bytes [P][4] = B, G, R, 255 of the estimate, as read_bgra of the means"""
        out = np.empty((self.n_pixels, 4), dtype=np.uint8)
        _check(self.L.drt_read_bucket_resolve_bgra(self.ctx, _ptr(out, C.c_uint8)), "drt_read_bucket_resolve_bgra")
        return out

    def bind_lobes(self, map_or_preset, n=None):
        """drt_bind_lobes: n films beside the main film that split it by the first vertex's scattering lobe, on a film that holds no
        samples. map_or_preset: a name of LOBE_PRESETS, or a pydrt.lobe_map(...) (n: its highest film + 1 unless given); None unbinds"""
        n, m = _lobe_bind_args(map_or_preset, n)
        _check(self.L.drt_bind_lobes(self.ctx, n, C.byref(m) if m is not None else None), "drt_bind_lobes")
        self.n_lobes = n

    def read_lobe_film(self, c):
        """(pixels [P][S+1], means [P][S], variances [P][S]) of lobe film c"""
        c = _u32(c, "read_lobe_film: c")
        if not getattr(self, "n_lobes", 0) or c >= self.n_lobes:
            _check(self.L.drt_read_lobe_film(self.ctx, c, None, None, None), "drt_read_lobe_film")  # (says which, touches nothing)
        S, n = self.S, self.n_pixels
        px, av, va = np.empty((n, S + 1)), np.empty((n, S)), np.empty((n, S))
        _check(self.L.drt_read_lobe_film(self.ctx, c, _ptr(px, C.c_double), _ptr(av, C.c_double), _ptr(va, C.c_double)), "drt_read_lobe_film")
        return px, av, va

    def lobe_film_device_ptrs(self, c):
        a, b, d = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self.L.drt_lobe_film_device_ptrs(self.ctx, _u32(c, "lobe_film_device_ptrs: c"), C.byref(a), C.byref(b), C.byref(d)),
               "drt_lobe_film_device_ptrs")
        return a.value, b.value, d.value

    def read_lobe_xyz(self, c):
        """[P][3]: drt_read_xyz's conversion of lobe film c"""
        out = np.empty((self.n_pixels, 3))
        _check(self.L.drt_read_lobe_xyz(self.ctx, _u32(c, "read_lobe_xyz: c"), _ptr(out, C.c_double)), "drt_read_lobe_xyz")
        return out

    def read_lobe_bgra(self, c, which=1):
        """BMP pixel bytes [P][4] = B, G, R, 255 of lobe film c, as read_bgra"""
        out = np.empty((self.n_pixels, 4), dtype=np.uint8)
        _check(self.L.drt_read_lobe_bgra(self.ctx, _u32(c, "read_lobe_bgra: c"), int(which), _ptr(out, C.c_uint8)), "drt_read_lobe_bgra")
        return out

    def bind_sensor(self, curves):
        """drt_bind_sensor: a sensor film of one channel per curve ([n][S], at most MAX_SENSOR_CHANNELS) beside the main film, on a
        film without samples. None or an empty sequence unbinds."""
        arr, n = _sensor_curves(curves, self.S)
        _check(self.L.drt_bind_sensor(self.ctx, None if arr is None else _ptr(arr, C.c_double), n), "drt_bind_sensor")
        self.n_sensor = n

    def read_sensor_film(self):
        """(pixels [P][n + 1], means [P][n], variances [P][n]) of the sensor film"""
        n = getattr(self, "n_sensor", 0)
        px = np.empty((self.n_pixels, n + 1), dtype=np.float64)
        av = np.empty((self.n_pixels, n), dtype=np.float64)
        va = np.empty((self.n_pixels, n), dtype=np.float64)
        _check(self.L.drt_read_sensor_film(self.ctx, _ptr(px, C.c_double), _ptr(av, C.c_double), _ptr(va, C.c_double)), "drt_read_sensor_film")
        return px, av, va

    def sensor_film_device_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self.L.drt_sensor_film_device_ptrs(self.ctx, C.byref(a), C.byref(b), C.byref(c)), "drt_sensor_film_device_ptrs")
        return a.value, b.value, c.value

    def read_sensor_bgra(self, which, matrix):
        """BMP pixel bytes [n][4] = B, G, R, 255 of the sensor film's sum / filter (0) or mean (1) through the 3 x n matrix"""
        n = getattr(self, "n_sensor", 0)
        if n == 0:
            _check(self.L.drt_read_sensor_bgra(self.ctx, int(which), None, None), "drt_read_sensor_bgra")
        m = _sensor_matrix(matrix, n)
        out = np.empty((self.n_pixels, 4), dtype=np.uint8)
        _check(self.L.drt_read_sensor_bgra(self.ctx, int(which), _ptr(m, C.c_double), _ptr(out, C.c_uint8)), "drt_read_sensor_bgra")
        return out

    def read_hit_indices(self, num_samples):
        n = self.n_pixels * num_samples
        out = np.empty((n, int(self.params.max_depth)), dtype=np.int32)
        _check(self.L.drt_read_hit_indices(self.ctx, _ptr(out, C.c_int32), n), "drt_read_hit_indices")
        return out

    def batch_spp(self):
        return int(self.L.drt_batch_spp(self.ctx))

    def shade_instantiation(self):
        """which shade kernel the context's dense launches run: "general", "simple" or "closed" (drt_shade_instantiation)"""
        return SHADE_INSTANTIATIONS[int(self.L.drt_shade_instantiation(self.ctx))]

    def shade_closed_lds(self):
        """whether the closed instantiation runs in its form with window headers in LDS, five waves per SIMD (drt_shade_closed_lds)"""
        return int(self.L.drt_shade_closed_lds(self.ctx)) == 1

    def shade_closed_waves(self):
        """waves per SIMD of the closed kernel a context's dense launches run: 6 (drt_shade_kernel_closed_lds6, workgroups of 512 lanes),
        5 (drt_shade_kernel_closed_lds), 4 (drt_shade_kernel_closed); 0: not the closed instantiation (drt_shade_closed_waves)"""
        return int(self.L.drt_shade_closed_waves(self.ctx))

    def stats(self):
        st = Stats()
        _check(self.L.drt_get_stats(self.ctx, C.byref(st)), "drt_get_stats")
        return st

    def render_adaptive(self, min_spp, max_spp, step, rel_error, floor=0.0):
        """Adaptive sampling (drt_render_adaptive): returns {"rounds", "pixels_at_max", "paths"}."""
        a = make_adaptive(min_spp, max_spp, step, rel_error, floor)
        _check(self.L.drt_render_adaptive(self.ctx, C.byref(a)), "drt_render_adaptive")
        return {"rounds": a.rounds, "pixels_at_max": a.pixels_at_max, "paths": a.paths}

    def render_adaptive_continue(self, max_spp, step, rel_error, floor=0.0, max_rounds=0):
        """Adaptive sampling continued on the film the context holds (drt_render_adaptive_continue), every pixel from its own count;
        max_rounds = 0: to the end. Returns {"rounds", "pixels_at_max", "paths", "still_active"}: rounds and paths of this call."""
        a = make_adaptive(2, max_spp, step, rel_error, floor)  # (min_spp is not used: the smallest the checks accept)
        left = C.c_uint32()
        _check(self.L.drt_render_adaptive_continue(self.ctx, C.byref(a), max_rounds, C.byref(left)), "drt_render_adaptive_continue")
        return {"rounds": a.rounds, "pixels_at_max": a.pixels_at_max, "paths": a.paths, "still_active": left.value}

    def denoise(self, radius=5, patch=1, k=1.0, alpha=1.0):
        """Variance-guided denoising of the film the context holds (drt_denoise_film), into buffers of the context's own: the film
        itself does not change. Returns {"unusable", "kernel_ms"}; read_denoised() / read_denoised_bgra() fetch the result."""
        d = make_denoise(radius, patch, k, alpha)
        _check(self.L.drt_denoise_film(self.ctx, C.byref(d)), "drt_denoise_film")
        return {"unusable": d.unusable, "kernel_ms": d.kernel_ms}

    def read_denoised(self):
        """(mean', var') of the last denoise(), [n][S] each"""
        mean = np.empty((self.n_pixels, self.S), dtype=np.float64)
        var = np.empty((self.n_pixels, self.S), dtype=np.float64)
        _check(self.L.drt_read_denoised(self.ctx, _ptr(mean, C.c_double), _ptr(var, C.c_double)), "drt_read_denoised")
        return mean, var

    def read_denoised_bgra(self):
        """BMP pixel bytes [n][4] of the denoised mean (the conversion of read_bgra(1))"""
        out = np.empty((self.n_pixels, 4), dtype=np.uint8)
        _check(self.L.drt_read_denoised_bgra(self.ctx, _ptr(out, C.c_uint8)), "drt_read_denoised_bgra")
        return out

    def render_features(self, n_samples=0, first_sample=0, flags=0):
        """First-hit feature buffers (drt_render_features) into buffers of the context's own: n_samples of every pixel from
        first_sample on, or (0) each pixel's count from the held film's filter column. The film and the render state do not
        change. Returns {"empty_pixels", "rays", "kernel_ms"}; read_features() / read_feature_bgra() fetch the result."""
        f = make_features(n_samples, first_sample)
        f.flags = flags
        _check(self.L.drt_render_features(self.ctx, C.byref(f)), "drt_render_features")
        return {"empty_pixels": f.empty_pixels, "rays": f.rays, "kernel_ms": f.kernel_ms}

    def read_features(self):
        """(mean [n][8], m2 [n][8], ids [n] int32) of the last render_features()"""
        mean = np.empty((self.n_pixels, FEATURE_CHANNELS), dtype=np.float64)
        m2 = np.empty((self.n_pixels, FEATURE_CHANNELS), dtype=np.float64)
        ids = np.empty(self.n_pixels, dtype=np.int32)
        _check(self.L.drt_read_features(self.ctx, _ptr(mean, C.c_double), _ptr(m2, C.c_double), _ptr(ids, C.c_int32)), "drt_read_features")
        return mean, m2, ids

    def read_feature_bgra(self, which, lo, hi):
        """BMP pixel bytes [n][4] of the mean normal (FEATURE_NORMAL: x, y, z to R, G, B), depth or coverage (grey), [lo, hi] to 0..255"""
        out = np.empty((self.n_pixels, 4), dtype=np.uint8)
        _check(self.L.drt_read_feature_bgra(self.ctx, int(which), float(lo), float(hi), _ptr(out, C.c_uint8)), "drt_read_feature_bgra")
        return out

    def render_mattes(self, n_samples=0, first_sample=0, flags=0):
        """ID mattes (drt_render_mattes) into buffers of the context's own: n_samples of every pixel from first_sample on, or (0)
        each pixel's count from the held film's filter column. The film, the render state and the feature buffers do not change.
        Returns {"empty_pixels", "overflow_pixels", "rays", "kernel_ms"}; read_mattes() / read_matte() / read_matte_bgra() fetch the result."""
        m = make_mattes(n_samples, first_sample)
        m.flags = flags
        _check(self.L.drt_render_mattes(self.ctx, C.byref(m)), "drt_render_mattes")
        return _mattes_report(m)

    def read_mattes(self):
        """(ids [n][2][6] int32, counts [n][2][6] uint32, tail [n][4] uint32 = c_p, misses, other per layer) of the last render_mattes()"""
        ids = np.empty((self.n_pixels, MATTE_LAYERS, MATTE_SLOTS), dtype=np.int32)
        counts = np.empty((self.n_pixels, MATTE_LAYERS, MATTE_SLOTS), dtype=np.uint32)
        tail = np.empty((self.n_pixels, 4), dtype=np.uint32)
        _check(self.L.drt_read_mattes(self.ctx, _ptr(ids, C.c_int32), _ptr(counts, C.c_uint32), _ptr(tail, C.c_uint32)), "drt_read_mattes")
        return ids, counts, tail

    def read_matte(self, layer, id_list):
        """coverage [n]: the share of every pixel's samples whose id in the layer is in id_list (MATTE_ID_MISS: the misses)"""
        lst = np.ascontiguousarray(id_list, dtype=np.int32).reshape(-1)
        out = np.empty(self.n_pixels, dtype=np.float64)
        _check(self.L.drt_read_matte(self.ctx, int(layer), _ptr(lst, C.c_int32), len(lst), _ptr(out, C.c_double)), "drt_read_matte")
        return out

    def read_matte_bgra(self, layer):
        """BMP pixel bytes [n][4] of a layer's preview: every slot's palette colour weighted by its share"""
        out = np.empty((self.n_pixels, 4), dtype=np.uint8)
        _check(self.L.drt_read_matte_bgra(self.ctx, int(layer), _ptr(out, C.c_uint8)), "drt_read_matte_bgra")
        return out

    def cast_rays(self, origins, dirs):
        """Closest hits of caller-supplied rays (drt_cast_rays). numpy arrays [n][3]: host mode, returns a RAY_HIT_DTYPE record array
        [n]. Contiguous float64 torch tensors on the context's device: device mode, enqueued on the context's stream without waiting;
        returns a uint8 tensor [n][104] (view it as RAY_HIT_DTYPE after .cpu().numpy())."""
        if _is_tensor(origins) or _is_tensor(dirs):
            torch = sys.modules["torch"]
            dev = int(self.params.device)
            o, d = _rays_tensor(origins, "origins", dev), _rays_tensor(dirs, "dirs", dev)
            if o.shape != d.shape:
                raise ValueError("origins and dirs: the same shape")
            hits = torch.empty((o.shape[0], 104), dtype=torch.uint8, device=o.device)
            _check(self.L.drt_cast_rays(self.ctx, o.data_ptr(), d.data_ptr(), o.shape[0], hits.data_ptr(), RAYS_DEVICE), "drt_cast_rays")
            return hits
        o, d = _rays_f64(origins, "origins"), _rays_f64(dirs, "dirs")
        if o.shape != d.shape:
            raise ValueError("origins and dirs: the same shape")
        hits = np.zeros(o.shape[0], dtype=RAY_HIT_DTYPE)
        _check(self.L.drt_cast_rays(self.ctx, o.ctypes.data, d.ctypes.data, o.shape[0], hits.ctypes.data, 0), "drt_cast_rays")
        return hits

    def test_visibility(self, p0, p1):
        """points_mutually_visible of caller-supplied pairs (drt_test_visibility): uint8 [n], 1 visible. numpy arrays: host mode;
        torch tensors on the context's device: device mode, a uint8 tensor, enqueued without waiting."""
        if _is_tensor(p0) or _is_tensor(p1):
            torch = sys.modules["torch"]
            dev = int(self.params.device)
            a, b = _rays_tensor(p0, "p0", dev), _rays_tensor(p1, "p1", dev)
            if a.shape != b.shape:
                raise ValueError("p0 and p1: the same shape")
            vis = torch.empty(a.shape[0], dtype=torch.uint8, device=a.device)
            _check(self.L.drt_test_visibility(self.ctx, a.data_ptr(), b.data_ptr(), a.shape[0], vis.data_ptr(), RAYS_DEVICE), "drt_test_visibility")
            return vis
        a, b = _rays_f64(p0, "p0"), _rays_f64(p1, "p1")
        if a.shape != b.shape:
            raise ValueError("p0 and p1: the same shape")
        vis = np.zeros(a.shape[0], dtype=np.uint8)
        _check(self.L.drt_test_visibility(self.ctx, a.ctypes.data, b.ctypes.data, a.shape[0], vis.ctypes.data, 0), "drt_test_visibility")
        return vis

    def cast_pixels(self, xy, samples):
        """The path's own camera ray of pixel xy[i] = (x, y) of the whole image and sample samples[i], and its closest hit
        (drt_cast_pixels). Returns (origins [n][3], dirs [n][3], hits). numpy arrays: host mode; int32 / uint32-valued torch tensors
        (dtype int32, values below 2^31) on the context's device: device mode, tensors back, enqueued without waiting."""
        if _is_tensor(xy) or _is_tensor(samples):
            torch = sys.modules["torch"]
            dev = int(self.params.device)
            for t, name in ((xy, "xy"), (samples, "samples")):
                if t.dtype != torch.int32 or not t.is_contiguous() or t.device.type != "cuda" or t.device.index != dev:
                    raise ValueError("%s: a contiguous int32 tensor on the context's device (cuda:%d)" % (name, dev))
            if xy.dim() != 2 or xy.shape[1] != 2 or samples.dim() != 1 or samples.shape[0] != xy.shape[0]:
                raise ValueError("xy: an [n][2] tensor, samples: [n]")
            n = xy.shape[0]
            o = torch.empty((n, 3), dtype=torch.float64, device=xy.device)
            d = torch.empty((n, 3), dtype=torch.float64, device=xy.device)
            hits = torch.empty((n, 104), dtype=torch.uint8, device=xy.device)
            _check(self.L.drt_cast_pixels(self.ctx, xy.data_ptr(), samples.data_ptr(), n, o.data_ptr(), d.data_ptr(), hits.data_ptr(), RAYS_DEVICE),
                   "drt_cast_pixels")
            return o, d, hits
        xy, samples = _pixels_u32(xy, samples)
        n = xy.shape[0]
        o, d, hits = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=RAY_HIT_DTYPE)
        _check(self.L.drt_cast_pixels(self.ctx, xy.ctypes.data, samples.ctypes.data, n, o.ctypes.data, d.ctypes.data, hits.ctypes.data, 0), "drt_cast_pixels")
        return o, d, hits

    def bind_rays(self, origins, dirs=None, weights=None):
        """A ray film (drt_bind_rays): from now on the path of image pixel (x, y), sample s starts with origins[s % L][y][x],
        dirs[s % L][y][x] and is weighted by weights[s % L][y][x] (None: 1.0). numpy arrays [L][h][w][3] or [h][w][3] over the WHOLE
        image: host mode, the tile's rows are copied. float64 torch tensors on the context's device: device mode, used in place and
        kept referenced until the next bind_rays. bind_rays(None) goes back to the camera. The film must hold no samples."""
        if origins is None:
            _check(self.L.drt_bind_rays(self.ctx, None), "drt_bind_rays")
            self._ray_arrays = None
            return
        t, keep = _ray_table(origins, dirs, weights, int(self.params.width), int(self.params.height), int(self.params.device))
        _check(self.L.drt_bind_rays(self.ctx, C.byref(t)), "drt_bind_rays")
        self._ray_arrays = keep if t.flags & RAYS_DEVICE else None

    def set_camera(self, camera_or_bundle):
        """drt_set_camera: from now on the context renders through this camera (a Camera, or a SceneBundle's). The film must hold no
        samples. Bit for bit a fresh context's results with that camera."""
        cam = _camera_of(camera_or_bundle)
        _check(self.L.drt_set_camera(self.ctx, C.byref(cam)), "drt_set_camera")

    def update_surfaces(self, surfaces, first=0, rebuild=False):
        """drt_update_surfaces: surfaces [first, first + n) replaced; types, materials and the surface count stay. A ctypes Surface array
        or a numpy [n][14] float64 array of raw rows (surface_rows): host mode, checked before anything changes. A float64 torch tensor
        [n][14] on the context's device: device mode, enqueued on the context's stream without waiting. rebuild: build the hierarchy anew
        (host mode only). The film must hold no samples. Bit for bit a fresh context's results on the updated scene."""
        ptr, n, flags, keep = _update_args(surfaces, int(self.params.device))
        if rebuild:
            flags |= SURFACES_REBUILD
        _check(self.L.drt_update_surfaces(self.ctx, ptr, first, n, flags), "drt_update_surfaces")
        if flags & SURFACES_DEVICE:
            self._update_rows = keep  # until the stream has read it: the next update or close() at the latest

    def update_spectra(self, rows, first=0):
        """drt_update_spectra: rows [first, first + n) of the scene's SPD table (SceneBundle.spds numbering) replaced. A numpy [n][S]
        float64 array: host mode, checked before anything changes. A float64 torch tensor [n][S] on the context's device: device mode,
        enqueued on the context's stream without waiting. The colour-matching rows are refused; the film must hold no samples. Bit for
        bit a fresh context's results on the scene with those rows."""
        ptr, n, flags, keep = _spectra_args(rows, self.S, int(self.params.device))
        _check(self.L.drt_update_spectra(self.ctx, ptr, first, n, flags), "drt_update_spectra")
        if flags & SPECTRA_DEVICE:
            self._spectra_rows = keep  # until the stream has read it: the next update or close() at the latest

    def update_materials(self, materials, first=0):
        """drt_update_materials: materials [first, first + n) given the shininess and roughness of these Material records (a ctypes
        array or a sequence); every other field must equal what the context holds. The film must hold no samples."""
        ptr, n, _keep = _materials_args(materials)
        _check(self.L.drt_update_materials(self.ctx, ptr, first, n, 0), "drt_update_materials")

    def update_report(self):
        """drt_get_update_report: {"updates", "refits_since_build", "extent", "kernel_ms"}"""
        r = UpdateReport()
        _check(self.L.drt_get_update_report(self.ctx, C.byref(r)), "drt_get_update_report")
        return {n: getattr(r, n) for n, _ in r._fields_}

    def rebuild_hierarchy(self):
        """drt_rebuild_hierarchy: the hierarchy built anew on the device from the context's current surfaces, enqueued on the context's
        stream without waiting. No result changes by a bit; needs no empty film; nothing happens in a context without the hierarchy."""
        _check(self.L.drt_rebuild_hierarchy(self.ctx, 0), "drt_rebuild_hierarchy")

    def hierarchy_report(self):
        """drt_get_hierarchy_report: {"nodes", "leaf_surfaces", "depth", "device_builds", "built_by", "kernel_ms"}"""
        r = HierarchyReport()
        _check(self.L.drt_get_hierarchy_report(self.ctx, C.byref(r)), "drt_get_hierarchy_report")
        return {n: getattr(r, n) for n, _ in r._fields_ if n != "pad"}

    def read_hierarchy(self):
        """drt_read_hierarchy: (nodes, leaf_surface) -- the tree in use as a BVH_NODE structured array, and the surface index in every
        leaf slot (uint32)"""
        rep = self.hierarchy_report()
        nodes = np.zeros(rep["nodes"], dtype=BVH_NODE)
        leaf = np.zeros(rep["leaf_surfaces"], dtype=np.uint32)
        _check(self.L.drt_read_hierarchy(self.ctx, nodes.ctypes.data, len(nodes), _ptr(leaf, C.c_uint32), len(leaf)), "drt_read_hierarchy")
        return nodes, leaf

    def read_sample_counts(self):
        out = np.empty((int(self.params.tile_h), int(self.params.tile_w)), dtype=np.uint32)
        _check(self.L.drt_read_sample_counts(self.ctx, _ptr(out, C.c_uint32)), "drt_read_sample_counts")
        return out

    def render_sample_map(self, targets, add=False):
        """Every tile pixel rendered to the count `targets` gives it (drt_render_sample_map; add: that many more samples). targets: a
        numpy integer array (tile_h, tile_w) or flat; a torch int32 / uint32 tensor on the context's device, which the library reads
        where it is; or a torch CPU tensor. Returns {"rounds", "paths", "pixels_rendered", "pixels_above", "max_count"}."""
        m = SampleMap()
        m.flags = MAP_ADD if add else 0
        tw, th = int(self.params.tile_w), int(self.params.tile_h)
        if _is_tensor(targets) and targets.device.type != "cpu":
            torch = sys.modules["torch"]
            t = targets
            if t.dtype not in (torch.int32, torch.uint32):
                raise ValueError("render_sample_map: a device tensor of int32 or uint32 (int32 values are read as unsigned)")
            if tuple(t.shape) not in ((th, tw), (th * tw,)) or not t.is_contiguous():
                raise ValueError("render_sample_map: a contiguous tensor of shape (%d, %d) or (%d,)" % (th, tw, th * tw))
            if t.device.type != "cuda" or t.device.index != int(self.params.device):
                raise ValueError("render_sample_map: a tensor on the context's device (cuda:%d)" % int(self.params.device))
            torch.cuda.current_stream(t.device).synchronize()  # what filled the tensor is done before the context's stream reads it
            m.targets = t.data_ptr()
            m.flags |= MAP_DEVICE
            keep = t
        else:
            if _is_tensor(targets):
                torch = sys.modules["torch"]
                targets = targets.view(torch.int32).numpy().view(np.uint32) if targets.dtype == torch.uint32 else targets.numpy()
            keep = _map_u32(targets, tw, th, "render_sample_map")
            m.targets = keep.ctypes.data
        _check(self.L.drt_render_sample_map(self.ctx, C.byref(m)), "drt_render_sample_map")
        del keep
        return _map_report(m)

    def read_active_list(self):
        """the tile pixels still active after the last adaptive round (DRT_ADAPTIVE_ROUNDS stops a render early), ascending"""
        out = np.empty(self.n_pixels, dtype=np.uint32)
        n = C.c_uint32()
        _check(self.L.drt_read_active_list(self.ctx, _ptr(out, C.c_uint32), self.n_pixels, C.byref(n)), "drt_read_active_list")
        return out[:n.value].copy()


class Group:
    """drt_group_*: one host thread, several GPUs; the tile's rows dealt cyclically over `devices` (None: all visible)."""

    def __init__(self, bundle, params, devices=None):
        self.L = hip_lib()
        self.bundle, self.params, self.S = bundle, params, bundle.S
        self.n_pixels = int(params.tile_w) * int(params.tile_h)
        if devices is None:
            arr, n = None, 0
        else:
            arr, n = (C.c_int32 * len(devices))(*devices), len(devices)
        self.g = self.L.drt_group_create(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(params), arr, n)
        if not self.g:
            raise RuntimeError("drt_group_create: " + self.L.drt_last_error().decode())

    def size(self):
        return int(self.L.drt_group_size(self.g))

    def render(self, first_sample=None, num_samples=None):
        fs = int(self.params.first_sample) if first_sample is None else first_sample
        ns = int(self.params.spp) if num_samples is None else num_samples
        _check(self.L.drt_group_render(self.g, fs, ns), "drt_group_render")

    def read_film(self):
        px = np.empty((self.n_pixels, self.S + 1)); av = np.empty((self.n_pixels, self.S)); va = np.empty((self.n_pixels, self.S))
        f64p = C.POINTER(C.c_double)
        _check(self.L.drt_group_read_film(self.g, px.ctypes.data_as(f64p), av.ctypes.data_as(f64p), va.ctypes.data_as(f64p)), "drt_group_read_film")
        return px, av, va

    def write_film(self, px, av, va):
        f64p = C.POINTER(C.c_double)
        px, av, va = (np.ascontiguousarray(a, dtype=np.float64) for a in (px, av, va))
        _check(self.L.drt_group_write_film(self.g, px.ctypes.data_as(f64p), av.ctypes.data_as(f64p), va.ctypes.data_as(f64p)), "drt_group_write_film")

    def stats(self):
        st = Stats()
        _check(self.L.drt_group_get_stats(self.g, C.byref(st)), "drt_group_get_stats")
        return st

    def render_adaptive(self, min_spp, max_spp, step, rel_error, floor=0.0):
        """drt_group_render_adaptive: returns {"rounds", "pixels_at_max", "paths"} (rounds: the most any device ran)."""
        a = make_adaptive(min_spp, max_spp, step, rel_error, floor)
        _check(self.L.drt_group_render_adaptive(self.g, C.byref(a)), "drt_group_render_adaptive")
        return {"rounds": a.rounds, "pixels_at_max": a.pixels_at_max, "paths": a.paths}

    def render_adaptive_continue(self, max_spp, step, rel_error, floor=0.0, max_rounds=0):
        """drt_group_render_adaptive_continue: as Renderer.render_adaptive_continue (rounds: the most any device ran; still_active: all devices')."""
        a = make_adaptive(2, max_spp, step, rel_error, floor)
        left = C.c_uint32()
        _check(self.L.drt_group_render_adaptive_continue(self.g, C.byref(a), max_rounds, C.byref(left)), "drt_group_render_adaptive_continue")
        return {"rounds": a.rounds, "pixels_at_max": a.pixels_at_max, "paths": a.paths, "still_active": left.value}

    def read_sample_counts(self):
        out = np.empty((int(self.params.tile_h), int(self.params.tile_w)), dtype=np.uint32)
        _check(self.L.drt_group_read_sample_counts(self.g, _ptr(out, C.c_uint32)), "drt_group_read_sample_counts")
        return out

    def render_sample_map(self, targets, add=False):
        """drt_group_render_sample_map: as Renderer.render_sample_map, from a host array over the whole tile in image order."""
        if _is_tensor(targets):
            raise ValueError("Group.render_sample_map: a host array (device maps are per context)")
        m = SampleMap()
        m.flags = MAP_ADD if add else 0
        keep = _map_u32(targets, int(self.params.tile_w), int(self.params.tile_h), "Group.render_sample_map")
        m.targets = keep.ctypes.data
        _check(self.L.drt_group_render_sample_map(self.g, C.byref(m)), "drt_group_render_sample_map")
        del keep
        return _map_report(m)

    def denoise(self, radius=5, patch=1, k=1.0, alpha=1.0):
        """drt_group_denoise: the group's film gathered and filtered on its first device. Returns (mean', var', {"unusable", "kernel_ms"})."""
        d = make_denoise(radius, patch, k, alpha)
        mean = np.empty((self.n_pixels, self.S), dtype=np.float64)
        var = np.empty((self.n_pixels, self.S), dtype=np.float64)
        _check(self.L.drt_group_denoise(self.g, C.byref(d), _ptr(mean, C.c_double), _ptr(var, C.c_double)), "drt_group_denoise")
        return mean, var, {"unusable": d.unusable, "kernel_ms": d.kernel_ms}

    def render_features(self, n_samples=0, first_sample=0):
        """drt_group_render_features: every device its own rows. Returns (mean, m2, ids, {"empty_pixels", "rays", "kernel_ms"}), image order."""
        f = make_features(n_samples, first_sample)
        mean = np.empty((self.n_pixels, FEATURE_CHANNELS), dtype=np.float64)
        m2 = np.empty((self.n_pixels, FEATURE_CHANNELS), dtype=np.float64)
        ids = np.empty(self.n_pixels, dtype=np.int32)
        _check(self.L.drt_group_render_features(self.g, C.byref(f), _ptr(mean, C.c_double), _ptr(m2, C.c_double), _ptr(ids, C.c_int32)),
               "drt_group_render_features")
        return mean, m2, ids, {"empty_pixels": f.empty_pixels, "rays": f.rays, "kernel_ms": f.kernel_ms}

    def render_mattes(self, n_samples=0, first_sample=0):
        """drt_group_render_mattes: every device its own rows. Returns (ids, counts, tail, report) as Renderer.read_mattes(), image order."""
        m = make_mattes(n_samples, first_sample)
        ids = np.empty((self.n_pixels, MATTE_LAYERS, MATTE_SLOTS), dtype=np.int32)
        counts = np.empty((self.n_pixels, MATTE_LAYERS, MATTE_SLOTS), dtype=np.uint32)
        tail = np.empty((self.n_pixels, 4), dtype=np.uint32)
        _check(self.L.drt_group_render_mattes(self.g, C.byref(m), _ptr(ids, C.c_int32), _ptr(counts, C.c_uint32), _ptr(tail, C.c_uint32)),
               "drt_group_render_mattes")
        return ids, counts, tail, _mattes_report(m)

    def cast_rays(self, origins, dirs):
        """drt_group_cast_rays: the list in contiguous shares, one per device; a RAY_HIT_DTYPE record array in list order."""
        o, d = _rays_f64(origins, "origins"), _rays_f64(dirs, "dirs")
        if o.shape != d.shape:
            raise ValueError("origins and dirs: the same shape")
        hits = np.zeros(o.shape[0], dtype=RAY_HIT_DTYPE)
        _check(self.L.drt_group_cast_rays(self.g, o.ctypes.data, d.ctypes.data, o.shape[0], hits.ctypes.data), "drt_group_cast_rays")
        return hits

    def test_visibility(self, p0, p1):
        """drt_group_test_visibility: uint8 [n] in list order."""
        a, b = _rays_f64(p0, "p0"), _rays_f64(p1, "p1")
        if a.shape != b.shape:
            raise ValueError("p0 and p1: the same shape")
        vis = np.zeros(a.shape[0], dtype=np.uint8)
        _check(self.L.drt_group_test_visibility(self.g, a.ctypes.data, b.ctypes.data, a.shape[0], vis.ctypes.data), "drt_group_test_visibility")
        return vis

    def cast_pixels(self, xy, samples):
        """drt_group_cast_pixels: (origins, dirs, hits) in list order."""
        xy, samples = _pixels_u32(xy, samples)
        n = xy.shape[0]
        o, d, hits = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=RAY_HIT_DTYPE)
        _check(self.L.drt_group_cast_pixels(self.g, xy.ctypes.data, samples.ctypes.data, n, o.ctypes.data, d.ctypes.data, hits.ctypes.data),
               "drt_group_cast_pixels")
        return o, d, hits

    def bind_rays(self, origins, dirs=None, weights=None):
        """drt_group_bind_rays: as Renderer.bind_rays with numpy arrays (host mode only); every device copies its own rows."""
        if origins is None:
            _check(self.L.drt_group_bind_rays(self.g, None), "drt_group_bind_rays")
            return
        if _is_tensor(origins) or _is_tensor(dirs) or _is_tensor(weights):
            raise ValueError("Group.bind_rays: numpy arrays (a group takes host pointers only)")
        t, _ = _ray_table(origins, dirs, weights, int(self.params.width), int(self.params.height), 0)
        _check(self.L.drt_group_bind_rays(self.g, C.byref(t)), "drt_group_bind_rays")

    def bind_depth_cuts(self, depths):
        """drt_group_bind_depth_cuts: as Renderer.bind_depth_cuts, every context checked before any is changed"""
        arr, n = _depth_array(depths)
        _check(self.L.drt_group_bind_depth_cuts(self.g, arr, n), "drt_group_bind_depth_cuts")

    def read_depth_film(self, cut):
        """drt_group_read_depth_film: cut film `cut` of the whole tile, in image order"""
        px = np.empty((self.n_pixels, self.S + 1)); av = np.empty((self.n_pixels, self.S)); va = np.empty((self.n_pixels, self.S))
        f64p = C.POINTER(C.c_double)
        _check(self.L.drt_group_read_depth_film(self.g, int(cut), px.ctypes.data_as(f64p), av.ctypes.data_as(f64p), va.ctypes.data_as(f64p)),
               "drt_group_read_depth_film")
        return px, av, va

    def bind_buckets(self, n):
        """drt_group_bind_buckets: as Renderer.bind_buckets, every context checked and every film allocated before any is changed"""
        n = _u32(0 if n is None else n, "bind_buckets: n")
        _check(self.L.drt_group_bind_buckets(self.g, n), "drt_group_bind_buckets")
        self.n_buckets = n

    def read_bucket_film(self, b):
        """drt_group_read_bucket_film: bucket b's film of the whole tile, in image order"""
        b = _u32(b, "read_bucket_film: b")
        if not getattr(self, "n_buckets", 0) or b >= self.n_buckets:
            _check(self.L.drt_group_read_bucket_film(self.g, b, None, None, None), "drt_group_read_bucket_film")
        px, av, va = np.empty((self.n_pixels, self.S + 1)), np.empty((self.n_pixels, self.S)), np.empty((self.n_pixels, self.S))
        f64p = C.POINTER(C.c_double)
        _check(self.L.drt_group_read_bucket_film(self.g, b, px.ctypes.data_as(f64p), av.ctypes.data_as(f64p), va.ctypes.data_as(f64p)),
               "drt_group_read_bucket_film")
        return px, av, va

    def resolve_buckets(self, trim=None):
        """drt_group_resolve_buckets: as Renderer.resolve_buckets on every device, every context checked before any resolves"""
        n = getattr(self, "n_buckets", 0)
        t = max(n - 1, 0) // 2 if trim is None else _u32(trim, "resolve_buckets: trim")
        _check(self.L.drt_group_resolve_buckets(self.g, t), "drt_group_resolve_buckets")

    def read_bucket_resolve(self):
        """drt_group_read_bucket_resolve: (estimate, error) of the whole tile, in image order"""
        _check(self.L.drt_group_read_bucket_resolve(self.g, None, None), "drt_group_read_bucket_resolve")
        est, err = np.empty((self.n_pixels, self.S)), np.empty((self.n_pixels, self.S))
        f64p = C.POINTER(C.c_double)
        _check(self.L.drt_group_read_bucket_resolve(self.g, est.ctypes.data_as(f64p), err.ctypes.data_as(f64p)), "drt_group_read_bucket_resolve")
        return est, err

    def bind_lobes(self, map_or_preset, n=None):
        """drt_group_bind_lobes: as Renderer.bind_lobes, every context checked and every film allocated before any is changed"""
        n, m = _lobe_bind_args(map_or_preset, n)
        _check(self.L.drt_group_bind_lobes(self.g, n, C.byref(m) if m is not None else None), "drt_group_bind_lobes")
        self.n_lobes = n

    def read_lobe_film(self, c):
        """drt_group_read_lobe_film: lobe film c of the whole tile, in image order"""
        c = _u32(c, "read_lobe_film: c")
        if not getattr(self, "n_lobes", 0) or c >= self.n_lobes:
            _check(self.L.drt_group_read_lobe_film(self.g, c, None, None, None), "drt_group_read_lobe_film")
        px, av, va = np.empty((self.n_pixels, self.S + 1)), np.empty((self.n_pixels, self.S)), np.empty((self.n_pixels, self.S))
        f64p = C.POINTER(C.c_double)
        _check(self.L.drt_group_read_lobe_film(self.g, c, px.ctypes.data_as(f64p), av.ctypes.data_as(f64p), va.ctypes.data_as(f64p)),
               "drt_group_read_lobe_film")
        return px, av, va

    def bind_sensor(self, curves):
        """drt_group_bind_sensor: as Renderer.bind_sensor, every context checked and every film allocated before any is changed"""
        arr, n = _sensor_curves(curves, self.S)
        _check(self.L.drt_group_bind_sensor(self.g, None if arr is None else _ptr(arr, C.c_double), n), "drt_group_bind_sensor")
        self.n_sensor = n

    def read_sensor_film(self):
        """drt_group_read_sensor_film: the sensor film of the whole tile, in image order"""
        n = getattr(self, "n_sensor", 0)
        px = np.empty((self.n_pixels, n + 1)); av = np.empty((self.n_pixels, n)); va = np.empty((self.n_pixels, n))
        f64p = C.POINTER(C.c_double)
        _check(self.L.drt_group_read_sensor_film(self.g, px.ctypes.data_as(f64p), av.ctypes.data_as(f64p), va.ctypes.data_as(f64p)),
               "drt_group_read_sensor_film")
        return px, av, va

    def reset_film(self):
        _check(self.L.drt_group_reset_film(self.g), "drt_group_reset_film")

    def set_camera(self, camera_or_bundle):
        """drt_group_set_camera: every context is checked before any is changed"""
        cam = _camera_of(camera_or_bundle)
        _check(self.L.drt_group_set_camera(self.g, C.byref(cam)), "drt_group_set_camera")

    def update_surfaces(self, surfaces, first=0, rebuild=False):
        """drt_group_update_surfaces: as Renderer.update_surfaces in host mode (a ctypes Surface array or numpy rows)"""
        if _is_tensor(surfaces):
            raise ValueError("Group.update_surfaces: a Surface array or numpy rows (a group takes host pointers only)")
        ptr, n, flags, _keep = _update_args(surfaces, 0)
        _check(self.L.drt_group_update_surfaces(self.g, ptr, first, n, flags | (SURFACES_REBUILD if rebuild else 0)), "drt_group_update_surfaces")

    def update_spectra(self, rows, first=0):
        """drt_group_update_spectra: as Renderer.update_spectra in host mode (numpy rows)"""
        if _is_tensor(rows):
            raise ValueError("Group.update_spectra: numpy rows (a group takes host pointers only)")
        ptr, n, flags, _keep = _spectra_args(rows, self.S, 0)
        _check(self.L.drt_group_update_spectra(self.g, ptr, first, n, flags), "drt_group_update_spectra")

    def update_materials(self, materials, first=0):
        """drt_group_update_materials: as Renderer.update_materials"""
        ptr, n, _keep = _materials_args(materials)
        _check(self.L.drt_group_update_materials(self.g, ptr, first, n, 0), "drt_group_update_materials")

    def rebuild_hierarchy(self):
        """drt_group_rebuild_hierarchy: as Renderer.rebuild_hierarchy, every context from its own device copy of the surfaces"""
        _check(self.L.drt_group_rebuild_hierarchy(self.g, 0), "drt_group_rebuild_hierarchy")

    def close(self):
        if self.g:
            self.L.drt_group_destroy(self.g)
            self.g = None


def render_tile(bundle, params):
    """One-shot drt_render_tile with host buffers. Returns (pixels, avgs, vars, stats)."""
    L = hip_lib()
    n = int(params.tile_w) * int(params.tile_h)
    S = bundle.S
    px = np.zeros((n, S + 1), dtype=np.float64)
    av = np.zeros((n, S), dtype=np.float64)
    va = np.zeros((n, S), dtype=np.float64)
    st = Stats()
    rc = L.drt_render_tile(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(params), _ptr(px, C.c_double),
                           _ptr(av, C.c_double), _ptr(va, C.c_double), C.byref(st))
    _check(rc, "drt_render_tile")
    return px, av, va, st


def denoise_buffers(bundle, params, pixels, avgs, vars_, radius=5, patch=1, k=1.0, alpha=1.0):
    """One-shot drt_denoise_buffers on host buffers of a whole tile_w x tile_h film (a stored .spd triplet, say), on params.device.
    Returns (mean', var', {"unusable", "kernel_ms"})."""
    n, S = int(params.tile_w) * int(params.tile_h), bundle.S
    px = np.ascontiguousarray(pixels, dtype=np.float64).reshape(n, S + 1)
    av = np.ascontiguousarray(avgs, dtype=np.float64).reshape(n, S)
    va = np.ascontiguousarray(vars_, dtype=np.float64).reshape(n, S)
    d = make_denoise(radius, patch, k, alpha)
    mean = np.empty((n, S), dtype=np.float64)
    var = np.empty((n, S), dtype=np.float64)
    _check(hip_lib().drt_denoise_buffers(C.byref(bundle.scene), C.byref(params), C.byref(d), _ptr(px, C.c_double), _ptr(av, C.c_double),
                                         _ptr(va, C.c_double), _ptr(mean, C.c_double), _ptr(var, C.c_double)), "drt_denoise_buffers")
    return mean, var, {"unusable": d.unusable, "kernel_ms": d.kernel_ms}


def selftest_arith(op, a, b=None, device=0):
    a = np.ascontiguousarray(a, dtype=np.float64)
    n = a.size
    b = np.ascontiguousarray(b if b is not None else np.zeros_like(a), dtype=np.float64)
    out = np.empty(2 * n if op == 2 else n, dtype=np.float64)
    _check(hip_lib().drt_selftest_arith(device, op, _ptr(a, C.c_double), _ptr(b, C.c_double), _ptr(out, C.c_double), n),
           "drt_selftest_arith")
    return out


def selftest_path_ids(bases, steps, n_samples, tile_w, device=0):
    """The trace kernel's path-id arithmetic on the device: for each base id, the ids base .. base + sum(steps) - 1 handed out
    steps[k] at a time. Returns uint64 [len(bases)][sum(steps)][4]: pixel, sample, i, j (include/drt_hip.h)."""
    bases = np.ascontiguousarray(bases, dtype=np.uint64)
    steps = np.ascontiguousarray(steps, dtype=np.uint32)
    out = np.zeros((bases.size, int(steps.sum()), 4), dtype=np.uint64)
    _check(hip_lib().drt_selftest_path_ids(device, _ptr(bases, C.c_uint64), bases.size, _ptr(steps, C.c_uint32), steps.size, n_samples,
                                           tile_w, _ptr(out, C.c_uint64)), "drt_selftest_path_ids")
    return out


(UNIT_LINE_SPHERE, UNIT_LINE_PLANE, UNIT_REFLECT, UNIT_TRANSMIT, UNIT_ROTATION_BETWEEN, UNIT_SAMPLE_SPHERE, UNIT_SAMPLE_DISC,
 UNIT_GGX, UNIT_GGX_ATT, UNIT_FS_DIELECTRIC, UNIT_FS_CONDUCTOR, UNIT_SEED_AND_DRAW, UNIT_BVH_BOX, UNIT_LINE_PLANE_LIMITED,
 UNIT_BVH_SPHERE) = range(15)
_UNIT_OUT = {UNIT_LINE_SPHERE: 1, UNIT_LINE_PLANE: 1, UNIT_REFLECT: 3, UNIT_TRANSMIT: 3, UNIT_ROTATION_BETWEEN: 9,
             UNIT_SAMPLE_SPHERE: 4, UNIT_SAMPLE_DISC: 4, UNIT_GGX: 1, UNIT_GGX_ATT: 1, UNIT_FS_DIELECTRIC: 1, UNIT_FS_CONDUCTOR: 1,
             UNIT_SEED_AND_DRAW: 2, UNIT_BVH_BOX: 1, UNIT_LINE_PLANE_LIMITED: 1, UNIT_BVH_SPHERE: 2}


MAT_EVALUATE, MAT_SAMPLE = 0, 1
MAT_MODE_UNPAIRED, MAT_MODE_SIMPLE = 1, 2


def selftest_material(renderer, func, records):
    """The material layer of `renderer`'s device scene over `records` ([n][k] doubles, layouts in include/drt_hip.h; u64 arguments as
    their bit patterns): MAT_EVALUATE returns [n][S + 1] (reflectance, flags word), MAT_SAMPLE [n][6] (dir, 1/pdf, state bits, draws)."""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    n, k = rec.shape
    m = renderer.S + 1 if func == MAT_EVALUATE else 6
    out = np.zeros((n, m), dtype=np.float64)
    _check(hip_lib().drt_selftest_material(renderer.ctx, func, _ptr(rec, C.c_double), k, _ptr(out, C.c_double), m, n),
           "drt_selftest_material")
    return out


def bvh_stats(bundle):
    """(nodes, surfaces in leaves, levels, stack capacity) of the hierarchy the library builds for this scene; no GPU needed."""
    v = [C.c_uint32() for _ in range(4)]
    _check(hip_lib().drt_bvh_stats(C.byref(bundle.scene), *[C.byref(x) for x in v]), "drt_bvh_stats")
    return tuple(x.value for x in v)


def selftest_unit(func, records, device=0):
    """One of the path's device functions over `records` ([n][k] doubles; u64 arguments as their bit patterns). Returns [n][m]."""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    if rec.ndim == 1:
        rec = rec.reshape(-1, 1)
    n, k = rec.shape
    m = _UNIT_OUT[func]
    out = np.zeros((n, m), dtype=np.float64)
    _check(hip_lib().drt_selftest_unit(device, func, _ptr(rec, C.c_double), k, _ptr(out, C.c_double), m, n), "drt_selftest_unit")
    return out


DIVISION_SHARED, DIVISION_DRAW = 0, 1
_DIVISION_OUT = {DIVISION_SHARED: 8, DIVISION_DRAW: 3}


def selftest_division(func, records, device=0):
    """A form that replaces a `/` of the path loop beside that `/`, over `records` ([n][k] doubles, layouts in include/drt_hip.h).
    Record i runs on thread i: 64 consecutive records share a wave. Returns [n][m]."""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    if rec.ndim == 1:
        rec = rec.reshape(-1, 1)
    n, k = rec.shape
    m = _DIVISION_OUT[func]
    out = np.zeros((n, m), dtype=np.float64)
    _check(hip_lib().drt_selftest_division(device, func, _ptr(rec, C.c_double), k, _ptr(out, C.c_double), m, n), "drt_selftest_division")
    return out


BUILD_LEVEL_COUNTS = 33  # BUILD_LEVELS + 1 (csrc/drt_build_kernels.h)


def selftest_build_sort(keys, keys_out=None, pos_out=None, device=0):
    """The radix sort of a device hierarchy build over `keys` (uint64, below 2^63), through the build's own enqueue code. Returns
    (keys_out, pos_out): the key and the position that end in every slot. The two may be given, as contiguous views of the caller's
    (a test puts guard words around them)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    m = keys.size
    keys_out = np.zeros(m, dtype=np.uint64) if keys_out is None else keys_out
    pos_out = np.zeros(m, dtype=np.uint32) if pos_out is None else pos_out
    for a, t in ((keys_out, np.uint64), (pos_out, np.uint32)):
        if a.dtype != t or a.shape != (m,) or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
            raise ValueError("selftest_build_sort: an output array is not a contiguous %s[%d]" % (np.dtype(t).name, m))
    _check(hip_lib().drt_selftest_build_sort(device, _ptr(keys, C.c_uint64), m, _ptr(keys_out, C.c_uint64), _ptr(pos_out, C.c_uint32)),
           "drt_selftest_build_sort")
    return keys_out, pos_out


def selftest_build_topology(sorted_keys, device=0):
    """The topology passes of a device hierarchy build over ascending keys, through the build's own enqueue code. Returns (child
    [m - 1][2] int32, count [m - 1][2] int32, the 33 level counts uint32, the level table [m - 2][2] uint32: (inner node, parent * 2 +
    child slot), the deepest level first)."""
    keys = np.ascontiguousarray(sorted_keys, dtype=np.uint64)
    m = keys.size
    child, count = np.zeros((max(m - 1, 1), 2), dtype=np.int32), np.zeros((max(m - 1, 1), 2), dtype=np.int32)
    level_count = np.zeros(BUILD_LEVEL_COUNTS, dtype=np.uint32)
    levels = np.zeros((max(m - 2, 0), 2), dtype=np.uint32)
    _check(hip_lib().drt_selftest_build_topology(device, _ptr(keys, C.c_uint64), m, _ptr(child, C.c_int32), _ptr(count, C.c_int32),
                                                 _ptr(level_count, C.c_uint32), _ptr(levels, C.c_uint32) if m > 2 else None),
           "drt_selftest_build_topology")
    return child, count, level_count, levels


def selftest_live_resources():
    """What the process holds through the library right now: (device allocations, pinned allocations, events, streams)."""
    out = (C.c_uint64 * 4)()
    _check(hip_lib().drt_selftest_live_resources(out), "drt_selftest_live_resources")
    return tuple(int(v) for v in out)


# ------------------------------------------------------------------------------------------------
# Synthetic scenes

def _xorshift64_stream(seed):
    x = seed & 0xFFFFFFFFFFFFFFFF
    while True:
        x ^= (x << 13) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 7
        x ^= (x << 17) & 0xFFFFFFFFFFFFFFFF
        yield (x >> 33) / 2147483647.0


def synthetic_sphere_scene(n_spheres, width, height, seed=0x5EED, spectra_dir=None):
    """The many-sphere scene of BASELINE config 5: n spheres, centres uniform in [-20,20]x[-20,20]x[-40,0], radii
    uniform [0.05,0.35] from xorshift64 (draw order cx,cy,cz,r), materials round-robin over {blue, green, red, white,
    teal plastic, mirror, rough gold}, one 10x10 plane light at y=25 (emission constant 1), vacuum base + escape;
    pinhole camera (0,0,30) -> (0,0,-20), fov 60. Materials/SPDs come from cornell_plane_light.scn via the host loader."""
    base = load_scene(os.path.join(REPO, "scenes", "cornell_plane_light.scn"), width, height, spectra_dir=spectra_dir)
    names = base.material_names()
    mats = []
    for i in range(int(base.scene.num_materials)):
        m = base.scene.materials[i]
        mats.append({k: getattr(m, k) for k in ("is_black_body", "is_emissive", "shininess", "roughness", "emission_spd",
                                                 "diffuse_spd", "glossy_spd", "mirror_spd", "refract_spd", "extinct_spd",
                                                 "dir_func")} | {"bdsfs": [m.bdsfs[j] for j in range(m.num_bdsfs)]})
    cycle = [names.index(n) for n in ("blue_plastic", "green_plastic", "red_plastic", "white_plastic", "teal_plastic",
                                      "mirror", "gold")]
    g = _xorshift64_stream(seed)
    surfaces = []
    for i in range(n_spheres):
        cx = -20.0 + 40.0 * next(g)
        cy = -20.0 + 40.0 * next(g)
        cz = -40.0 + 40.0 * next(g)
        r = 0.05 + 0.30 * next(g)
        surfaces.append({"type": GEO_SPHERE, "material": cycle[i % len(cycle)], "position": (cx, cy, cz), "radius": r})
    u, v, n = plane_from_points((-5.0, 25.0, 5.0), (5.0, 25.0, 5.0), (-5.0, 25.0, -5.0))
    surfaces.append({"type": GEO_PLANE, "material": names.index("light"), "position": (-5.0, 25.0, 5.0), "u": u, "v": v, "normal": n})
    cam = init_camera((0.0, 0.0, 30.0), (0.0, 0.0, -20.0), 0.0, 60.0, 6.0, 0.3, 0.0, width, height)
    return build_scene(surfaces, mats, base.spds(), int(base.scene.base_material), int(base.scene.escape_material), cam)
