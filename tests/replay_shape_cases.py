"""The replay passes (drt_depth_cut_kernel, drt_sensor_kernel; DESIGN.md, sections 5j and 5l) at the shapes tests/cases.py never
reaches: the shapes, scene texts, cut lists and the expected-film helpers of tests/test_gpu_replay_shapes.py and
tests/test_replay_shapes_cpu.py.

Nothing here restates a rule. Cut d of a render is cases.oracle_render_device_pow at max_depth = d (depth_cut_cases); the sensor film is
sensor_rule.sensor_film over the oracle's one-sample renders (sensor_cases); the curves are sensor_cases.seeded_curves. The helpers take
a bundle and a key that names it, so that an edited bundle has an oracle too; every render is made once and shared, and nothing writes
to what they return. With cpu=True the oracle keeps glibc's power: no GPU needed, and two films that differ there differ with the
device's power too (the power never steers a path).

Shape by shape, what the shared cases leave out (every one of those is at most 32 x 32 pixels and 4 samples, S <= 137):
  A  samples in more than one window of 64 headers, alone and with first_sample != 0;
  B  row blocks: films offset by the block's first pixel, header slots by the block's stride;
  C  more pixels than the device holds waves: a wave takes a second work item;
  D  a table too large for LDS, and a table that fits where table and curves together do not;
  E  S = 256 and S = 193: four wavelength sets, the last full or with one active lane;
  F  1, 6 and 7 cuts (deep_paths of tests/cases.py; its eight-entry list's prefixes);
  G  live edits (plane_light_16 and the edits of scene_update_cases / material_update_cases).
"""
import numpy as np

import cases
import depth_cut_cases as DC
import material_update_cases as MU
import oracle_py as O
import pydrt
import sensor_cases as SC
import sensor_rule

PLAIN = "cornell_plane_light.scn"
LDS_BYTES = 64 * 1024  # what a block may ask for: the launcher's `<= 64 * 1024` (create_impl) and `<= 65536` (sensor_alloc)


def many_materials_scene(n_materials, n_spheres):
    """cornell_plane_light.scn plus n_materials plastics of their own colours (two spectral rows each) on n_spheres small spheres"""
    text = open(cases.scene_path(PLAIN)).read()
    for k in range(n_materials):
        text += "\nMaterial\nname m%d\ndiffuse rgb %.3f, %.3f, %.3f\nglossy rgb %.3f, 0.1, 0.1\nshininess %d.0\nbdsfs bp_diffuse_bdsf, bp_glossy_bdsf\ndir_func cos_weighted_sample_hemisphere\n" % (
            k, 0.1 + 0.8 * ((k * 7) % 11) / 11.0, 0.1 + 0.8 * ((k * 3) % 13) / 13.0, 0.1 + 0.8 * (k % 17) / 17.0, 0.05 + 0.3 * (k % 5) / 5.0, 10 + k % 90)
    for k in range(n_spheres):
        text += "\nSurface\nname s%d\ntype sphere\nposition %.3f, %.3f, %.3f\nradius 0.12\nmaterial m%d\n" % (
            k, -2.5 + 5.0 * (k % 10) / 9.0, -2.6 + 0.35 * (k // 10), -2.0 + 0.37 * (k % 7), k % n_materials)
    return text


# name -> the shape. scene: a file of scenes/, or (materials, spheres) for many_materials_scene. rows: bundle.scene.num_spds.
# Random pixel scheme everywhere; batch_spp 0 unless given.
SHAPES = {
    # A: one pair takes 64, 65 or 130 samples of each of 64 pixels (the tests change spp)
    "windows": dict(size=(8, 8), spp=130, depth=6, seed=21, cuts=(1, 3, 6), S=69, rows=28),
    # B: four row blocks of 16 rows; (i) pairs of 4 samples, (ii) pairs of 70: blocks and the second header window meet
    "blocks_4x64": dict(size=(64, 64), tile=dict(x0=30, tile_w=4, tile_h=64), spp=8, batch_spp=2, depth=6, seed=22, cuts=(1, 3, 6), S=69, rows=28),
    "blocks_2x64": dict(size=(64, 64), tile=dict(x0=31, tile_w=2, tile_h=64), spp=140, batch_spp=31, depth=4, seed=23, cuts=(1, 2, 4), S=69, rows=28),
    # C: 9216 pixels, more than the 8192 waves of an MI355X
    "items": dict(size=(96, 96), grid=(380.0, 720.0, 10.0), spp=2, depth=3, seed=24, cuts=(1, 2, 3), S=35, rows=28),
    # D: see table_bytes / sensor_bytes below for what each makes of the 64 KiB
    "rows_328": dict(size=(16, 16), scene=(150, 40), spp=3, depth=6, seed=4, cuts=(1, 2, 3, 6), S=69, rows=328),
    "rows_54_2p5nm": dict(size=(16, 16), scene=(13, 13), grid=(380.0, 720.0, 2.5), spp=3, depth=6, seed=4, cuts=(1, 2, 3, 6), S=137, rows=54),
    "rows_38_2p5nm": dict(size=(16, 16), scene=(5, 5), grid=(380.0, 720.0, 2.5), spp=3, depth=6, seed=4, cuts=(1, 2, 3, 6), S=137, rows=38),
    "lds_s256": dict(size=(16, 16), grid=(380.0, 635.0, 1.0), spp=3, depth=6, seed=4, cuts=(1, 2, 3, 6), S=256, rows=28),
    "lds_s193": dict(size=(16, 16), grid=(440.0, 632.0, 1.0), spp=3, depth=6, seed=4, cuts=(1, 2, 3, 6), S=193, rows=28),
    # E: four sets; 193 = 3 * 64 + 1 (the 1 nm grid must bracket 630 nm, where the glass is sampled)
    "sets_s256": dict(size=(12, 12), grid=(380.0, 635.0, 1.0), spp=3, depth=6, seed=25, cuts=(1, 3, 6), S=256, rows=28),
    "sets_s193": dict(size=(12, 12), grid=(440.0, 632.0, 1.0), spp=3, depth=6, seed=25, cuts=(1, 3, 6), S=193, rows=28),
}
CHANNELS = 3  # sensor channels where a shape does not say

# D, sensor side: (shape, curves) -> (the table fits LDS, the table and the curves fit LDS). The passes differ only in the middle
# case -- (True, False): the shade kernel reads LDS, the sensor kernel memory -- and its neighbour (True, True) is the control.
# The scene's own 54 rows at S = 137 (59 184 bytes) and 28 rows at S = 256 (57 344) would fit; the table the launcher measures has the
# derived rows too (device_spd_rows: 77 and 38 rows), so rows_54_2p5nm and lds_s256 are out of LDS whatever the curves, as rows_328
# is. rows_38_2p5nm (53 device rows) and lds_s193 (38) are the shapes in which the sensor falls back alone.
SENSOR_LDS = {
    ("rows_328", 3): (False, False),
    ("rows_54_2p5nm", 8): (False, False), ("rows_54_2p5nm", 1): (False, False),
    ("rows_38_2p5nm", 8): (True, False), ("rows_38_2p5nm", 1): (True, True),
    ("lds_s256", 8): (False, False), ("lds_s256", 3): (False, False),
    ("lds_s193", 8): (True, False), ("lds_s193", 3): (True, True),
}
TABLE_SHAPES = ("rows_328", "rows_54_2p5nm", "rows_38_2p5nm", "lds_s256", "lds_s193")


def sensor_channels(name):
    """the curve counts a shape is rendered with"""
    return tuple(n for (shape, n) in SENSOR_LDS if shape == name) or (CHANNELS,)

# F: deep_paths (16 x 16, depth 40) with 1, 6 and 7 cuts: the single cut below max_depth, the others prefixes of the eight-entry list
DEEP = "deep_paths"
DEEP_CUT_LISTS = ((12,), DC.CUTS[DEEP][:6], DC.CUTS[DEEP][:7])

# G: plane_light_16, its cut list, and the edits: name -> (cases module, case name, context behind DRT_FORCE_BVH)
LIVE = "plane_light_16"
LIVE_CUTS = DC.CUTS[LIVE]
EDITS = {
    "set_camera": ("scene", "cam_plane_light_16", False),
    "update_surfaces": ("scene", "plane_light_16", False),
    "update_surfaces_rebuild": ("scene", "plane_light_16", True),
    "update_spectra": ("material", "glass_refract", False),
    "rebuild_hierarchy": (None, None, True),
}

# B: kernel pairs of one drt_render call, in row blocks and (DRT_NO_ROW_BLOCKS) without -- row_block_count, row_block_rows,
# row_block_fit and equal_split of csrc/drt_pair_rule.h; tests/test_replay_shapes_cpu.py takes them from the header itself
BLOCK_PLANS = {
    "blocks_4x64": dict(blocks=4, rows=16, fit=5, pairs=(4, 4), plain_pairs=(2, 2, 2, 2)),
    "blocks_2x64": dict(blocks=4, rows=16, fit=77, pairs=(70, 70), plain_pairs=(28, 28, 28, 28, 28)),
}

_bundles, _films, _contributions = {}, {}, {}


def load(name):
    """(bundle, params) of a shape"""
    if name not in _bundles:
        s = SHAPES[name]
        w, h = s["size"]
        grid = s.get("grid", (380.0, 720.0, 5.0))
        scene = s.get("scene", PLAIN)
        text = many_materials_scene(*scene) if isinstance(scene, tuple) else open(cases.scene_path(scene)).read()
        bundle = pydrt.load_scene_text(text, w, h, min_wl=grid[0], max_wl=grid[1], wl_interval=grid[2])
        params = pydrt.make_params(w, h, spp=s["spp"], max_depth=s["depth"], seed=s["seed"], batch_spp=s.get("batch_spp", 0), **s.get("tile", {}))
        _bundles[name] = (bundle, params)
    return _bundles[name]


def params_with(params, **changes):
    p = pydrt.Params.from_buffer_copy(params)
    for k, v in changes.items():
        setattr(p, k, v)
    return p


def tile_pixels(params):
    return int(params.tile_w) * int(params.tile_h)


# ---- the 64 KiB, in the launcher's terms ----

def device_spd_rows(bundle):
    """Rows of the table the kernels read, which is what the launcher measures against LDS (create_impl, csrc/drt_launcher.hip): the
    scene's own, a diffuse / pi row per distinct diffuse row, two pair rows per material whose list holds dielectric or conductor
    Fresnel functions (and not both), and the all-zero row."""
    mats = [bundle.scene.materials[i] for i in range(int(bundle.scene.num_materials))]
    diffuse = {int(m.diffuse_spd) for m in mats if int(m.diffuse_spd) >= 0}
    pairs = 0
    for m in mats:
        lobes = set(MU.bdsfs_of(m))
        d, c = bool(lobes & {MU.FS_REFLECT, MU.FS_TRANSMIT}), bool(lobes & {MU.FS_CONDUCTOR, MU.CT_CONDUCTOR})
        pairs += 2 * int(d != c)
    return int(bundle.scene.num_spds) + len(diffuse) + pairs + 1


def scene_table_bytes(bundle):
    """the scene's own rows: what the arithmetic of a shape's description is about"""
    return int(bundle.scene.num_spds) * bundle.S * 8


def table_bytes(bundle):
    """the table a kernel stages: `<= LDS_BYTES` is the launcher's spds_in_lds"""
    return device_spd_rows(bundle) * bundle.S * 8


def sensor_bytes(bundle, n_curves):
    """the table and n curves behind it: `<= LDS_BYTES` (and the table's own fit) keeps the sensor kernel's table in LDS"""
    return (device_spd_rows(bundle) + n_curves) * bundle.S * 8


# ---- expected films ----

def _oracle_params(params, **changes):
    """what the oracle's film depends on: batch_spp and the flags shape launches only"""
    return params_with(params, **dict(changes, batch_spp=0, flags=0))


def _render(bundle, p, cpu):
    if cpu:
        return O.oracle_render_tile(bundle, p, num_threads=16, math_mode=O.MATH_DEVICE)
    return cases.oracle_render_device_pow(bundle, p, num_threads=16)


def oracle_film(key, bundle, params, cpu=False, **changes):
    """(pixels, means, variances) of the oracle's render of `bundle` (which `key` names) with `params`"""
    p = _oracle_params(params, **changes)
    k = (key, bytes(p), cpu)
    if k not in _films:
        _films[k] = _render(bundle, p, cpu)[:3]
    return _films[k]


def oracle_at(key, bundle, params, depth, cpu=False, **changes):
    """depth_cut_cases.oracle_at for a bundle: the render at max_depth = depth, what cut `depth` must equal"""
    return oracle_film(key, bundle, params, cpu=cpu, max_depth=depth, **changes)


def contributions(key, bundle, params, cpu=False, **changes):
    """[spp][P][S], as sensor_cases.samples_device: sample m's contribution is the oracle's render with spp = 1, first_sample = m.
    Kept per sample, so that 64, 65 and 130 samples of one shape share their renders."""
    p = _oracle_params(params, **changes)
    out = []
    for m in range(int(p.first_sample), int(p.first_sample) + int(p.spp)):
        q = params_with(p, spp=1, first_sample=m)
        k = (key, bytes(q), cpu)
        if k not in _contributions:
            _contributions[k] = _render(bundle, q, cpu)[0][:, :-1].copy()
        out.append(_contributions[k])
    return np.stack(out)


def sensor_film(key, bundle, params, curves, cpu=False, **changes):
    """the rule's sensor film of the render"""
    p = _oracle_params(params, **changes)
    return sensor_rule.sensor_film(curves, contributions(key, bundle, params, cpu=cpu, **changes), first_sample=int(p.first_sample))


def curves_for(bundle, n=CHANNELS):
    return SC.seeded_curves(n, bundle.S)


def assert_film(got, want, what):
    for g, w, buf in zip(got, want, ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "%s, %s: %s" % (what, buf, cases.first_difference(g, w))


def differing_pixels(a, b):
    """[P] bool: the pixels in which two films' sums differ"""
    return (a[0] != b[0]).any(axis=1)


# ---- G: the edited bundles ----

def edit_case(name):
    """(before, after) bundles of a live edit; after is None where the edit changes no result (rebuild_hierarchy)"""
    module, case, _ = EDITS[name]
    if module is None:
        return cases.load_case(LIVE)[0], None
    import scene_update_cases as U
    c = (U if module == "scene" else MU).load(case)
    return c["before"], c["after"]


def live_params():
    return cases.load_case(LIVE)[1]
