"""Depth-cut films (drt_bind_depth_cuts): the shared cases and the oracle call.

The rule needs no oracle code of its own: cut d of one render equals, bit for bit, the existing oracle's render of the same case with
max_depth = d. oracle_at() is that render -- cases.oracle_render_device_pow on a copy of the params -- made once per (case, depth)
and shared; nothing writes to what it returns. oracle_at_cpu() is the same render without the device's power table, for the tests
that run without a GPU (the power never steers a path, and two films that differ with glibc's power differ with the device's)."""
import cases
import oracle_py as O
import pydrt

# case -> cut depths (ascending, each <= the case's max_depth). Neighbouring cuts of every list have different oracle films
# (tests/test_depth_cuts_cpu.py checks it): many_lights and spheres_1500 are constant from depth 3, first_scene from depth 1.
CUTS = {
    "plane_light_16": (1, 2, 3, 7, 8),  # glass, mirror, gold, plastic; S = 69 with its tail
    "gold_mirror": (1, 2, 3, 7),  # conductor lists
    "many_lights": (1, 2, 3),  # 12 lights: records wider than 64 words, and the multi-light product
    "lights": (1, 2, 3),  # point and sphere lights
    "lens": (1, 2, 4),  # thin lens
    "deep_paths": (1, 4, 12, 13, 16, 17, 21, 40),  # eight cuts; vertices behind the header's third block and in the table block
    "grid_10nm": (1, 3, 6),  # S = 35
    "grid_4nm": (1, 3, 6),  # S = 86
    "grid_2p5nm": (1, 3, 6),  # S = 137
    "spheres_1500": (1, 2, 3),  # hierarchy pipeline
}
# nothing beyond the first hit, and an all-NaN film: the cuts are all the same film, NaN for NaN
FLAT_CUTS = {
    "first_scene": (1, 4),
    "example_scene": (1, 4),
}
ALL_CUTS = dict(CUTS, **FLAT_CUTS)


def params_at(params, depth, **changes):
    """a copy of the params with max_depth = depth (and any other field changed)"""
    p = pydrt.Params.from_buffer_copy(params)
    p.max_depth = depth
    for k, v in changes.items():
        setattr(p, k, v)
    return p


_bundles, _device, _cpu = {}, {}, {}


def load(name):
    if name not in _bundles:
        _bundles[name] = cases.load_case(name)
    return _bundles[name]


def oracle_at(name, depth, **changes):
    """(pixels, means, variances, hits, stats) of the oracle's render of `name` at max_depth = depth, device power"""
    key = (name, depth, tuple(sorted(changes.items())))
    if key not in _device:
        bundle, params = load(name)
        _device[key] = cases.oracle_render_device_pow(bundle, params_at(params, depth, **changes), want_hits=True, num_threads=16)
    return _device[key]


def oracle_at_cpu(name, depth):
    """the same render with glibc's power: no GPU needed"""
    key = (name, depth)
    if key not in _cpu:
        bundle, params = load(name)
        _cpu[key] = O.oracle_render_tile(bundle, params_at(params, depth), want_hits=True, num_threads=16, math_mode=O.MATH_DEVICE)
    return _cpu[key]


def assert_film(got, want, what):
    for g, w, buf in zip(got, want, ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "%s, %s: %s" % (what, buf, cases.first_difference(g, w))
