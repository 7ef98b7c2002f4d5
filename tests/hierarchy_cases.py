"""Device hierarchy builds (drt_rebuild_hierarchy): the inputs of tests/test_hierarchy_cpu.py and
tests/test_gpu_hierarchy.py that tests/scene_update_cases.py does not have -- the two scenes made to take the rule's other paths."""
import numpy as np

import pydrt
import scene_update_cases as U

DEEP_EXTENT = 16.0


def coincident_spheres(n=300):
    """n spheres with one centre and different radii: every key is equal, every split is the median's. The centre is the origin, where
    a box is symmetric and its centre exact whatever the radius."""
    return [("sphere", (0.0, 0.0, 0.0), 0.5 + 0.01 * k) for k in range(n)]


def deep_spheres():
    """64 spheres whose tree is 63 inner levels deep without the rule's depth budget: coordinates that halve along the three axes in
    turn, so every key but one has a highest set bit of its own and every split by that bit peels one sphere off. Per axis: one
    sphere at the extent (quantised to 2^21 - 1) and twenty at 1.5 * extent / 2^(k + 1), k = 1 .. 20 (quantised to 2^(20 - k) +
    2^(19 - k) for k < 20 and to 1 for k = 20: the factor 1.5 keeps the highest bit clear of the rounding of a box's centre); the last
    sphere sits at the origin (key 0)."""
    s = []
    for k in range(21):
        for axis in range(3):
            p = [0.0, 0.0, 0.0]
            p[axis] = DEEP_EXTENT if k == 0 else 1.5 * DEEP_EXTENT / 2.0 ** (k + 1)
            s.append(("sphere", tuple(p), 1.0))
    return s + [("sphere", (0.0, 0.0, 0.0), 1.0)]


_own = {}


def load(name):
    """a case of scene_update_cases, or one of the two scenes above as a case whose "before" and "after" are one scene (the point
    light is never intersected: the tree holds the spheres alone). Both are forced behind the tree."""
    if name not in ("coincident_300", "deep_64"):
        return U.load(name)
    if name not in _own:
        spheres = coincident_spheres() if name == "coincident_300" else deep_spheres()
        b = U.small_scene(spheres + [("point_light", (5.0, 10.0, 10.0))])
        _own[name] = U._case(b, b, pydrt.make_params(16, 16, spp=2, max_depth=3, seed=33), forced=True)
    return _own[name]


def sphere_rows(spheres):
    """raw surface rows of ("sphere", position, radius) tuples, for the rule alone (the material word stays 0)"""
    rows = np.zeros((len(spheres), pydrt.SURFACE_ROW))
    head = np.zeros(len(spheres), dtype=[("type", "<u4"), ("material", "<u4")])
    head["type"] = pydrt.GEO_SPHERE
    rows[:, 0] = head.view("<f8")
    for i, s in enumerate(spheres):
        rows[i, U.ROW_POS], rows[i, U.ROW_RADIUS] = s[1], s[2]
    return rows
