"""The key sets of tests/test_gpu_build_passes.py (drt_selftest_build_sort, drt_selftest_build_topology): made for
the places where a multi-tile radix sort and a level-by-level topology pass go wrong, not drawn from scenes. Not a test file:
tests/test_hierarchy_cpu.py checks with the rule alone that the topology sets give valid trees, tests/test_gpu_build_passes.py runs all
of them on the device. Everything here is seeded and a pure function of its arguments. Every key is below 2^63.

The sort's families (SORT_FAMILIES), each at every size of SORT_SIZES:
  random                 seeded random 63-bit keys
  byte_0 .. byte_7       only byte k varies (a seeded draw of all its values), the other bytes constant and non-zero: the pass of that byte
                         alone decides the order, so a pass with a wrong shift reorders these
  distinct_2, _4, _256   keys drawn from that many values: stability decides most of the order
  one_value, unbounded   all keys equal; all BUILD_KEY_UNBOUNDED
  ascending, descending  already sorted (with the duplicates a sorted draw has); strictly descending, every byte moving
  runs                   runs of 1500 equal keys, the runs in descending order: every full run straddles a tile boundary (1500 > 1024)
                         and moves as a whole
  unbounded_tail         a random prefix, then BUILD_KEY_UNBOUNDED to the end, the tail's length no multiple of 64
SORT_SIZES are the tile (1024) and the block (256) and a wave (64) with both neighbours, two and three tiles exactly, a last tile of one
element (1025, 2049, 3073, 4097), and 5000 and 20481 = 20 tiles + 1: a digit table of 5 and of 21 columns."""
import numpy as np

UNBOUNDED = np.uint64(2 ** 63 - 1)
SORT_SIZES = [2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073, 4097, 5000, 20481]
SORT_FAMILIES = (["random"] + ["byte_%d" % k for k in range(8)] + ["distinct_2", "distinct_4", "distinct_256", "one_value", "unbounded",
                 "ascending", "descending", "runs", "unbounded_tail"])
TOPOLOGY_FAMILIES = ["random", "distinct_2", "distinct_4", "distinct_256", "one_value", "unbounded", "unbounded_tail"]
TOPOLOGY_SIZES = [2, 3, 4, 5, 257, 1025, 5000, 20481]
RUN = 1500
_OTHER_BYTES = 0x1122334455667788  # every byte non-zero, the top one below 0x80
_STRIDE = 0x00003FFFF1F1F1F3      # 20481 of them stay below 2^62


def _rng(family, m):
    return np.random.default_rng([SORT_FAMILIES.index(family), m, 0x5EED])


def _random(rng, m):
    return rng.integers(0, 2 ** 63, m, dtype=np.uint64)


def sort_keys(family, m):
    """the keys of a family at size m, in the order the sort is handed them"""
    rng = _rng(family, m)
    if family == "random":
        return _random(rng, m)
    if family.startswith("byte_"):
        k = int(family[5:])
        values = rng.integers(0, 128 if k == 7 else 256, m, dtype=np.uint64)  # (byte 7 holds bit 63)
        return (np.uint64(_OTHER_BYTES) & ~np.uint64(0xFF << (8 * k))) | (values << np.uint64(8 * k))
    if family.startswith("distinct_"):
        values = np.unique(_random(rng, 4 * int(family[9:])))[: int(family[9:])]
        return rng.permutation(values)[rng.integers(0, len(values), m)]
    if family == "one_value":
        return np.full(m, 0x0123456789ABCDEF, dtype=np.uint64)
    if family == "unbounded":
        return np.full(m, UNBOUNDED, dtype=np.uint64)
    if family == "ascending":
        return np.sort(_random(rng, m))
    if family == "descending":
        return np.uint64(2 ** 62) + np.uint64(_STRIDE) * np.arange(m, 0, -1, dtype=np.uint64)
    if family == "runs":
        values = np.sort(np.unique(_random(rng, 4 * (m // RUN + 1)))[: m // RUN + 1])[::-1]
        return values[np.arange(m) // RUN]
    if family == "unbounded_tail":
        tail = max(m // 3, 1)
        tail += 1 if tail % 64 == 0 else 0
        key = _random(rng, m)
        key[m - tail:] = UNBOUNDED
        return key
    raise KeyError(family)


def comb():
    """deep_64's key pattern (tests/hierarchy_cases.py), from keys: 63 distinct keys with one bit each, bit k of key k, so that every
    split by the highest differing bit peels one key's duplicates off; key 2^k comes 1 + k % 3 times, and key 0 three times. 129 keys,
    sorted."""
    key = [0, 0, 0]
    for k in range(63):
        key += [1 << k] * (1 + k % 3)
    return np.array(key, dtype=np.uint64)


BLOB_BITS, BLOB_PEELED = 12, 18


def deep_blob(peeled=BLOB_PEELED):
    """2^12 keys that differ in their low 12 bits only (0 .. 4095) below `peeled` keys with one high bit each (2^62, 2^61, ...), sorted:
    a split by the highest differing bit peels the last key off, so the top levels hold one inner node each and the blob lies below
    them, its large levels at the bottom of the level table. tests/test_hierarchy_cpu.py states where the depth budget takes over (at
    depth 17, for 18 and for 19 peeled keys) and what every level holds."""
    blob = np.arange(1 << BLOB_BITS, dtype=np.uint64)
    return np.concatenate([blob, np.sort(np.uint64(1) << np.arange(62, 62 - peeled, -1).astype(np.uint64))])


def topology_sets():
    """[(name, sorted keys)]: what the topology passes are run on"""
    sets = [("%s-%d" % (f, m), np.sort(sort_keys(f, m))) for f in TOPOLOGY_FAMILIES for m in TOPOLOGY_SIZES]
    return sets + [("comb", comb()), ("deep_blob", deep_blob()), ("deep_blob_19", deep_blob(19))]


TOPOLOGY_NAMES = ["%s-%d" % (f, m) for f in TOPOLOGY_FAMILIES for m in TOPOLOGY_SIZES] + ["comb", "deep_blob", "deep_blob_19"]
_topology = {}


def topology_keys(name):
    if not _topology:
        _topology.update(topology_sets())
    return _topology[name]
