"""GPU (-m gpu): the sort and the topology passes of a device hierarchy build (csrc/drt_build_kernels.h) on keys
made for them (tests/build_pass_cases.py), through drt_selftest_build_sort and drt_selftest_build_topology -- which run the enqueue
helpers drt_rebuild_hierarchy runs (tests/test_hierarchy_cpu.py checks that both name them). Every comparison is exact. The sort is held
to np.argsort(kind="stable"): the sorted keys and the position that ends in every slot, at 2 to 20481 keys, one to 21 tiles of 1024. The
topology is held to tests/hierarchy_rule.py: child and count byte for byte, the level counts, and the level table level by level as
sets (the order within a level is the order of the kernel's atomics and is free)."""
import numpy as np
import pytest

import build_pass_cases as B
import hierarchy_rule as R
import pydrt

pytestmark = pytest.mark.gpu

GUARD = 64
KEY_GUARD, POS_GUARD = np.uint64(0xC3C3C3C3C3C3C3C3), np.uint32(0x3C3C3C3C)


@pytest.mark.parametrize("m", B.SORT_SIZES)
@pytest.mark.parametrize("family", B.SORT_FAMILIES)
def test_the_sort_is_numpys_stable_argsort(family, m):
    key = B.sort_keys(family, m)
    assert key.dtype == np.uint64 and key.shape == (m,) and (key <= B.UNBOUNDED).all()
    order = np.argsort(key, kind="stable")
    keys_room, pos_room = np.full(m + 2 * GUARD, KEY_GUARD), np.full(m + 2 * GUARD, POS_GUARD)
    keys_out, pos_out = pydrt.selftest_build_sort(key, keys_room[GUARD:GUARD + m], pos_room[GUARD:GUARD + m])
    assert np.array_equal(pos_out, order), "%s, %d keys: first wrong slot %d" % (family, m, int(np.flatnonzero(pos_out != order)[0]))
    assert np.array_equal(keys_out, key[order])
    for room, guard in ((keys_room, KEY_GUARD), (pos_room, POS_GUARD)):
        assert (room[:GUARD] == guard).all() and (room[GUARD + m:] == guard).all(), "%s, %d keys: a guard word changed" % (family, m)
    if family.startswith("byte_"):  # what the family is for: only that byte differs, and it does
        diff = np.bitwise_or.reduce(key ^ key[0])
        assert diff & ~np.uint64(0xFF << (8 * int(family[5:]))) == 0 and (diff != 0 or m < 4)


def test_the_sort_families_are_what_they_say():
    """the premises a family's name promises, at the largest size (no device call)"""
    m = B.SORT_SIZES[-1]
    assert m == 20 * 1024 + 1
    for n in (2, 4, 256):
        assert len(np.unique(B.sort_keys("distinct_%d" % n, m))) == n
    assert (np.diff(B.sort_keys("ascending", m).astype(np.float64)) >= 0).all()
    d = B.sort_keys("descending", m)
    assert (d[:-1] > d[1:]).all() and all(len(np.unique((d >> np.uint64(8 * k)) & np.uint64(255))) > 1 for k in range(8))
    runs = B.sort_keys("runs", m)
    starts = np.flatnonzero(np.diff(runs.astype(np.float64)) != 0) + 1
    assert starts.tolist() == list(range(B.RUN, m, B.RUN)) and (runs[starts - 1] > runs[starts]).all()
    tail = B.sort_keys("unbounded_tail", m)
    n_tail = int((tail == B.UNBOUNDED).sum())
    assert n_tail % 64 != 0 and (tail[m - n_tail:] == B.UNBOUNDED).all() and n_tail > 1024


def test_the_selftests_refuse_what_they_cannot_run():
    key = np.array([3, 2, 1], dtype=np.uint64)
    with pytest.raises(RuntimeError, match="out of order"):
        pydrt.selftest_build_topology(key)
    with pytest.raises(RuntimeError, match="not in 2"):
        pydrt.selftest_build_topology(key[:1])
    with pytest.raises(RuntimeError, match="bit 63"):
        pydrt.selftest_build_sort(np.array([1, 2 ** 63], dtype=np.uint64))
    with pytest.raises(RuntimeError, match="not in 1"):
        pydrt.selftest_build_sort(key[:0])


@pytest.mark.parametrize("name", B.TOPOLOGY_NAMES)
def test_the_topology_is_the_rules(name):
    key = B.topology_keys(name)
    m = len(key)
    assert (key[:-1] <= key[1:]).all()
    want_child, want_count, depth = R.topology(key)
    levels, _ = R.check_tree(want_child, want_count, m)
    assert levels == depth <= R.BVH_STACK
    entries = R.level_entries(want_child, want_count)
    assert len(entries) == depth and sum(len(e) for e in entries) == m - 2
    child, count, level_count, table = pydrt.selftest_build_topology(key)
    assert child.tobytes() == want_child.tobytes(), name + ": child"
    assert count.tobytes() == want_count.tobytes(), name + ": count"
    want_counts = np.zeros(pydrt.BUILD_LEVEL_COUNTS, dtype=np.uint32)
    want_counts[0] = 1
    want_counts[1:depth] = [len(e) for e in entries[1:]]
    assert np.array_equal(level_count, want_counts), "%s: level counts %s, the tree has %s" % (name, level_count.tolist(), want_counts.tolist())
    # the table: the deepest level first, level 1 last
    assert table.shape == (m - 2, 2)
    at = 0
    for d in range(depth - 1, 0, -1):
        got = sorted(map(tuple, table[at:at + len(entries[d])].tolist()))
        assert got == entries[d], "%s: level %d of the table (%d entries from %d on)" % (name, d, len(entries[d]), at)
        at += len(entries[d])
    assert at == m - 2
    if name == "deep_blob":  # (tests/test_hierarchy_cpu.py says why) a level of 2048 below 18 levels of one node, and the deepest level the rule allows
        assert depth == 30 and level_count[:18].tolist() == [1] * 18 and level_count[28:].tolist() == [2048, 1, 0, 0, 0]
    if name == "deep_blob_19":  # the same with both deepest levels large
        assert depth == 30 and level_count[:18].tolist() == [1] * 18 and level_count[28:].tolist() == [1537, 1015, 0, 0, 0]
