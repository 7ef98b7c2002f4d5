"""CPU: the plan of a kernel pair (csrc/drt_pair_rule.h), run on the host as the launcher runs it.

tests/host/pair_rule_main.cpp reads cases and prints every field of the plan the header makes of them; it is built with the address and
undefined-behaviour sanitizers as a program of its own. The functions below whose names start with `was_` restate, expression by
expression, what the launcher computed inline before the header existed (window_copy, enqueue_pair, enqueue_trace, create_impl's pool
sample, round_pairs, render_pairs and enqueue_blocks): the program must give the same numbers, field for field.

One rule is held to a property instead: the split of a call's samples into pairs of equal size. The inline form took n_pairs =
ceil(num / fit) pairs of ceil(num / n_pairs) samples and the rest in the last one -- 256 samples where 125 fit went out as 86 + 86 + 84,
not the 86 + 85 + 85 its comment promised. equal_split keeps the number of pairs and the largest pair and makes the sizes differ by one
sample at the most."""
import itertools
import os
import re
import subprocess

import pytest

import cases

CSRC = os.path.join(cases.REPO, "daily-ray-trace_amd", "csrc")
INCLUDE = os.path.join(cases.REPO, "include")
FLAG_RECORD_HITS = 1
TRACE_BLOCK, SHADE_WAVES, SHADE_PIXEL_CHUNK = 256, 4, 16  # (any values would do: the rules take them as arguments)
U32 = 0xFFFFFFFF
UNSET = (-1, U32, 0)  # the three overrides of the shade queue

W, H = 96, 200
WINDOWS = {"closed": (0, 10, 70, 30, 150), "part": (1, 10, 70, 30, 150), "no columns": (1, 40, 40, 30, 150), "the tile": (1, 0, W, 0, H),
           "rows 30..50": (1, 10, 70, 30, 50)}
N_PIX = (1, 63, 64, 4096, 96 * 200, 1024 ** 2, 4096 ** 2)
N_SAMPLES = (1, 3, 64, 256)


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pair") / "pair_rule_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + CSRC, "-I" + INCLUDE, os.path.join(cases.REPO, "tests", "host", "pair_rule_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def run(rule_program, lines):
    """the program's answers to `lines`, one list of ints per line ('|' dropped)"""
    text = "".join(" ".join(str(int(v)) if not isinstance(v, str) else v for v in line) + "\n" for line in lines)
    r = subprocess.run([rule_program], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]  # ends clean: no report of the program's or a sanitizer's
    out = [x.split() for x in r.stdout.splitlines()]
    assert len(out) == len(lines) and all(o[0] == line[0] for o, line in zip(out, lines))
    return [[int(v) for v in o[1:] if v != "|"] for o in out]


# ---- spans: (first_sample, n, hits_sample_offset, row0, rows, stride, has_list, list_len), as enqueue_pair's arguments were ----

def whole_span(first, n, hso=0):
    return (first, n, hso, 0, 0, 0, 0, 0)      # enqueue_pair(ctx, first_sample + done, n, done)


def block_span(first, n, row0, rows):
    return (first, n, 0, row0, rows, n, 0, 0)  # enqueue_pair(ctx, first_sample + at, n, 0, r0, rows, n)


def list_span(first, n, length):
    return (first, n, 0, 0, 0, n, 1, length)   # enqueue_pair(ctx, at, ns, 0, 0, 0, ns, list + off, len)


def test_the_named_spans_are_the_callers_arguments(rule_program):
    got = run(rule_program, [("span", "whole", 7, 3, 12), ("span", "block", 7, 5, 34, 17), ("span", "list", 2, 4, 1000),
                             ("narrow",) + block_span(7, 22, 34, 17) + (12, 3), ("narrow",) + whole_span(7, 20, 40) + (6, 2),
                             ("narrow",) + list_span(0, 8, 1000) + (4, 4)])
    assert got[0] == list(whole_span(7, 3, 12)) and got[1] == list(block_span(7, 5, 34, 17)) and got[2] == list(list_span(2, 4, 1000))
    # redo_batches: enqueue_pair(ctx, b.first_sample + done, min(safe, ...), b.hits_sample_offset + done, b.row0, b.rows, 0, b.list, b.list_len)
    assert got[3] == [7 + 12, 3, 12, 34, 17, 0, 0, 0] and got[4] == [7 + 6, 2, 46, 0, 0, 0, 0, 0] and got[5] == [4, 4, 4, 0, 0, 0, 1, 1000]


# ---- geometry ----

def was_window_copy(tile_h, row0, rows, window):
    """(lo, hi, stage0) of window_copy, or None where it returned before launching anything"""
    _, wx0, wx1, wy0, wy1 = window
    if rows == 0:
        row0, rows = 0, tile_h
    lo, hi = max(row0, wy0), min(row0 + rows, wy1)
    if hi <= lo or wx1 <= wx0:
        return None
    return lo, hi, (lo - wy0) * (wx1 - wx0)


def was_enqueue_trace(p, ctx_n_pix, batch_spp, first, n, hso, row0=0, rows=0, stride=0, has_list=0, list_len=0, col0=0, cols=0):
    """the fields of TraceParams and DevRayTable that enqueue_trace worked out of its arguments"""
    whole = rows == 0
    if whole:
        row0, rows = 0, p["tile_h"]
    if cols == 0:
        col0, cols = 0, p["tile_w"]
    n_pix = list_len if has_list else ctx_n_pix if (whole and cols == p["tile_w"]) else rows * cols
    return [p["x0"] + col0, p["y0"] + row0 * p["row_stride"], cols, rows, p["row_stride"], n_pix, stride if stride else batch_spp,
            1 if p["flags"] & FLAG_RECORD_HITS else 0, 0 if (has_list or whole) else row0 * p["tile_w"]]


def was_enqueue_pair(p, batch_spp, span, window):
    """(geometry, tile): what enqueue_pair worked out between its HIP calls, and the arguments it gave enqueue_trace"""
    first, n, hso, row0, rows, stride, has_list, list_len = span
    win_open, wx0, wx1, wy0, wy1 = window
    ctx_n_pix = p["tile_w"] * p["tile_h"]
    windowed = bool(win_open and not has_list)
    t_row0, t_rows = (row0 if rows else 0), (rows if rows else p["tile_h"])
    l_row0, l_rows, l_cols = t_row0, t_rows, p["tile_w"]
    if windowed:
        lo, hi = max(t_row0, wy0), min(t_row0 + t_rows, wy1)
        l_row0, l_rows, l_cols = lo, (hi - lo if hi > lo else 0), wx1 - wx0
    nothing = windowed and (l_rows == 0 or l_cols == 0)
    tile = None
    if windowed:
        if not nothing:
            tile = was_enqueue_trace(p, ctx_n_pix, batch_spp, first, n, hso, l_row0, l_rows, stride, 0, 0, wx0, l_cols)
    else:
        tile = was_enqueue_trace(p, ctx_n_pix, batch_spp, first, n, hso, row0, rows, stride, has_list, list_len)
    n_pix = list_len if has_list else l_rows * l_cols if windowed else rows * p["tile_w"] if rows else ctx_n_pix
    pix0 = row0 * p["tile_w"] if (rows and not has_list) else 0
    stage0 = (l_row0 - min(l_row0, wy0)) * l_cols if windowed else 0
    counted = (t_rows * p["tile_w"] if windowed else n_pix) * n
    return dict(windowed=windowed, nothing=nothing, t_row0=t_row0, t_rows=t_rows, l_row0=l_row0, l_rows=l_rows, l_cols=l_cols, n_pix=n_pix,
                pix0=pix0, stage0=stage0, counted=counted), tile


def params_of(x0=0, y0=0, row_stride=1, flags=0):
    return dict(x0=x0, y0=y0, tile_w=W, tile_h=H, row_stride=row_stride, flags=flags)


def pair_line(p, batch_spp, span, window):
    return ("pair", p["x0"], p["y0"], p["tile_w"], p["tile_h"], p["row_stride"], p["flags"], batch_spp) + tuple(span) + tuple(window)


def check_pair(got, p, batch_spp, span, window, what):
    g, tile = was_enqueue_pair(p, batch_spp, span, window)
    windowed, nothing, t_row0, t_rows, l_row0, l_rows, col0, l_cols, n_pix, pix0, stage0, counted = got[:12]
    assert (windowed, nothing, t_row0, t_rows) == (g["windowed"], g["nothing"], g["t_row0"], g["t_rows"]), what
    assert (n_pix, pix0, counted) == (g["n_pix"], g["pix0"], g["counted"]), what
    if not nothing:  # (no kernels otherwise: the launch's rows and film position are nobody's)
        assert (l_row0, l_rows, l_cols, stage0) == (g["l_row0"], g["l_rows"], g["l_cols"], g["stage0"]), what
        assert col0 == (window[1] if windowed else 0), what
        assert got[16:] == tile, what
    else:
        assert tile is None and got[16:] == [-1] * 9 and n_pix == 0, what
    # the one invariant three places used to keep each for itself: the rows window_copy moves are the rows the pair renders
    if windowed:
        copy = was_window_copy(p["tile_h"], span[3], span[4], window)
        assert (copy is None) == bool(nothing) and bool(got[15]) == bool(nothing), what
        if copy is not None:
            assert tuple(got[12:15]) == copy == (l_row0, l_row0 + l_rows, stage0), what


def test_geometry_and_trace_tile_are_what_the_launcher_computed(rule_program):
    spans = {"whole tile": whole_span(5, 3, 6), "row block above": block_span(5, 4, 0, 17), "row block across the upper edge": block_span(5, 4, 17, 17),
             "row block inside": block_span(5, 4, 68, 17), "row block across the lower edge": block_span(5, 4, 136, 17),
             "row block below": block_span(5, 4, 187, 13), "list range": list_span(2, 4, 1234), "a redone block": (9, 2, 4, 68, 17, 0, 0, 0)}
    settings = [(params_of(), 3), (params_of(x0=4, y0=3, row_stride=2), 3), (params_of(flags=FLAG_RECORD_HITS), 64)]
    todo = [(p, b, s, w) for (p, b) in settings for s in spans for w in WINDOWS]
    got = run(rule_program, [pair_line(p, b, spans[s], WINDOWS[w]) for p, b, s, w in todo])
    seen = set()
    for (p, b, s, w), g in zip(todo, got):
        check_pair(g, p, b, spans[s], WINDOWS[w], "%s, window %s" % (s, w))
        seen.add((s, w, bool(g[0]), bool(g[1])))
    assert ("row block above", "part", True, True) in seen and ("row block inside", "part", True, False) in seen
    assert ("row block inside", "rows 30..50", True, True) in seen and ("whole tile", "no columns", True, True) in seen
    assert all(not windowed for s, _, windowed, _ in seen if s == "list range")  # a list pair ignores an open window


def test_every_row_block_of_a_tile_agrees_with_its_window_copy(rule_program):
    """the 12 blocks of test_render_in_row_blocks_is_the_same_film's tile, and blocks of other heights, under every window"""
    todo = []
    for per in (17, 13, 50, 200, 1):
        for r0 in range(0, H, per):
            for w in WINDOWS:
                todo.append((block_span(0, 12, r0, min(per, H - r0)), w))
    got = run(rule_program, [pair_line(params_of(), 3, s, WINDOWS[w]) for s, w in todo])
    for (s, w), g in zip(todo, got):
        check_pair(g, params_of(), 3, s, WINDOWS[w], "rows %d+%d, window %s" % (s[3], s[4], w))
    # the blocks' launches tile the window: every live pixel once
    for w in ("part", "the tile", "rows 30..50"):
        _, wx0, wx1, wy0, wy1 = WINDOWS[w]
        rows = sorted((g[4], g[4] + g[5], g[10]) for (s, ww), g in zip(todo, got) if ww == w and s[4] == min(17, H - s[3]) and s[3] % 17 == 0 and not g[1])
        assert rows[0][0] == wy0 and rows[-1][1] == wy1 and all(a[1] == b[0] for a, b in zip(rows, rows[1:]))
        assert all(stage0 == (lo - wy0) * (wx1 - wx0) for lo, _, stage0 in rows)


def was_pool_sample(p, win, window, k):
    """the tile create_impl put into ctx->params (and ctx->n_pix, ctx->batch_spp = 1, the hit log off) around its one enqueue_trace call"""
    _, wx0, wx1, wy0, wy1 = window
    live_px = (wx1 - wx0) * (wy1 - wy0) if win else p["tile_w"] * p["tile_h"]
    pp = dict(p)
    if win and live_px > 0:
        pp["x0"] += wx0
        pp["tile_w"] = wx1 - wx0
        pp["y0"] += wy0 * p["row_stride"]
        pp["tile_h"] = wy1 - wy0
    pp["tile_h"] = (pp["tile_h"] + k - 1) // k
    pp["row_stride"] = p["row_stride"] * k
    pp["flags"] = p["flags"] & ~FLAG_RECORD_HITS
    n_sample = pp["tile_w"] * pp["tile_h"]
    return was_enqueue_trace(pp, n_sample, 1, p.get("first_sample", 0), 1, 0)


def test_the_pool_sample_tile_is_the_one_create_made_by_swapping_the_context(rule_program):
    todo = [(params_of(x0=4, y0=3, row_stride=rs), w, k) for rs in (1, 3) for w in ("closed", "part", "no columns") for k in (1, 4, 7)]
    got = run(rule_program, [("sample", p["x0"], p["y0"], W, H, p["row_stride"]) + WINDOWS[w] + (k,) for p, w, k in todo])
    for (p, w, k), g in zip(todo, got):
        assert g == was_pool_sample(p, WINDOWS[w][0], WINDOWS[w], k), (p, w, k)
    assert got[[(w, k, p["row_stride"]) for p, w, k in todo].index(("part", 4, 3))] == [14, 3 + 30 * 3, 60, 30, 12, 1800, 1, 0, 0]
    lives = (0, 1, (128 << 10) - 1, 128 << 10, 3 * (128 << 10) + 5, 4096 ** 2)
    assert run(rule_program, [("step", v) for v in lives]) == [[max(1, v // (128 << 10))] for v in lives]


# ---- the work queues ----

def was_trace_chunk(n_paths, grid, bvh, override):
    waves = grid * (TRACE_BLOCK // 64)
    c = n_paths // (waves * 16) // 64 * 64
    chunk = min(max(c, 64), 256 if bvh else 1024)
    return override if override else chunk


def test_trace_chunk(rule_program):
    todo = [(px * n, grid, bvh, over) for px in N_PIX for n in N_SAMPLES for grid in (1, 256, 2048) for bvh in (0, 1) for over in (0, 128)]
    got = run(rule_program, [("trace", n_paths, grid, TRACE_BLOCK, bvh, over) for n_paths, grid, bvh, over in todo])
    assert [g[0] for g in got] == [was_trace_chunk(*t) for t in todo]
    assert {g[0] for g in got} >= {64, 128, 256, 1024}
    grids = [(n_paths, cap) for n_paths in (1, 255, 256, 257, 96 * 200 * 3, 4096 ** 2 * 256) for cap in (1, 256, 2048)]
    assert run(rule_program, [("tgrid", n_paths, TRACE_BLOCK, cap) for n_paths, cap in grids]) == \
        [[min((n_paths + TRACE_BLOCK - 1) // TRACE_BLOCK, cap)] for n_paths, cap in grids]


def was_shade_queue(n_pix, n, tail_count, tail_staged, shade_grid_cap, o_chunk, o_subs, o_tail_period):
    """enqueue_pair from `sp.chunk =` to `uint32_t sgrid =`; o_chunk: (uint32_t)atoi(getenv("DRT_SHADE_CHUNK")), -1 without the variable"""
    chunk = 64 // tail_count if tail_count else SHADE_PIXEL_CHUNK
    if tail_count and not tail_staged:
        tail_items, waves_ = (n_pix + chunk - 1) // chunk, shade_grid_cap * SHADE_WAVES
        if 2 * tail_items < waves_:
            chunk = max(1, chunk // 4)
        elif tail_items < 2 * waves_:
            chunk = max(1, chunk // 2)
    if o_chunk >= 0:
        chunk = max(1, min(64 // tail_count if tail_count else SHADE_PIXEL_CHUNK, o_chunk))
    groups = (n_pix + chunk - 1) // chunk
    inline_tail = tail_count != 0
    waves = shade_grid_cap * SHADE_WAVES
    subs = o_subs
    if subs == U32:
        p_balance = n_pix // (waves * 64)
        p_atomic = (256 + n - 1) // n
        P = min(max(max(p_balance, p_atomic), 1), chunk)
        subs = (chunk + P - 1) // P
        if subs == 1 and not inline_tail:
            subs = 0
    subs = min(subs, chunk)
    if subs == 0 or (subs == 1 and not inline_tail) or groups * (chunk + 1) >= U32:
        sub_pixels, items_per_group = chunk, 1
    else:
        sub_pixels = (chunk + subs - 1) // subs
        items_per_group = (chunk + sub_pixels - 1) // sub_pixels + (1 if inline_tail else 0)
    if groups * items_per_group >= U32:
        return [chunk, sub_pixels, items_per_group, 0, 0, 0, 1]  # return fail(-1, "tile too large for the shade work queue")
    n_items = groups * items_per_group
    tail_period_mains = 0
    if inline_tail and items_per_group > 1:
        mains = items_per_group - 1
        tail_period_mains = mains if groups >= 8 * waves else max(1, mains // 3)
        if o_tail_period:
            tail_period_mains = min(mains, o_tail_period)
    sgrid = min((n_items + SHADE_WAVES - 1) // SHADE_WAVES, shade_grid_cap)
    return [chunk, sub_pixels, items_per_group, n_items, tail_period_mains, sgrid, 0]


def test_shade_queue(rule_program):
    overrides = [UNSET, (2, U32, 0), (-1, 3, 0), (-1, U32, 2)]
    todo = list(itertools.product(N_PIX, N_SAMPLES, (0, 5, 16), (0, 1), (256, 1024, 2048), overrides))
    todo += [(96 * 200, 3, tc, 0, 1024, o) for tc in (0, 5, 16) for o in ((0, U32, 0), (1000, U32, 0), (U32, U32, 0), (-1, 0, 0), (-1, 1, 0), (-1, 1000, 0), (-1, U32, 1000))]
    got = run(rule_program, [("shade", px, n, tc, st, cap, SHADE_WAVES, SHADE_PIXEL_CHUNK) + tuple(o) for px, n, tc, st, cap, o in todo])
    for (px, n, tc, st, cap, o), g in zip(todo, got):
        assert g == was_shade_queue(px, n, tc, st, cap, *o), (px, n, tc, st, cap, o)
    assert not any(g[6] for g in got)
    assert len({tuple(g[:3]) for g in got}) > 20 and {g[0] for g in got} >= {1, 2, 3, 4, 6, 12, 16}  # every branch of the chunk rule


def test_shade_queue_too_large_for_its_counter(rule_program):
    """groups * items_per_group >= 2^32 - 1: one pixel per group (DRT_SHADE_CHUNK=1), on either side of the bound, with and without a tail pass"""
    todo = [(px, 1, tc, 0, 1024, (1, U32, 0)) for tc in (0, 16) for px in (U32 - 1, U32, 1 << 33, (U32 + 1) // 2 - 1, (U32 + 1) // 2)]
    got = run(rule_program, [("shade", px, n, tc, st, cap, SHADE_WAVES, SHADE_PIXEL_CHUNK) + tuple(o) for px, n, tc, st, cap, o in todo])
    for (px, n, tc, st, cap, o), g in zip(todo, got):
        assert g == was_shade_queue(px, n, tc, st, cap, *o), (px, tc)
    # (with a tail pass a group is two items up to 2^31 - 1 groups; from 2^31 on the rule falls back to one item per group)
    assert [g[6] for g in got] == [0, 1, 1, 0, 0] * 2 and got[8][2] == 2 and got[9][2] == 1


# ---- the splits ----

def test_equal_split(rule_program):
    todo = [(num, fit) for num in range(1, 301) for fit in (1, 3, 64, 125)]
    got = run(rule_program, [("split", num, fit) for num, fit in todo])
    for (num, fit), g in zip(todo, got):
        n_pairs, sizes = g[0], g[1:]
        was_n_pairs = (num + fit - 1) // fit
        was_each = (num + was_n_pairs - 1) // was_n_pairs  # render_pairs' `each`, enqueue_blocks' `n_blk`: the largest pair, then as now
        assert n_pairs == len(sizes) == was_n_pairs and max(sizes) == was_each <= fit, (num, fit)
        assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1 and sum(sizes) == num, (num, fit, sizes)
        assert sizes == sorted(sizes, reverse=True)
    assert got[todo.index((256, 125))] == [3, 86, 85, 85] and got[todo.index((100, 64))] == [2, 50, 50]
    assert run(rule_program, [("split", 0, 3)]) == [[0]]  # no samples: no pairs


def was_round_pairs(n_pix, batch_spp, k, n_in):
    budget = max(1, n_pix * batch_spp * 5 // 8)
    m_fit = min(min(k, budget), 4096)
    n_sp = (k + m_fit - 1) // m_fit
    m = (k + n_sp - 1) // n_sp
    p_fit = max(1, budget // m)
    n_pp = (n_in + p_fit - 1) // p_fit
    return [m, (n_in + n_pp - 1) // n_pp]


def test_round_pairs(rule_program):
    todo = [(n_pix, batch, k, n_in) for n_pix, batch in ((96 * 200, 3), (1024 ** 2, 64)) for k in (1, 7, 4096, 1 << 31) for n_in in (1, 1000, 1 << 24)]
    got = run(rule_program, [("round",) + t for t in todo])
    assert got == [was_round_pairs(*t) for t in todo]
    assert got[todo.index((96 * 200, 3, 1 << 31, 1 << 24))] == [4096, 8]


def test_row_blocks(rule_program):
    def was_count(num, batch, tile_h):  # render_pairs
        if not (num > batch and batch < 32 and tile_h >= 64):
            return 1
        want = (num * 8 + batch * 5 - 1) // (batch * 5)
        return min(min(want, 16), tile_h // 16)

    def was_fit(num, n_pix, batch, per, w):  # enqueue_blocks
        return max(1, min(min(num, 4096), n_pix * batch * 5 // 8 // (per * w)))

    counts = [(num, batch, h) for num in (1, 3, 4, 20, 23, 256, 5000) for batch in (1, 3, 16, 31, 32) for h in (48, 63, 64, 200, 4096)]
    got = run(rule_program, [("blocks",) + t for t in counts])
    assert [g[0] for g in got] == [was_count(*t) for t in counts]
    assert got[counts.index((23, 3, 200))] == [12] and got[counts.index((20, 3, 200))] == [11] and got[counts.index((256, 16, 4096))] == [16]
    rows = [(h, n) for h in (64, 200, 512, 4096) for n in (1, 2, 7, 8, 12, 16)]
    assert run(rule_program, [("brows",) + t for t in rows]) == [[(h + n - 1) // n] for h, n in rows]
    fits = [(num, w * h, batch, (h + n - 1) // n, w) for num in (3, 23, 256, 100000) for w, h, batch in ((96, 200, 3), (4096, 4096, 16), (512, 512, 4))
            for n in (2, 8, 12, 16)]
    fits += [(100000, 4096 * 4096, 31, 1, 4096), (5, 96 * 200, 1, 200, 96)]  # the cap of 4096 samples of a pixel; never less than one
    got = run(rule_program, [("fit",) + t for t in fits])
    assert [g[0] for g in got] == [was_fit(*t) for t in fits]
    assert got[fits.index((23, 96 * 200, 3, 17, 96))] == [22] and got[-2:] == [[4096], [1]]


# ---- the text ----

def test_the_launcher_launches_from_the_rules_text():
    rule = open(os.path.join(CSRC, "drt_pair_rule.h")).read()
    assert re.findall(r"#include\s+(\S+)", rule) == ["<algorithm>", "<cstdint>", '"drt_hip.h"']  # no HIP include, no kernel header
    assert "hip/" not in rule and "__global__" not in rule and "__device__" not in rule
    launcher = open(os.path.join(CSRC, "drt_launcher.hip")).read()
    assert '#include "drt_pair_rule.h"' in launcher
    for name in ("window_rows", "pair_geometry", "trace_tile", "pair_trace_tile", "pool_sample_step", "pool_sample_tile", "trace_grid", "trace_chunk",
                 "shade_queue", "equal_split", "row_block_count", "row_block_rows", "row_block_fit", "round_pairs"):
        assert len(re.findall(r"^static inline \w+ %s\(" % name, rule, re.M)) == 1, name  # defined once ...
        assert not re.search(r"^(static|inline)[\w\s]*\b%s\(" % name, launcher, re.M), name   # ... and not restated in the launcher
        if name != "trace_tile":  # (pair_trace_tile's own business)
            assert re.search(r"\b%s\(" % name, launcher), name
    pair = launcher[launcher.index("static int enqueue_pair(drt_context *ctx"):]
    pair = pair[:pair.index("\n}\n")]
    assert "getenv(" not in pair and pair.startswith("static int enqueue_pair(drt_context *ctx, const PairSpan &span)\n{")
    for fn in ("enqueue_pair", "enqueue_trace"):
        heads = re.findall(r"^static int %s\(([^)]*)\)" % fn, launcher, re.M)
        assert heads and all("=" not in h for h in heads), fn  # no default argument, in the declaration or the definition
    assert set(re.findall(r"^static int enqueue_trace\(([^)]*)\)", launcher, re.M)) == {"drt_context *ctx, const TraceTile &tile, const PairSpan &span"}
    for knob in ("DRT_SHADE_CHUNK", "DRT_DEBUG_SHADE_MODE", "DRT_DEBUG_TAIL_PHASE_A_OFF"):  # read once, when the context is created
        assert launcher.count('getenv("%s")' % knob) == 1
        assert abs(launcher.index('getenv("%s")' % knob) - launcher.index('getenv("DRT_SHADE_SUBS")')) < 800, knob
    create = launcher[launcher.index("static int create_impl(drt_context *ctx"):]
    create = create[:create.index("\n}\n")]
    assert not re.search(r"ctx->params\s*=\s*(pp|keep)\b|ctx->n_pix\s*=\s*(n_sample|keep_pix|npx)\b|ctx->batch_spp\s*=\s*1\b", create)
    assert re.search(r"struct Batch \{ PairSpan span; uint64_t seq; \};", launcher)
