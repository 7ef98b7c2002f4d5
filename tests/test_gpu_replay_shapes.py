"""GPU (-m gpu): the replay passes -- depth-cut films and sensor films (sections 5j and 5l) -- at the shapes of
tests/replay_shape_cases.py, which the shared cases of tests/cases.py never reach: more samples than a window of 64 headers, row
blocks, more work items than waves, tables outside LDS, four wavelength sets, 1, 6 and 7 cuts, and live edits with a pass bound.

Every shape runs once with depth cuts bound and once with a sensor bound (the two cannot be bound together). The rules are the two
suites' own: cut d is cases.oracle_render_device_pow at max_depth = d, the sensor film is sensor_rule.sensor_film over the oracle's
one-sample renders. Every comparison is cases.same_bits over pixels, means and variances, of the pass films and of the main film;
there is no tolerance anywhere. tests/test_replay_shapes_cpu.py shows on the oracle alone that the shapes are lit and tell depths
apart, and takes the kernel pairs counted here from csrc/drt_pair_rule.h."""
import contextlib
import os

import numpy as np
import pytest

import cases
import depth_cut_cases as DC
import pydrt
import replay_shape_cases as RS
import sensor_cases as SC

pytestmark = pytest.mark.gpu

KINDS = ("cuts", "sensor")


@contextlib.contextmanager
def environment(**knobs):
    saved = {k: os.environ.get(k) for k in knobs}
    try:
        for k, v in knobs.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class Cuts:
    """depth cuts as a pass: one film per cut, each the oracle's render at that depth"""

    def __init__(self, depths):
        self.depths = tuple(depths)
        self.names = ["cut %d (depth %d) against the oracle at that depth" % (c, d) for c, d in enumerate(self.depths)]

    def bind(self, r):
        r.bind_depth_cuts(self.depths)

    def read(self, r):
        return [r.read_depth_film(c) for c in range(len(self.depths))]

    def expected(self, key, bundle, params, **changes):
        return [RS.oracle_at(key, bundle, params, d, **changes) for d in self.depths]


class Sensor:
    """a sensor as a pass: one film, the rule's"""

    def __init__(self, curves):
        self.curves = curves
        self.names = ["the sensor film of %d channels against the rule" % len(curves)]

    def bind(self, r):
        r.bind_sensor(self.curves)

    def read(self, r):
        return [r.read_sensor_film()]

    def expected(self, key, bundle, params, **changes):
        return [RS.sensor_film(key, bundle, params, self.curves, **changes)]


def pass_of(kind, bundle, depths, channels=RS.CHANNELS):
    return Cuts(depths) if kind == "cuts" else Sensor(RS.curves_for(bundle, channels))


def render(bundle, params, pas, calls=None):
    """(main film, [pass films], stats, the context's batch_spp) of a fresh context with the pass bound"""
    r = pydrt.Renderer(bundle, params)
    try:
        pas.bind(r)
        for first, n in (calls or [(None, None)]):
            r.render(first, n)
        return r.read_film(), pas.read(r), r.stats(), r.batch_spp()
    finally:
        r.close()


def check(key, bundle, params, pas, main, films, what, **changes):
    """the main film against the oracle, every pass film against its rule"""
    RS.assert_film(main, RS.oracle_film(key, bundle, params, **changes), "%s: the main film against the oracle" % what)
    want = pas.expected(key, bundle, params, **changes)
    assert len(films) == len(want)
    for got, w, name in zip(films, want, pas.names):
        RS.assert_film(got, w, "%s: %s" % (what, name))


@pytest.fixture(scope="module")
def torch():
    """torch, imported and its device context made once, in no test's own time"""
    import torch
    torch.cuda.get_device_properties(0)
    torch.zeros(1, device="cuda:0")
    return torch


def shape_pass(name, kind, channels=RS.CHANNELS):
    bundle, params = RS.load(name)
    return bundle, params, pass_of(kind, bundle, RS.SHAPES[name]["cuts"], channels)


# ------------------------------------------------------------------------------------------------ A: header windows
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spp", [64, 65, 130])
def test_one_pair_takes_more_samples_than_a_window_of_headers(spp, kind):
    """64 samples fill the first window, 65 put one sample into the second, 130 go into a third: s0 != 0 in the header index and in
    the film update's divisor"""
    bundle, params, pas = shape_pass("windows", kind)
    p = RS.params_with(params, spp=spp)
    main, films, st, batch = render(bundle, p, pas)
    assert batch == spp and st.launches == 1, "one kernel pair is meant to take all %d samples (batch_spp %d, %d pairs)" % (spp, batch, st.launches)
    check("windows", bundle, p, pas, main, films, "%d samples in one pair" % spp)


@pytest.mark.parametrize("kind", KINDS)
def test_a_second_call_of_65_samples_starts_at_sample_65(kind):
    """render(0, 65); render(65, 65): first_sample != 0 meets s0 != 0, on films that hold the first call's samples"""
    bundle, params, pas = shape_pass("windows", kind)
    assert int(params.spp) == 130
    main, films, st, batch = render(bundle, params, pas, calls=[(0, 65), (65, 65)])
    assert batch == 130 and st.launches == 2
    check("windows", bundle, params, pas, main, films, "two calls of 65 samples")


# ------------------------------------------------------------------------------------------------ B: row blocks
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(RS.BLOCK_PLANS))
def test_row_blocks_offset_the_pass_films_and_stride_the_headers(name, kind):
    """Four blocks of 16 rows: the pass films start at pixel 0, 64, 128, 192 (blocks_4x64; 0, 32, 64, 96 of blocks_2x64) and the
    header slots per pixel are the pair's 4 (70) samples, not batch_spp's 2 (31). With DRT_NO_ROW_BLOCKS the same films from
    whole-tile pairs; the pair counts are the rule's (tests/test_replay_shapes_cpu.py), so neither run can be the other."""
    bundle, params, pas = shape_pass(name, kind)
    plan = RS.BLOCK_PLANS[name]
    assert not int(params.flags) & pydrt.FLAG_RECORD_HITS  # (the hit log rules row blocks out)
    with environment(DRT_NO_ROW_BLOCKS=None, DRT_POOL_BLOCKS=None):
        main, films, st, batch = render(bundle, params, pas)
    with environment(DRT_NO_ROW_BLOCKS="1", DRT_POOL_BLOCKS=None):
        main1, films1, st1, _ = render(bundle, params, pas)
    print("%s, %s: %d kernel pairs in row blocks, %d without" % (name, kind, st.launches, st1.launches))
    assert batch == int(params.batch_spp)
    assert st.launches == plan["blocks"] * len(plan["pairs"]) and st.launches >= 4 and st.redone_launches == 0
    assert st1.launches == len(plan["plain_pairs"]) and st1.launches != st.launches
    check(name, bundle, params, pas, main, films, "in row blocks")
    check(name, bundle, params, pas, main1, films1, "DRT_NO_ROW_BLOCKS")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(RS.BLOCK_PLANS))
def test_a_row_block_that_runs_out_of_records_is_replayed_narrowed(name, kind):
    """DRT_POOL_BLOCKS=1 leaves a pool for one worst-case sample of every tile pixel. A block pair of blocks_2x64 is 32 pixels x 70
    samples against 128 such paths: it runs out, and the block is rendered again in narrowed spans (PairSpan::narrowed: the context's
    own header stride, the block's film offset) with the pass bound. A block pair of blocks_4x64 is 64 pixels x 4 samples, as many
    paths as the pool is sized for in the worst case, so it cannot run out: there the knob must change nothing. (Measured on an
    MI355X: 8 launches redone for blocks_2x64, none for blocks_4x64, with either pass.)"""
    bundle, params, pas = shape_pass(name, kind)
    with environment(DRT_NO_ROW_BLOCKS=None, DRT_POOL_BLOCKS="1"):
        main, films, st, _ = render(bundle, params, pas)
    print("%s, %s: %d launches redone" % (name, kind, st.redone_launches))
    plan = RS.BLOCK_PLANS[name]
    if plan["rows"] * int(params.tile_w) * plan["pairs"][0] > RS.tile_pixels(params):
        assert st.redone_launches > 0, "no launch ran out of record blocks"
    check(name, bundle, params, pas, main, films, "tiny record pool under row blocks")


# ------------------------------------------------------------------------------------------------ C: more items than waves
@pytest.mark.parametrize("kind", KINDS)
def test_more_pixels_than_the_device_holds_waves(kind, torch):
    """Both passes launch at most as many waves as the device holds at once, and a wave draws work items until none is left: with
    more pixels than waves (the cut pass has n_sets items per pixel, the sensor pass one) over a thousand items go to waves that have
    finished one already -- the accumulators of another pixel, and the loop back edge the sensor kernel's first version hung on."""
    prop = torch.cuda.get_device_properties(0)
    bound = prop.multi_processor_count * prop.max_threads_per_multi_processor // 64
    bundle, params, pas = shape_pass("items", kind)
    n_pix = RS.tile_pixels(params)
    assert n_pix > bound, "%d pixels, and the device holds %d waves" % (n_pix, bound)
    main, films, st, _ = render(bundle, params, pas)
    assert st.launches == 1
    check("items", bundle, params, pas, main, films, "%d pixels on %d waves" % (n_pix, bound))


# ------------------------------------------------------------------------------------------------ D: tables outside LDS
@pytest.mark.parametrize("name", RS.TABLE_SHAPES)
def test_cuts_with_the_table_in_lds_and_in_memory(name):
    """rows_328, rows_54_2p5nm and lds_s256: drt_depth_cut_kernel<4, false>; rows_38_2p5nm and lds_s193: the same scenes' kernels
    with the table staged"""
    bundle, params, pas = shape_pass(name, "cuts")
    fits = RS.table_bytes(bundle) <= 64 * 1024
    assert fits == RS.SENSOR_LDS[(name, RS.sensor_channels(name)[0])][0]
    assert fits == (name in ("rows_38_2p5nm", "lds_s193"))
    main, films, _, _ = render(bundle, params, pas)
    check(name, bundle, params, pas, main, films, "table %s LDS" % ("in" if fits else "outside"))


@pytest.mark.parametrize("name, n", sorted(RS.SENSOR_LDS))
def test_sensor_with_table_and_curves_in_lds_the_curves_alone_and_the_fallback_between(name, n):
    """(table fits, table and curves fit): (False, False) the shade kernel and drt_sensor_kernel<false> both read memory; (True, True)
    both read LDS; (True, False) is the sensor film's own fallback -- the shade kernel reads LDS while the sensor kernel, with the
    same table eight curves short of fitting, reads memory -- and the fewer-curves run of the same shape is its control."""
    bundle, params, pas = shape_pass(name, "sensor", channels=n)
    table_fits = RS.table_bytes(bundle) <= 64 * 1024
    both_fit = table_fits and RS.sensor_bytes(bundle, n) <= 64 * 1024
    assert (table_fits, both_fit) == RS.SENSOR_LDS[(name, n)]
    assert n * bundle.S * 8 <= 64 * 1024
    main, films, _, _ = render(bundle, params, pas)
    assert films[0][1].shape[1] == n
    check(name, bundle, params, pas, main, films, "%d curves, table fits: %s, with the curves: %s" % (n, table_fits, both_fit))


# ------------------------------------------------------------------------------------------------ E: four wavelength sets
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["sets_s256", "sets_s193"])
def test_four_wavelength_sets(name, kind):
    """S = 256: no inactive lane in any set; S = 193: one active lane in the fourth"""
    bundle, params, pas = shape_pass(name, kind)
    assert bundle.S == RS.SHAPES[name]["S"] and (bundle.S + 63) // 64 == 4 and bundle.S % 64 == {"sets_s256": 0, "sets_s193": 1}[name]
    main, films, _, _ = render(bundle, params, pas)
    check(name, bundle, params, pas, main, films, "S = %d" % bundle.S)


@pytest.mark.parametrize("name", ["sets_s256", "sets_s193"])
def test_delta_curves_over_four_sets_give_the_main_films_own_columns(name):
    bundle, params = RS.load(name)
    S = bundle.S
    w = SC.delta_wavelengths(S)
    assert w[-1] == S - 1 and len(set(w // 64)) == 4
    (px, av, va), films, _, _ = render(bundle, params, Sensor(SC.delta_curves(S, w)))
    want = (np.concatenate([px[:, w], px[:, S:]], axis=1), av[:, w], va[:, w])
    RS.assert_film(films[0], want, "%s: delta curves against the main film from the device alone" % name)
    RS.assert_film((px, av, va), RS.oracle_film(name, bundle, params), "%s: the main film against the oracle" % name)
    assert (va[:, w] != 0).any(axis=0).all(), "every picked wavelength is lit, the last one included"


# ------------------------------------------------------------------------------------------------ F: cut counts
@pytest.mark.parametrize("depths", RS.DEEP_CUT_LISTS, ids=lambda d: "%d_cuts" % len(d))
def test_one_six_and_seven_cuts(depths):
    """drt_depth_cut_kernel<1>, <6> and <7>: every count is an instantiation with accumulators of its own"""
    bundle, params = DC.load(RS.DEEP)
    D = int(params.max_depth)
    assert len(depths) in (1, 6, 7) and depths[-1] < D
    main, films, st, _ = render(bundle, params, Cuts(depths))
    DC.assert_film(main, DC.oracle_at(RS.DEEP, D)[:3], "%d cuts: the main film against the oracle" % len(depths))
    for c, d in enumerate(depths):
        DC.assert_film(films[c], DC.oracle_at(RS.DEEP, d)[:3], "%d cuts: cut %d (depth %d) against the oracle at that depth" % (len(depths), c, d))
    assert cases.stat_counts(st) == cases.stat_counts(DC.oracle_at(RS.DEEP, D)[4])


# ------------------------------------------------------------------------------------------------ G: live edits
def live_pass(kind, bundle):
    return pass_of(kind, bundle, RS.LIVE_CUTS)


def changed_rows(before, after):
    """(first_row, rows) of the smallest range that holds every SPD row in which the two bundles differ"""
    new, old = after.spds(), before.spds()
    rows = [k for k in range(new.shape[0]) if not cases.same_bits(new[k], old[k])]
    assert rows
    return rows[0], new[rows[0]:rows[-1] + 1]


def apply_edit(r, edit, before, after):
    if edit == "set_camera":
        r.set_camera(after)
    elif edit.startswith("update_surfaces"):
        r.update_surfaces(pydrt.surface_rows(after), rebuild=edit.endswith("rebuild"))
    elif edit == "update_spectra":
        first, rows = changed_rows(before, after)
        r.update_spectra(rows, first=first)
    else:
        builds = r.hierarchy_report()["device_builds"]
        r.rebuild_hierarchy()
        assert r.hierarchy_report()["device_builds"] == builds + 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("edit", sorted(RS.EDITS))
def test_a_live_edit_between_two_renders_with_a_pass_bound(edit, kind):
    """render, drt_reset_film, the edit, render: main and pass films of the second render are a fresh context's on the edited bundle
    with the same pass bound, and the rule's on the edited scene; the first render's are the rule's on the scene before, and differ
    (after drt_rebuild_hierarchy, which changes no result: the same)."""
    before, after = RS.edit_case(edit)
    forced = RS.EDITS[edit][2]
    target = after if after is not None else before
    p = RS.live_params()
    pas = live_pass(kind, before)
    with environment(DRT_FORCE_BVH="1" if forced else None):
        r = pydrt.Renderer(before, p)
        try:
            assert bool(r.stats().path_flags & pydrt.PATH_BVH) == forced
            pas.bind(r)
            r.render()
            first = (r.read_film(), pas.read(r))
            r.reset_film()
            assert not any(a.any() for film in pas.read(r) for a in film), "drt_reset_film zeroes the pass films"
            apply_edit(r, edit, before, after)
            r.render()
            second = (r.read_film(), pas.read(r))
        finally:
            r.close()
        fresh_main, fresh_films, _, _ = render(target, p, pas)
    check(RS.LIVE, before, p, pas, first[0], first[1], "%s: before the edit" % edit)
    RS.assert_film(second[0], fresh_main, "%s: the main film against a fresh context's" % edit)
    for got, want, name in zip(second[1], fresh_films, pas.names):
        RS.assert_film(got, want, "%s: against a fresh context, %s" % (edit, name.split(" against")[0]))
    check(RS.EDITS[edit][:2] if after is not None else RS.LIVE, target, p, pas, second[0], second[1], "%s: after the edit" % edit)
    same = cases.same_bits(first[0][0], second[0][0]), cases.same_bits(first[1][-1][0], second[1][-1][0])
    assert same == ((True, True) if after is None else (False, False)), "%s: (main, pass) film unchanged: %s" % (edit, same)


def torch_film(torch, n, S):
    dev = torch.device("cuda:0")
    return [torch.zeros((n, S + 1), dtype=torch.float64, device=dev), torch.zeros((n, S), dtype=torch.float64, device=dev),
            torch.zeros((n, S), dtype=torch.float64, device=dev)]


@pytest.mark.parametrize("kind", KINDS)
def test_the_main_film_in_the_callers_tensors_the_pass_films_in_the_context(kind, torch):
    """drt_bind_film moves the main film into caller memory; the pass films stay the context's own"""
    bundle, p = cases.load_case(RS.LIVE)
    pas = live_pass(kind, bundle)
    t = torch_film(torch, RS.tile_pixels(p), bundle.S)
    r = pydrt.Renderer(bundle, p)
    try:
        r.bind_film(*(x.data_ptr() for x in t))
        pas.bind(r)
        r.render()
        r.synchronize()
        main = tuple(x.cpu().numpy() for x in t)
        films = pas.read(r)
        RS.assert_film(r.read_film(), main, "drt_read_film against the tensors")
    finally:
        r.close()
    check(RS.LIVE, bundle, p, pas, main, films, "main film in torch tensors")


@pytest.mark.parametrize("kind", KINDS)
def test_on_a_torch_stream(kind, torch):
    """drt_set_stream: trace, shade and the replay pass on the caller's stream (its handle is not 0, which would mean the context's own);
    the tensors are copied back on that stream with nothing in between, so they are right only if the kernels ran there"""
    bundle, p = cases.load_case(RS.LIVE)
    pas = live_pass(kind, bundle)
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    assert stream.cuda_stream != 0
    r = pydrt.Renderer(bundle, p)
    try:
        with torch.cuda.stream(stream):
            t = torch_film(torch, RS.tile_pixels(p), bundle.S)
            r.bind_film(*(x.data_ptr() for x in t))
            r.set_stream(stream.cuda_stream)
            pas.bind(r)
            r.render()
            main = tuple(x.to("cpu", non_blocking=False).numpy() for x in t)
        films = pas.read(r)
        RS.assert_film(r.read_film(), main, "drt_read_film against the tensors")
    finally:
        r.close()
    check(RS.LIVE, bundle, p, pas, main, films, "on a torch stream")
