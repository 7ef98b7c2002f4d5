"""The shapes of tests/replay_shape_cases.py without a GPU (-m "not gpu"): every shape is a valid input for what its GPU test claims.

On the oracle alone (oracle_py.oracle_render_tile, math_mode=MATH_DEVICE): the wavelength counts and the byte sizes a shape is chosen
for, that neighbouring cuts have different films, that every sensor channel's means and variances are lit, and that the row blocks of
shape B and the quarters of shape C each hold pixels in which neighbouring cuts differ -- so a black tile, or a block that no cut
tells from the next, cannot pass on the GPU for the wrong reason. The kernel pairs that tests/test_gpu_replay_shapes.py counts are
taken from csrc/drt_pair_rule.h through tests/host/pair_rule_main.cpp."""
import os
import subprocess

import numpy as np
import pytest

import cases
import depth_cut_cases as DC
import replay_shape_cases as RS

CSRC = os.path.join(cases.REPO, "daily-ray-trace_amd", "csrc")
INCLUDE = os.path.join(cases.REPO, "include")


@pytest.mark.parametrize("name", sorted(RS.SHAPES))
def test_wavelengths_rows_and_tile_are_the_shapes(name):
    s = RS.SHAPES[name]
    bundle, params = RS.load(name)
    tile = s.get("tile", {})
    assert bundle.S == s["S"] and int(bundle.scene.num_spds) == s["rows"]
    assert RS.tile_pixels(params) == tile.get("tile_w", s["size"][0]) * tile.get("tile_h", s["size"][1])
    assert list(s["cuts"]) == sorted(set(s["cuts"])) and 1 <= s["cuts"][0] and s["cuts"][-1] <= s["depth"]


def test_what_each_table_shape_makes_of_64_kib():
    """the figures the shapes' descriptions give (scene rows), and what the launcher measures (device rows)"""
    scene = {n: RS.scene_table_bytes(RS.load(n)[0]) for n in RS.TABLE_SHAPES}
    assert scene == {"rows_328": 328 * 69 * 8, "rows_54_2p5nm": 54 * 137 * 8, "rows_38_2p5nm": 38 * 137 * 8, "lds_s256": 28 * 256 * 8, "lds_s193": 28 * 193 * 8}
    assert scene["rows_328"] == 181056 > RS.LDS_BYTES and scene["rows_54_2p5nm"] == 59184 <= RS.LDS_BYTES and scene["lds_s256"] == 57344 <= RS.LDS_BYTES
    rows = {n: RS.device_spd_rows(RS.load(n)[0]) for n in RS.TABLE_SHAPES}
    assert rows == {"rows_328": 488, "rows_54_2p5nm": 77, "rows_38_2p5nm": 53, "lds_s256": 38, "lds_s193": 38}
    for (name, n), (table_fits, both_fit) in RS.SENSOR_LDS.items():
        bundle = RS.load(name)[0]
        assert (RS.table_bytes(bundle) <= RS.LDS_BYTES) == table_fits, name
        assert (table_fits and RS.sensor_bytes(bundle, n) <= RS.LDS_BYTES) == both_fit, (name, n)
        assert n * bundle.S * 8 <= RS.LDS_BYTES, "the curves alone must fit, or the bind is refused"
    # the two shapes in which the sensor kernel falls back alone, each with its control
    assert RS.table_bytes(RS.load("rows_38_2p5nm")[0]) == 58088 and RS.sensor_bytes(RS.load("rows_38_2p5nm")[0], 8) == 66856
    assert RS.sensor_bytes(RS.load("rows_38_2p5nm")[0], 1) == 59184
    assert RS.table_bytes(RS.load("lds_s193")[0]) == 58672 and RS.sensor_bytes(RS.load("lds_s193")[0], 8) == 71024
    assert RS.sensor_bytes(RS.load("lds_s193")[0], 3) == 63304
    # E: S = 256 reads the table from memory in every kernel, S = 193 from LDS with three curves behind it
    assert RS.table_bytes(RS.load("sets_s256")[0]) == 77824 > RS.LDS_BYTES and RS.sensor_bytes(RS.load("sets_s193")[0], RS.CHANNELS) == 63304
    # every other shape keeps table and curves in LDS
    for name in ("windows", "blocks_4x64", "blocks_2x64", "items"):
        assert RS.sensor_bytes(RS.load(name)[0], RS.CHANNELS) <= RS.LDS_BYTES


def spp_variants(name):
    return (64, 65, 130) if name == "windows" else (RS.SHAPES[name]["spp"],)


@pytest.mark.parametrize("name", sorted(RS.SHAPES))
def test_neighbouring_cuts_have_different_films(name):
    bundle, params = RS.load(name)
    depths = RS.SHAPES[name]["cuts"] + (() if RS.SHAPES[name]["cuts"][-1] == RS.SHAPES[name]["depth"] else (RS.SHAPES[name]["depth"],))
    for spp in spp_variants(name):
        films = [RS.oracle_at(name, bundle, params, d, cpu=True, spp=spp) for d in depths]
        for (a, fa), (b, fb) in zip(zip(depths, films), list(zip(depths, films))[1:]):
            for k, buf in enumerate(("pixels", "means", "variances")):
                assert not cases.same_bits(fa[k], fb[k]), "%s, %d samples: the %s at depths %d and %d are the same" % (name, spp, buf, a, b)


@pytest.mark.parametrize("depths", RS.DEEP_CUT_LISTS, ids=lambda d: "%d_cuts" % len(d))
def test_neighbouring_cuts_of_the_deep_lists_differ(depths):
    D = int(DC.load(RS.DEEP)[1].max_depth)
    assert len(depths) in (1, 6, 7) and depths[-1] < D
    full = depths + (D,)  # the single cut against the main film, too
    for a, b in zip(full, full[1:]):
        fa, fb = DC.oracle_at_cpu(RS.DEEP, a), DC.oracle_at_cpu(RS.DEEP, b)
        for k in range(3):
            assert not cases.same_bits(fa[k], fb[k]), "depths %d and %d" % (a, b)


@pytest.mark.parametrize("name", sorted(RS.SHAPES))
def test_every_sensor_channel_is_lit(name):
    bundle, params = RS.load(name)
    for spp in spp_variants(name):
        for n in RS.sensor_channels(name):
            px, av, va = RS.sensor_film(name, bundle, params, RS.curves_for(bundle, n), cpu=True, spp=spp)
            assert px.shape == (RS.tile_pixels(params), n + 1)
            assert (av != 0).any(axis=0).all() and (va != 0).any(axis=0).all(), "%s, %d curves" % (name, n)
            assert np.array_equal(px[:, n], np.full(px.shape[0], float(spp)))


def fractions(name, parts):
    """per neighbouring pair of cuts and per part of the tile's rows: the share of pixels in which the two cuts differ"""
    bundle, params = RS.load(name)
    depths = RS.SHAPES[name]["cuts"]
    films = [RS.oracle_at(name, bundle, params, d, cpu=True) for d in depths]
    w, h = int(params.tile_w), int(params.tile_h)
    assert h % parts == 0
    out = []
    for fa, fb in zip(films, films[1:]):
        differ = RS.differing_pixels(fa, fb).reshape(parts, h // parts * w)
        out.append(differ.mean(axis=1))
    return np.array(out)


@pytest.mark.parametrize("name", sorted(RS.BLOCK_PLANS))
def test_every_row_block_holds_pixels_in_which_neighbouring_cuts_differ(name):
    plan = RS.BLOCK_PLANS[name]
    f = fractions(name, plan["blocks"])
    print(name, f)
    assert f.shape[1] == 4 and (f >= 0.25).all(), f
    # and its sensor channels are lit block by block
    bundle, params = RS.load(name)
    av = RS.sensor_film(name, bundle, params, RS.curves_for(bundle), cpu=True)[1]
    per = plan["rows"] * int(params.tile_w)
    for b in range(plan["blocks"]):
        assert (av[b * per:(b + 1) * per] != 0).any(axis=0).all(), "block %d" % b


def test_every_quarter_of_the_items_shape_holds_pixels_in_which_neighbouring_cuts_differ():
    f = fractions("items", 4)
    print(f)
    assert (f >= 0.05).all(), f


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pair") / "pair_rule_main"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-I" + INCLUDE, os.path.join(cases.REPO, "tests", "host", "pair_rule_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.mark.parametrize("name", sorted(RS.BLOCK_PLANS))
def test_the_block_plans_are_the_pair_rules(rule_program, name):
    """what render_pairs and enqueue_blocks (csrc/drt_launcher.hip) ask the header, in their order"""
    plan = RS.BLOCK_PLANS[name]
    _, params = RS.load(name)
    spp, batch, w, h = int(params.spp), int(params.batch_spp), int(params.tile_w), int(params.tile_h)

    def ask(*line):
        r = subprocess.run([rule_program], input=" ".join(str(v) for v in line) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        return [int(v) for v in r.stdout.split()[1:]]

    assert ask("blocks", spp, batch, h) == [plan["blocks"]] and plan["blocks"] > 1
    assert ask("brows", h, plan["blocks"]) == [plan["rows"]] and plan["rows"] * plan["blocks"] == h
    assert ask("fit", spp, w * h, batch, plan["rows"], w) == [plan["fit"]]
    assert ask("split", spp, plan["fit"]) == [len(plan["pairs"])] + list(plan["pairs"])
    assert ask("split", spp, batch) == [len(plan["plain_pairs"])] + list(plan["plain_pairs"])
    assert plan["blocks"] * len(plan["pairs"]) >= 4 and plan["blocks"] * len(plan["pairs"]) != len(plan["plain_pairs"])
    # a block's pair has its own header stride, and its films start at the block's first pixel
    assert plan["pairs"][0] != batch and plan["rows"] * w > 0
    # the header array (tile pixels x batch_spp slots) holds a block's pair
    assert plan["rows"] * w * plan["pairs"][0] <= w * h * batch
