"""CPU: the continuation of adaptive sampling (drt_render_adaptive_continue) where no device is needed: the C-ABI's declarations,
the per-pixel rule (tests/adaptive_resume_rule.py) on hand-built snapshot tables, the version-3 checkpoint through libdrt_host.so,
and the drt_render host refusing bad DRT_ADAPTIVE_CHECKPOINT_ROUNDS / DRT_ADAPTIVE_RESUME settings before it touches a device."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import adaptive_resume_rule as RR
import adaptive_rule as R
import cases
import pydrt

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")


def test_the_header_declares_and_pydrt_lists_the_continuation():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "drt_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+drt_render_adaptive_continue\s*\(\s*drt_context\s*\*\s*ctx\s*,\s*drt_adaptive\s*\*\s*a\s*,\s*uint32_t\s+max_rounds\s*,"
                     r"\s*uint32_t\s*\*\s*still_active\s*\)\s*;", header)
    assert re.search(r"int\s+drt_group_render_adaptive_continue\s*\(\s*drt_group\s*\*\s*g\s*,\s*drt_adaptive\s*\*\s*a\s*,\s*uint32_t\s+max_rounds\s*,"
                     r"\s*uint32_t\s*\*\s*still_active\s*\)\s*;", header)
    assert {"drt_render_adaptive_continue", "drt_group_render_adaptive_continue"} <= set(pydrt.HIP_SYMBOLS)
    assert callable(pydrt.Renderer.render_adaptive_continue) and callable(pydrt.Group.render_adaptive_continue)
    assert C.sizeof(pydrt.Adaptive) == 48  # the struct did not grow: max_rounds and still_active are arguments


# a 3-wavelength table: rw = 1, cy = (1, 2, 1), interval 1 -> N = 4, so a pixel with mean m and variance sum v in every column has
# Y = m and E = sqrt(v / (n (n - 1)))
SPDS = np.array([[1.0, 1.0, 1.0], [1.0, 2.0, 1.0]])


def synthetic_snapshots(n_pix, ns, seed):
    """per count n: means 1, variance sums such that E(n) = e0[p] / sqrt(n) * wobble -- pixels converge at different counts"""
    rng = np.random.default_rng(seed)
    e0 = rng.uniform(0.05, 1.5, n_pix)
    snaps = {}
    for n in ns:
        e = e0 / np.sqrt(n) * rng.uniform(0.8, 1.25, n_pix)
        snaps[n] = (np.ones((n_pix, 3)), np.repeat((e * e * n * (n - 1))[:, None], 3, axis=1))
    return snaps


def fresh(snaps, n_pix, mn, mx, st, rel, floor=0.0):
    return R.sample_counts(lambda n: snaps[n], SPDS, 0, 1, 1.0, n_pix, mn, mx, st, rel, floor)[0]


def cont(snaps, start, mx, st, rel, floor=0.0, max_rounds=0):
    return RR.continue_counts(lambda n: snaps[n], SPDS, 0, 1, 1.0, start, mx, st, rel, floor, max_rounds)


def test_refining_is_the_same_as_having_asked_for_it_at_once():
    n_pix = 400
    snaps = synthetic_snapshots(n_pix, R.rounds(4, 40, 4), 11)
    p = fresh(snaps, n_pix, 4, 24, 4, 0.2)
    assert np.unique(p).size == 6
    counts, ran, paths, left = cont(snaps, p, 40, 4, 0.1)
    want = fresh(snaps, n_pix, 4, 40, 4, 0.1)
    grew = counts > p
    assert np.array_equal(counts, want) and left.size == 0
    assert np.unique(p[grew]).size >= 3 and (~grew).any() and (counts == 40).any() and (grew & (counts < 40)).any()
    assert paths == int(want.sum()) - int(p.sum()) and ran == int((counts - p).max()) // 4
    # split equals whole, the parts' samples add up, and the list left after k rounds is what the rule keeps, ascending
    for k in (1, 2, 3):
        c1, ran1, paths1, left1 = cont(snaps, p, 40, 4, 0.1, max_rounds=k)
        assert ran1 == k and left1.size > 0 and np.all(np.diff(left1) > 0)
        assert RR.allotment_contract(c1, left1, 40, 4)
        c2, ran2, paths2, left2 = cont(snaps, c1, 40, 4, 0.1)
        assert np.array_equal(c2, want) and paths1 + paths2 == paths and ran1 + ran2 == ran
    # a uniform start is a fresh start
    c3, ran3, paths3, _ = cont(snaps, np.full(n_pix, 4), 40, 4, 0.1)
    assert np.array_equal(c3, want) and paths3 + 4 * n_pix == int(want.sum())


def test_a_loosened_continuation_differs_from_the_fresh_render_where_it_should():
    n_pix = 400
    snaps = synthetic_snapshots(n_pix, R.rounds(4, 40, 4), 12)
    p = fresh(snaps, n_pix, 4, 24, 4, 0.1)
    # the same cap: nothing is left to do
    same, ran, paths, left = cont(snaps, p, 24, 4, 0.3)
    assert np.array_equal(same, p) and ran == 0 and paths == 0 and left.size == 0
    # a larger cap, a looser bound: only pixels P left at 24 go on; the others keep what P gave them, more than P' alone would have
    counts, ran, paths, left = cont(snaps, p, 40, 4, 0.15)
    want = fresh(snaps, n_pix, 4, 40, 4, 0.15)
    grew = counts > p
    assert grew.any() and (p[grew] == 24).all() and (counts >= want).all() and (counts != want).any()
    assert np.array_equal(counts[~grew], p[~grew]) and ((counts == 40) | (counts == p) | grew).all()


def test_the_allotment_contract():
    counts = np.array([4, 8, 12, 24, 24, 40])
    assert RR.allotment_contract(counts, [3, 4], 40, 5)          # one count: any step
    assert RR.allotment_contract(counts, [0, 1, 2], 40, 4)       # 36, 32, 28
    assert not RR.allotment_contract(counts, [0, 1, 2], 40, 5)
    assert RR.allotment_contract(counts, [0, 1, 2], 40, 2) and RR.allotment_contract(counts, [], 40, 5)


# ---- the checkpoint of an adaptive render (host/drt_checkpoint.c) ----

W, H, S = 5, 3, 69
N_PX = W * H
f64p = C.POINTER(C.c_double)


class AdaptiveLine(C.Structure):
    _fields_ = [("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("step", C.c_uint32), ("rel_error", C.c_double), ("floor", C.c_double)]


def host():
    Hl = pydrt.host_lib()
    Hl.parse_config.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]
    Hl.parse_config.restype = None
    Hl.drt_host_write_outputs.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, f64p, f64p, f64p,
                                          C.c_int, C.c_uint32, C.c_uint64]
    Hl.drt_host_write_outputs_adaptive.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, f64p, f64p, f64p,
                                                   C.c_int, C.c_uint64, C.POINTER(AdaptiveLine)]
    for f in (Hl.drt_host_load_checkpoint, Hl.drt_host_load_checkpoint_adaptive):
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, f64p, f64p, f64p, C.POINTER(C.c_uint32)]
    Hl.drt_host_load_checkpoint_adaptive.argtypes = Hl.drt_host_load_checkpoint.argtypes + [C.POINTER(AdaptiveLine)]
    Hl.drt_host_checkpoint_error.restype = C.c_char_p
    return Hl


def config_for(workdir, scene, spp):
    text = ("num_pixel_samples %d\nmax_cast_depth 4\noutput_width %d\noutput_height %d\nmin_wl 380.0\nmax_wl 720.0\nwl_interval 5.0\n"
            "pixel_scheme pixel_random\ninput_scene %s\noutput_spd %s/output.spd\naverage_spd %s/average.spd\nvariance_spd %s/variance.spd\n"
            % (spp, W, H, scene, workdir, workdir, workdir)).encode()
    buf = C.create_string_buffer(1136)
    host().parse_config(C.create_string_buffer(text, len(text) + 1), len(text), buf)
    return buf


def film_with_counts(counts, rng):
    counts = np.asarray(counts, dtype=np.float64)
    px = np.zeros((N_PX, S + 1))
    px[:, :S] = rng.uniform(0, 5, (N_PX, S)) * counts[:, None]
    px[:, S] = counts
    return px, px[:, :S] / counts[:, None], rng.uniform(0, 2, (N_PX, S))


def ptrs(*arrays):
    return [a.ctypes.data_as(f64p) for a in arrays]


@pytest.fixture
def workdir():
    d = tempfile.mkdtemp(prefix="ack", dir="/tmp")  # config_arguments path fields hold 63 characters
    open(os.path.join(d, "s.scn"), "w").write("Camera\n")
    yield d
    shutil.rmtree(d)


def load_adaptive(cfg):
    a, b, c = np.zeros((N_PX, S + 1)), np.zeros((N_PX, S)), np.zeros((N_PX, S))
    most, line = C.c_uint32(77), AdaptiveLine()
    rc = host().drt_host_load_checkpoint_adaptive(cfg, W, H, S, 1, *ptrs(a, b, c), C.byref(most), C.byref(line))
    return rc, most.value, (a, b, c), line, host().drt_host_checkpoint_error().decode()


def load_uniform(cfg):
    a, b, c = np.zeros((N_PX, S + 1)), np.zeros((N_PX, S)), np.zeros((N_PX, S))
    done = C.c_uint32(77)
    rc = host().drt_host_load_checkpoint(cfg, W, H, S, 1, *ptrs(a, b, c), C.byref(done))
    return rc, done.value, host().drt_host_checkpoint_error().decode()


def write_adaptive(cfg, film, line=None):
    line = line or AdaptiveLine(4, 24, 4, 0.05, 0.25)
    return host().drt_host_write_outputs_adaptive(cfg, W, H, S, 380.0, 5.0, *ptrs(*film), 1, 1, C.byref(line))


def test_a_version_3_checkpoint_round_trips_with_per_pixel_counts(workdir):
    rng = np.random.default_rng(4)
    scene = os.path.join(workdir, "s.scn")
    cfg = config_for(workdir, scene, 24)
    counts = rng.choice([4, 8, 12, 16, 20, 24], N_PX)
    counts[3] = 24
    film = film_with_counts(counts, rng)
    assert write_adaptive(cfg, film) == 0
    manifest = open(os.path.join(workdir, "output.spd.ckpt")).read()
    assert manifest.startswith("drt-checkpoint 3\nsamples 24\nwidth 5\nheight 3\n")
    assert manifest.splitlines()[-1] == "adaptive min_spp 4 max_spp 24 step 4 rel_error 0.050000000000000003 floor 0.25"
    assert sorted(os.listdir(workdir)) == ["average.spd", "average.spd.ck0", "output.spd", "output.spd.ck0", "output.spd.ckpt", "s.scn",
                                           "variance.spd", "variance.spd.raw.ck0"]
    rc, most, got, line, why = load_adaptive(cfg)
    assert rc == 0 and most == 24, why
    assert all(np.array_equal(g, f) for g, f in zip(got, film))
    assert (line.min_spp, line.max_spp, line.step, line.rel_error, line.floor) == (4, 24, 4, 0.05, 0.25)
    # a job that asks for more samples takes it over too; one that asks for fewer than a pixel holds does not
    assert load_adaptive(config_for(workdir, scene, 40))[0] == 0
    rc, _, _, _, why = load_adaptive(config_for(workdir, scene, 20))
    assert rc != 0 and "num_pixel_samples (20)" in why
    # the uniform loader keeps to version 2
    rc, done, why = load_uniform(cfg)
    assert rc != 0 and done == 0 and "not a checkpoint manifest of this version" in why
    # the next one goes to the other generation through the same switch, and retires this one
    film2 = film_with_counts(np.minimum(counts + 4, 24), rng)
    assert write_adaptive(cfg, film2) == 0
    assert "\ngeneration 1\n" in open(os.path.join(workdir, "output.spd.ckpt")).read() and not os.path.exists(os.path.join(workdir, "output.spd.ck0"))
    rc, most, got, _, why = load_adaptive(cfg)
    assert rc == 0 and np.array_equal(got[0], film2[0]), why
    # a uniform checkpoint (version 2) is a valid start
    film4 = film_with_counts(np.full(N_PX, 4), rng)
    assert host().drt_host_write_outputs(cfg, W, H, S, 380.0, 5.0, *ptrs(*film4), 1, 4, 1) == 0
    assert open(os.path.join(workdir, "output.spd.ckpt")).read().startswith("drt-checkpoint 2\nsamples 4\n")
    rc, most, got, line, why = load_adaptive(cfg)
    assert rc == 0 and most == 4 and np.array_equal(got[0], film4[0]) and line.step == 0, why
    assert load_uniform(cfg)[:2] == (0, 4)


@pytest.mark.parametrize("what, text", [("fraction", "holds 8.5 samples at pixel 6"), ("one", "holds 1 samples at pixel 6"),
                                        ("above", "holds 28 samples at pixel 6"), ("mean", "does not belong"),
                                        ("nan", "samples at pixel 6"), ("largest", "the manifest says 24")])
def test_the_adaptive_loader_refuses_films_whose_counts_or_means_are_off(workdir, what, text):
    rng = np.random.default_rng(5)
    cfg = config_for(workdir, os.path.join(workdir, "s.scn"), 24)
    counts = rng.choice([4, 8, 12, 16, 20, 24], N_PX)
    counts[3] = 24
    px, av, va = film_with_counts(counts, rng)
    assert write_adaptive(cfg, (px, av, va)) == 0 and load_adaptive(cfg)[0] == 0
    if what == "mean":
        av[6] = px[6, :S] / (counts[6] + 4)  # the mean of another count
    elif what == "largest":
        px[counts == 24, S] = 20.0           # every count a valid one, none the manifest's largest
        av[counts == 24] = px[counts == 24, :S] / 20.0
    else:
        px[6, S] = {"fraction": 8.5, "one": 1.0, "above": 28.0, "nan": float("nan")}[what]
    gen = [l for l in open(os.path.join(workdir, "output.spd.ckpt")).read().splitlines() if l.startswith("generation")][0].split()[1]
    H_ = host()
    H_.drt_host_write_spd.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, f64p]
    assert H_.drt_host_write_spd(os.path.join(workdir, "output.spd.ck" + gen).encode(), W, H, S, 1, 380.0, 5.0, *ptrs(px)) == 0
    assert H_.drt_host_write_spd(os.path.join(workdir, "average.spd.ck" + gen).encode(), W, H, S, 0, 380.0, 5.0, *ptrs(av)) == 0
    rc, most, _, _, why = load_adaptive(cfg)
    assert rc != 0 and most == 0 and text in why, why


@pytest.mark.parametrize("env, name", [
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_CHECKPOINT_ROUNDS": "0"}, "DRT_ADAPTIVE_CHECKPOINT_ROUNDS"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_CHECKPOINT_ROUNDS": "x"}, "DRT_ADAPTIVE_CHECKPOINT_ROUNDS"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_CHECKPOINT_ROUNDS": "-1"}, "DRT_ADAPTIVE_CHECKPOINT_ROUNDS"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_CHECKPOINT_ROUNDS": "1.5"}, "DRT_ADAPTIVE_CHECKPOINT_ROUNDS"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_RESUME": "yes"}, "DRT_ADAPTIVE_RESUME"),
    ({"DRT_ADAPTIVE_CHECKPOINT_ROUNDS": "2"}, "DRT_ADAPTIVE_CHECKPOINT_ROUNDS"),
    ({"DRT_ADAPTIVE_RESUME": "1"}, "DRT_ADAPTIVE_RESUME"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_CHECKPOINT_ROUNDS": "2", "DRT_CHECKPOINT_SPP": "8"}, "DRT_CHECKPOINT_SPP"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_RESUME": "1", "DRT_RESUME": "1"}, "DRT_RESUME"),
])
def test_the_host_refuses_bad_checkpoint_settings_before_any_device_call(tmp_path, env, name):
    """Exit status nonzero, the variable named on stderr, and no device opened: HIP_VISIBLE_DEVICES hides every device, so a run
    that got as far as the launcher would fail there with the launcher's message instead."""
    (tmp_path / "config.cfg").write_text(open(os.path.join(REPO, "config.cfg")).read())
    os.symlink(os.path.join(REPO, "scenes"), tmp_path / "scenes")
    os.symlink(os.path.join(REPO, "spectra"), tmp_path / "spectra")
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full.update(env)
    full["HIP_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([BIN, "config.cfg"], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0
    assert name in r.stderr, r.stderr
    assert "HIP launcher" not in r.stderr and "Rendering" not in r.stdout
