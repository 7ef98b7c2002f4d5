"""CPU: adaptive sampling's C-ABI struct, the convergence rule (tests/adaptive_rule.py) on hand-built films, and the drt_render
host refusing bad DRT_ADAPTIVE_* settings before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_rule as R
import cases
import pydrt

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")


def test_adaptive_struct_matches_the_header():
    A = pydrt.Adaptive
    assert C.sizeof(A) == 48
    assert [(n, getattr(A, n).offset) for n, _ in A._fields_] == [
        ("min_spp", 0), ("max_spp", 4), ("step", 8), ("flags", 12), ("rel_error", 16), ("floor", 24), ("rounds", 32),
        ("pixels_at_max", 36), ("paths", 40)]
    header = open(os.path.join(REPO, "include", "drt_hip.h")).read()
    body = re.search(r"typedef struct drt_adaptive\s*\{(.*?)\}\s*drt_adaptive;", header, re.S).group(1)
    names = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in A._fields_]


# a 3-wavelength table: rw = 1, cy = (1, 2, 1), interval 1 -> N = 4
SPDS = np.array([[1.0, 1.0, 1.0], [1.0, 2.0, 1.0]])


def rule(avgs, vars_, n, max_spp=16, rel_error=0.1, floor=0.0):
    return R.stays_active(SPDS, 0, 1, 1.0, np.array(avgs, dtype=np.float64), np.array(vars_, dtype=np.float64), n, max_spp, rel_error, floor)


def test_an_all_zero_film_stops_at_min_spp():
    counts, ran = R.sample_counts(lambda n: (np.zeros((5, 3)), np.zeros((5, 3))), SPDS, 0, 1, 1.0, 5, 4, 16, 4, 0.01, 0.0)
    assert ran == 1 and (counts == 4).all()


def test_a_nan_stays_active_until_max_spp():
    avgs = np.ones((3, 3)); vars_ = np.zeros((3, 3))
    avgs[0, 1] = vars_[0, 1] = np.nan  # a NaN sample leaves both rows NaN
    vars_[1, 2] = np.nan
    assert list(rule(avgs, vars_, 4)) == [True, True, False]
    assert list(rule(avgs, vars_, 16)) == [False, False, False]
    counts, ran = R.sample_counts(lambda n: (avgs, vars_), SPDS, 0, 1, 1.0, 3, 4, 16, 5, 0.1, 0.0)
    assert list(counts) == [16, 16, 4] and R.rounds(4, 16, 5) == [4, 9, 14, 16] and ran == 4


def test_an_error_exactly_at_the_bound_stops():
    # Y = (1 + 2 + 1) * 1 / 4 = 1; var / (n (n - 1)) = 0.5 / 2 at n = 2 -> sqrt 0.5 in every column -> E = 0.5 exactly
    avgs = np.ones((1, 3)); vars_ = np.full((1, 3), 0.5)
    Y, E = R.luminance_and_error(SPDS, 0, 1, 1.0, avgs, vars_, 2)
    assert Y[0] == 1.0 and E[0] == 0.5
    assert not rule(avgs, vars_, 2, rel_error=0.5)[0]
    assert rule(avgs, vars_, 2, rel_error=np.nextafter(0.5, 0.0))[0]


def test_the_floor_takes_over_for_dim_pixels():
    avgs = np.full((1, 3), 1e-6); vars_ = np.full((1, 3), 0.5)  # Y = 1e-6, E = 0.5
    assert rule(avgs, vars_, 2, rel_error=0.5)[0]
    assert not rule(avgs, vars_, 2, rel_error=0.5, floor=1.0)[0]
    assert rule(avgs, vars_, 2, rel_error=0.5, floor=0.99)[0]


def test_the_sums_run_in_wavelength_order_not_pairwise():
    # a sequential sum and numpy's pairwise one differ on these values; the rule must give the sequential one
    S = 200
    spds = np.ones((2, S))
    rng = np.random.default_rng(5)
    avgs = rng.random((1, S)) * 10.0 ** rng.integers(-8, 8, (1, S))
    Y, _ = R.luminance_and_error(spds, 0, 1, 1.0, avgs, np.zeros((1, S)), 4)
    seq = 0.0
    for v in avgs[0]:
        seq += 1.0 * v * 1.0
    N = 0.0
    for _ in range(S):
        N += 1.0
    assert Y[0] == seq * (1.0 / N)


@pytest.mark.parametrize("env, name", [
    ({"DRT_ADAPTIVE_ERROR": "0"}, "DRT_ADAPTIVE_ERROR"),
    ({"DRT_ADAPTIVE_ERROR": "-1"}, "DRT_ADAPTIVE_ERROR"),
    ({"DRT_ADAPTIVE_ERROR": "nan"}, "DRT_ADAPTIVE_ERROR"),
    ({"DRT_ADAPTIVE_ERROR": "inf"}, "DRT_ADAPTIVE_ERROR"),
    ({"DRT_ADAPTIVE_ERROR": "0.1x"}, "DRT_ADAPTIVE_ERROR"),
    ({"DRT_ADAPTIVE_ERROR": ""}, "DRT_ADAPTIVE_ERROR"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_MIN_SPP": "1"}, "DRT_ADAPTIVE_MIN_SPP"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_MIN_SPP": "100000"}, "DRT_ADAPTIVE_MIN_SPP"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_MIN_SPP": "-4"}, "DRT_ADAPTIVE_MIN_SPP"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_MIN_SPP": "four"}, "DRT_ADAPTIVE_MIN_SPP"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_STEP": "0"}, "DRT_ADAPTIVE_STEP"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_STEP": "2.5"}, "DRT_ADAPTIVE_STEP"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_FLOOR": "-0.5"}, "DRT_ADAPTIVE_FLOOR"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_FLOOR": "nan"}, "DRT_ADAPTIVE_FLOOR"),
    ({"DRT_ADAPTIVE_MIN_SPP": "4"}, "DRT_ADAPTIVE_MIN_SPP"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_CHECKPOINT_SPP": "8"}, "DRT_CHECKPOINT_SPP"),
    ({"DRT_ADAPTIVE_ERROR": "0.1", "DRT_RESUME": "1"}, "DRT_RESUME"),
])
def test_the_host_refuses_bad_adaptive_settings_before_any_device_call(tmp_path, env, name):
    """Exit status nonzero, the variable named on stderr, and no device opened: HIP_VISIBLE_DEVICES hides every device, so a run
    that got as far as the launcher would fail there with the launcher's message instead."""
    cfg = open(os.path.join(REPO, "config.cfg")).read()
    (tmp_path / "config.cfg").write_text(cfg)
    if os.path.isdir(os.path.join(REPO, "scenes")):
        os.symlink(os.path.join(REPO, "scenes"), tmp_path / "scenes")
        os.symlink(os.path.join(REPO, "spectra"), tmp_path / "spectra")
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full.update(env)
    full["HIP_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([BIN, "config.cfg"], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0
    assert name in r.stderr, r.stderr
    assert "HIP launcher" not in r.stderr and "Rendering" not in r.stdout
