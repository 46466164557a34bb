"""The ORB oracle (oracle/orb_ref.cpp) against a second, independent restatement
(oracle/orb_py.py), stage by stage, CPU only.

orb_py.py is numpy written from src/ORBextractor.cc and from the definitions of the
primitives (FAST-9/16 response and strict non-maximum suppression, bilinear interpolation, the
Gaussian, image moments), not from orb_ref.cpp. Every stage takes the oracle's output of the
stage before, so a divergence names its stage.

Exact: level sizes, scale tables, quotas, umax; the cell candidates with their order; the
quadtree survivors per level (as a set, then in order); m10 / m01; the 7x7 integer blur; the
descriptor bits given the oracle's angle and blur; every final keypoint field but the angle.

Bounded, each bound derived and none fitted to the code under test:
  * pyramid: level l is compared with resize_float of the ORACLE's level l-1. The reference's
    cv::resize interpolates with 11-bit weights. Each of the four weights (two per axis) is
    off by at most 1/4096, which moves the interpolated value of pixels <= 255 by at most
    255 * (4/4096 + 4/4096^2) = 0.2491; the source coordinate is rounded to float32 first
    (half an ulp of a number below the image size, at most 2^-15 below 1024) on a surface of
    slope <= 255 per axis: 2 * 255 * 2^-15 = 0.0156 more. delta = 0.2646 at these sizes
    (orb_py.resize_delta). Wherever the exact value is further than delta from a rounding half
    the oracle's pixel must be its rounding; everywhere it must be within 1 grey level.
    Measured for the oracle alone on these images: a pixel rounded the other way lies at most
    0.078 from the half.
  * angle: the oracle's fastAtan2 angle against atan2(m01, m10) in double precision, within
    the accuracy test_oracle_kat.test_fast_atan2_accuracy asserts for fastAtan2 (0.3 degrees;
    measured 0.0096).
  * blur_float: the 8-bit taps 18 34 49 55 49 34 18 / 256 against the true Gaussian, within
    255 * sum |k_i k_j / 65536 - g_i g_j| + 0.5 (orb_py.blur_bound, 3.07 grey levels; measured
    2.12).

Images (tools/synth.orb_case): textured, noise (quotas filled), lowcontrast (the minThFAST
pass), flat, blocky (plateaus under the strict NMS), checker (equal responses inside a node)
at 320x240, 333x257 and 641x481, and one 640x480 frame of the bench stream; 100 features reach
the size-sorted last expansion and Q14, 2000 on 320x240 run the quadtree out of candidates.
"""
import functools
import math

import numpy as np
import pytest

import orb_py as op
import pyoracle as orc
from test_oracle_kat import FAST_ATAN2_BOUND_DEG
from tools import synth

SIZES = [(320, 240), (333, 257), (641, 481)]
CASES = [(k, w, h) for (w, h) in SIZES for k in synth.ORB_CASE_KINDS] + [("synth", 640, 480)]
NFEATURES = [100, 1000, 2000]
case_ids = ["%s-%dx%d" % c for c in CASES]
EXACT_FIELDS = ("x", "y", "size", "response", "octave", "class_id")


@functools.lru_cache(maxsize=None)
def image(kind, w, h):
    img = synth.frame_stream(1)[0][0] if kind == "synth" else synth.orb_case(kind, w, h)
    assert img.shape == (h, w) and img.dtype == np.uint8
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def oracle_pyramid(case):
    return orc.pyramid(image(*case))


@functools.lru_cache(maxsize=None)
def oracle_candidates(case):
    return [orc.level_candidates(lev) for lev in oracle_pyramid(case)]


def as_tuples(c):
    assert np.array_equal(c["x"], np.rint(c["x"])) and np.array_equal(c["y"], np.rint(c["y"]))
    return list(zip(c["x"].astype(int).tolist(), c["y"].astype(int).tolist(), c["response"].astype(int).tolist()))


def borders(lev):
    rows, cols = lev.shape
    return 16, cols - 16, 16, rows - 16       # EDGE_THRESHOLD - 3, ORBextractor.cc:773-776


@functools.lru_cache(maxsize=None)
def oracle_selection(case, nfeatures):
    """Per level: the oracle's quadtree on the oracle's candidates -> level coordinates."""
    q = orc.orb_params(nfeatures)["quotas"]
    out = []
    for l, (lev, c) in enumerate(zip(oracle_pyramid(case), oracle_candidates(case))):
        sel = orc.distribute(c, *borders(lev), int(q[l]))
        out.append((sel, c["x"][sel] + 16, c["y"][sel] + 16, c["response"][sel]))
    return out


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("w,h", SIZES + [(640, 480), (1920, 1080)])
def test_level_sizes_and_tables(w, h):
    sizes, tab = op.level_sizes(w, h)
    assert sizes == orc.level_sizes(w, h)
    p = orc.orb_params()
    for k in ("scale", "inv_scale", "sigma2", "inv_sigma2"):
        assert tab[k].dtype == np.float32 and np.array_equal(tab[k], p[k]), k


@pytest.mark.parametrize("nfeatures", NFEATURES + [4000])
def test_quotas_and_umax(nfeatures):
    assert op.quotas(nfeatures) == orc.orb_params(nfeatures)["quotas"].tolist()
    assert op.umax_table() == orc.orb_params()["umax"].tolist()
    assert op.KP_DTYPE == orc.KP_DTYPE


# ------------------------------------------------------------------ pyramid
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_pyramid_within_derived_bound(case):
    pyr = oracle_pyramid(case)
    worst = 0.0
    for l in range(1, len(pyr)):
        sh, sw = pyr[l - 1].shape
        dh, dw = pyr[l].shape
        exact = op.resize_float(pyr[l - 1], dw, dh)
        delta = op.resize_delta(sw, sh)
        assert 0.249 < delta < 0.30
        got = pyr[l].astype(np.float64)
        assert np.abs(got - exact).max() < 1.0, "level %d: more than a grey level off" % l
        frac = exact - np.floor(exact)
        clear = np.abs(frac - 0.5) > delta
        bad = clear & (got != np.rint(exact))
        assert not bad.any(), "level %d: %d pixels round the wrong way" % (l, int(bad.sum()))
        wrong = got != np.floor(exact + 0.5)
        if wrong.any():
            worst = max(worst, float(np.abs(frac - 0.5)[wrong].max()))
    print("largest distance from the half of a pixel rounded the other way: %.4f" % worst)


# ------------------------------------------------------------------ FAST cells
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_cell_candidates_exact_in_order(case):
    kind = case[0]
    pyr = oracle_pyramid(case)
    for l, (lev, c) in enumerate(zip(pyr, oracle_candidates(case))):
        mine = op.fast_cells(lev, 20, 7)
        theirs = as_tuples(c)
        assert set(mine) == set(theirs), "level %d: %d / %d only on one side" % (
            l, len(set(mine) - set(theirs)), len(set(theirs) - set(mine)))
        assert mine == theirs, "level %d: same candidates, another order" % l
        assert (c["size"] == 7).all() and (c["angle"] == -1).all() and (c["octave"] == 0).all()
    # each image kind does what it is there for
    lev0 = as_tuples(oracle_candidates(case)[0])
    if kind == "flat":
        assert not lev0
    if kind == "lowcontrast":   # most of the candidates come from cells that fell back to minThFAST
        assert len(lev0) > 2 * len(op.fast_cells(pyr[0], 20, 20)) > 0
    if kind == "checker":       # one response shared by most candidates
        resp = np.array([r for _, _, r in lev0])
        assert (resp == np.bincount(resp).argmax()).mean() > 0.5


# ------------------------------------------------------------------ quadtree
@pytest.mark.parametrize("nfeatures", NFEATURES)
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_quadtree_survivors(case, nfeatures):
    kind, w, h = case
    q = op.quotas(nfeatures)
    total = 0
    for l, (lev, c) in enumerate(zip(oracle_pyramid(case), oracle_candidates(case))):
        theirs = oracle_selection(case, nfeatures)[l][0].tolist()
        mine = op.distribute(as_tuples(c), *borders(lev), q[l])
        assert set(mine) == set(theirs), "level %d: %d / %d survivors only on one side" % (
            l, len(set(mine) - set(theirs)), len(set(theirs) - set(mine)))
        assert mine == theirs, "level %d: same survivors, another order" % l
        total += len(mine)
        if kind == "noise" and nfeatures == 100:
            assert len(mine) >= q[l]                       # dense corners fill every quota
    if (w, h) == (320, 240) and nfeatures == 2000:
        assert total < nfeatures                           # the quadtree runs out of candidates


# ------------------------------------------------------------------ orientation
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_moments_exact_and_angle_within_fastatan2_bound(case):
    umax = op.umax_table()
    worst = 0.0
    for lev, (_, x, y, _) in zip(oracle_pyramid(case), oracle_selection(case, 1000)):
        m10, m01, ang = orc.orientation(lev, x, y)
        for i in range(len(x)):
            pm10, pm01 = op.moments(lev, int(x[i]), int(y[i]), umax)
            assert (pm10, pm01) == (int(m10[i]), int(m01[i])), (int(x[i]), int(y[i]))
            d = abs(float(ang[i]) - op.angle_deg(pm10, pm01))
            d = min(d, 360.0 - d)
            worst = max(worst, d)
            assert d < FAST_ATAN2_BOUND_DEG, (pm10, pm01, float(ang[i]))
    print("largest |fastAtan2 - atan2|: %.4f deg" % worst)


# ------------------------------------------------------------------ blur
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_blur_exact_and_gaussian_within_kernel_bound(case):
    bound = op.blur_bound()
    assert 0.5 < bound < 4.0
    worst = 0.0
    for lev in oracle_pyramid(case):
        theirs = orc.blur7(lev)
        assert np.array_equal(op.blur_int(lev), theirs)
        err = float(np.abs(theirs.astype(np.float64) - op.blur_float(lev)).max())
        worst = max(worst, err)
        assert err <= bound
    print("largest |blur7 - Gaussian|: %.3f of a bound of %.3f" % (worst, bound))


# ------------------------------------------------------------------ descriptors, composition
@pytest.mark.parametrize("nfeatures", NFEATURES)
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_descriptors_and_final_keypoints(case, nfeatures):
    img = image(*case)
    pyr = oracle_pyramid(case)
    ok, od = orc.extract(img, nfeatures)
    # the descriptor bits alone, given the oracle's blur and angle, level by level; the oracle's
    # staged entry points compose to its own extraction
    o = 0
    for lev, (_, x, y, _) in zip(pyr, oracle_selection(case, nfeatures)):
        n = len(x)
        if n == 0:
            continue
        blurred = orc.blur7(lev)
        ang = orc.orientation(lev, x, y)[2]
        assert np.array_equal(ang, ok["angle"][o:o + n])
        theirs = orc.describe(blurred, x, y, ang)
        assert np.array_equal(theirs, od[o:o + n])
        mine = op.describe(blurred, x, y, ang)
        assert np.array_equal(mine, theirs), "descriptor rows differ: %d of %d" % (int((mine != theirs).any(1).sum()), n)
        o += n
    assert o == len(ok)
    # the whole Python extraction on the oracle's pyramid and angles
    # (extract = finish(detect): detected once here, finished with either set of angles)
    det = op.detect(pyr, nfeatures, 20, 7)
    assert sum(len(d) for d in det) == len(ok), (sum(len(d) for d in det), len(ok))
    pk, pd = op.finish(pyr, det, angles=ok["angle"])
    for f in EXACT_FIELDS:
        assert np.array_equal(pk[f], ok[f]), f
    assert np.array_equal(pd, od)
    if case[1] < 400 and nfeatures == 1000:   # the one-call form is the same composition
        ek, ed = op.extract(img, nfeatures, 20, 7, pyramid=pyr, angles=ok["angle"])
        assert np.array_equal(ek, pk) and np.array_equal(ed, pd)
    # and with its own angles: the same keypoints, angles within the fastAtan2 bound
    pk2, _ = op.finish(pyr, det)
    d = np.abs(pk2["angle"].astype(np.float64) - ok["angle"])
    assert len(pk2) == len(ok) and (np.minimum(d, 360 - d) < FAST_ATAN2_BOUND_DEG).all()
