"""The isolation forest restatement (oracle/iforest_ref.h, behind orc.iforest) against the
reference's own include/isolation_forest.h, CPU only.

The header uses only the standard library, so it runs here as it is: oracle/iforest_ref_driver.cpp
(ours) calls Build(50, 12345, data, sample) and GetAnomalyScores, as
Object_Map::IsolationForestDeleteOutliers does (src/Object.cc:1202-1309), and `make -C oracle ref`
compiles it against the header in the reference tree into oracle/_ref/. The test makes that
binary when the tree is present and skips only when there is neither a tree nor a binary.
Scores must be equal bit for bit: both sides draw from the same mt19937 / uniform_int /
uniform_real / shuffle streams, sort the same values and sum the same path lengths in the same
order. (NaN scores -- one sampled point gives c(1) = 0 and 0/0 -- must be NaN on both sides.)
"""
import struct
import subprocess

import numpy as np
import pytest

import pyoracle as orc

SIZES = [2, 3, 4, 5, 7, 8, 16, 31, 33, 100, 257, 640, 1024, 2049, 4097]
KINDS = ["gaussian", "lattice", "duplicates", "one_point", "const_dim"]
TREES, SEED = 50, 12345


def cloud(kind, n):
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n)
    if kind == "gaussian":      # an object's map points, a few far outliers
        p = rng.normal([0, 0, 2], [0.05, 0.08, 0.03], (n, 3))
        p[: n // 20] += rng.uniform(-0.5, 0.5, (n // 20, 3))
    elif kind == "lattice":     # few distinct values per axis: ties in every sort and split
        p = rng.integers(0, 4, (n, 3)) * 0.25
    elif kind == "duplicates":  # every point present twice or more
        p = np.repeat(rng.normal(0, 1, ((n + 1) // 2, 3)), 2, axis=0)[:n]
    elif kind == "one_point":   # min == max on every axis: the root is a leaf
        p = np.tile([[0.3, -1.5, 2.0]], (n, 1))
    else:                       # a constant dimension: leaves whenever it is drawn
        p = rng.normal(0, 1, (n, 3))
        p[:, 1] = 0.75
    return np.ascontiguousarray(p, np.float32)


def record(pts, sample):
    return struct.pack("<iIII", len(pts), TREES, SEED, sample) + pts.tobytes()


def run_driver(driver, recs, sizes):
    out = subprocess.run([driver], input=b"".join(recs), stdout=subprocess.PIPE, check=True).stdout
    res, o = [], 0
    for n in sizes:
        (ok,) = struct.unpack_from("<i", out, o)
        o += 4
        if ok:
            res.append(np.frombuffer(out, np.float64, n, o).copy())
            o += 8 * n
        else:
            res.append(None)
    assert o == len(out)
    return res


@pytest.fixture(scope="module")
def driver():
    d = orc.build_ref()
    if d is None:
        pytest.skip("neither the reference tree nor a built oracle/_ref/iforest_ref_driver")
    return d


@pytest.fixture(scope="module")
def reference_scores(driver):
    """Every case through one run of the driver: {(kind, n, sample): scores or None}."""
    keys = [(k, n, s) for k in KINDS for n in SIZES for s in (n // 2, n // 3)]
    res = run_driver(driver, [record(cloud(k, n), s) for k, n, s in keys], [n for _, n, _ in keys])
    return dict(zip(keys, res))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_scores_equal_reference_header(reference_scores, kind, n):
    pts = cloud(kind, n)
    for sample in (n // 2, n // 3):
        ref = reference_scores[(kind, n, sample)]
        ok, got = orc.iforest_try(pts, TREES, SEED, sample)
        if sample == 0:  # n = 2 with n / 3: Build refuses an empty sample
            assert ref is None and not ok
            continue
        assert ok and ref is not None, (kind, n, sample)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (kind, n, sample)
        m = ~np.isnan(ref)
        assert np.array_equal(got[m].view(np.uint64), ref[m].view(np.uint64)), \
            "%s n=%d sample=%d: %d scores differ" % (kind, n, sample, int((got[m] != ref[m]).sum()))


@pytest.mark.parametrize("n", [1, 2, 100])
def test_both_refuse_bad_sample_sizes(driver, n):
    pts = cloud("gaussian", n)
    for sample in (0, n + 1, 4 * n):
        (ref,) = run_driver(driver, [record(pts, sample)], [n])
        ok, _ = orc.iforest_try(pts, TREES, SEED, sample)
        assert ref is None and not ok, (n, sample)
    (ref,) = run_driver(driver, [record(pts, n)], [n])      # sample == n is the largest allowed
    ok, got = orc.iforest_try(pts, TREES, SEED, n)
    assert ok and ref is not None and np.array_equal(got, ref, equal_nan=True)
