"""GPU ORB extraction against the definition-level restatement (oracle/orb_py.py) directly,
without the C++ oracle in between.

Every other extraction test compares the kernels with oracle/orb_ref.cpp, which was written by
the same hands; orb_py.py is numpy from src/ORBextractor.cc and the definitions of FAST-9/16,
strict non-maximum suppression, bilinear interpolation, image moments and rBRIEF
(tests/test_oracle_orb_py.py pins the oracle to it stage by stage on the CPU).

  * pyramid (k_resize_lds, k_pyr_tail): each level of ea.Orb.pyramid against
    orb_py.resize_float of the engine's own previous level. Where the exact bilinear value is
    further than delta from a rounding half the pixel must be its rounding, and everywhere within
    one grey level. delta = orb_py.resize_delta: the reference's 11-bit weights, each of the four
    off by at most 1/4096 on pixels <= 255 (0.2491), plus the float32 rounding of the source
    coordinate on a surface of slope <= 255 per axis (0.0156 below 1024 pixels): 0.2646.
    320x240, 333x257 and 641x481 are the smallest sizes at which every level still holds a
    30-pixel cell; they cover the k_pyr_tail level splits and the unaligned rows.
  * extraction (k_fast_band, k_distribute_mw / k_distribute, k_describe): on the engine's
    pyramid, x / y / size / response / octave / class_id and the order exactly; the angle within
    fastAtan2's accuracy (the bound test_oracle_kat.test_fast_atan2_accuracy asserts) of the
    double-precision atan2 of Python's own moments; the descriptors exactly, given the engine's
    angle, against describe(blur_int(level)).
  * the same through extract_batch_device: three mixed frames in one batch (the quadtree is
    k_distribute_mw up to 32 frames, as in the single call), and 33 frames, the smallest batch
    that takes the one-wave-per-tree k_distribute.
"""
import functools

import numpy as np
import pytest

import eao_accel as ea
import orb_py as op
from test_oracle_kat import FAST_ATAN2_BOUND_DEG
from tools import synth

pytestmark = pytest.mark.gpu

EXACT_FIELDS = ("x", "y", "size", "response", "octave", "class_id")
NFEATURES = [100, 1000, 2000]


@functools.lru_cache(maxsize=None)
def image(kind, w, h):
    img = synth.frame_stream(1)[0][0] if kind == "synth" else synth.orb_case(kind, w, h)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def engine(nfeatures, w, h, max_batch=1):
    return ea.Orb(nfeatures, 1.2, 8, 20, 7, w, h, max_batch=max_batch)


@functools.lru_cache(maxsize=None)
def engine_pyramid(kind, w, h):
    """The engine's pyramid of one image, checked against the definition before anything is
    built on it (test_pyramid_within_derived_bound reports the same check per size)."""
    pyr = engine(1000, w, h).pyramid(image(kind, w, h))
    check_pyramid(pyr, op.level_sizes(w, h)[0])
    return pyr


def check_pyramid(pyr, sizes):
    assert [(p.shape[1], p.shape[0]) for p in pyr] == sizes
    for l in range(1, len(pyr)):
        sh, sw = pyr[l - 1].shape
        dh, dw = pyr[l].shape
        exact = op.resize_float(pyr[l - 1], dw, dh)
        delta = op.resize_delta(sw, sh)
        got = pyr[l].astype(np.float64)
        assert np.abs(got - exact).max() < 1.0, "level %d: more than a grey level off" % l
        clear = np.abs(exact - np.floor(exact) - 0.5) > delta
        bad = clear & (got != np.rint(exact))
        assert not bad.any(), "level %d: %d pixels round the wrong way" % (l, int(bad.sum()))


@functools.lru_cache(maxsize=None)
def definition(kind, w, h, nfeatures):
    """Python's keypoints per level on the engine's pyramid."""
    return op.detect(engine_pyramid(kind, w, h), nfeatures, 20, 7)


@functools.lru_cache(maxsize=None)
def definition_angles(kind, w, h, nfeatures):
    """atan2(m01, m10) in degrees, double precision, of Python's moments at Python's keypoints."""
    umax = op.umax_table()
    return np.array([op.angle_deg(*op.moments(lev, x, y, umax))
                     for lev, d in zip(engine_pyramid(kind, w, h), definition(kind, w, h, nfeatures)) for x, y, _ in d],
                    np.float64)


def check_extraction(kind, w, h, nfeatures, gk, gd):
    pyr = engine_pyramid(kind, w, h)
    det = definition(kind, w, h, nfeatures)
    n = sum(len(d) for d in det)
    assert len(gk) == n, "%d keypoints, the definition gives %d" % (len(gk), n)
    # descriptors and keypoints given the engine's angles
    pk, pd = op.finish(pyr, det, angles=gk["angle"])
    for f in EXACT_FIELDS:
        if not np.array_equal(gk[f], pk[f]):
            bad = np.nonzero(gk[f] != pk[f])[0]
            raise AssertionError("field %s differs at %d keypoints, first %d: %r vs %r" % (
                f, len(bad), bad[0], gk[f][bad[0]], pk[f][bad[0]]))
    assert np.array_equal(gd, pd), "descriptor rows differ: %d of %d" % (int((gd != pd).any(1).sum()), n)
    # the angles against Python's own moments
    diff = np.abs(gk["angle"].astype(np.float64) - definition_angles(kind, w, h, nfeatures))
    diff = np.minimum(diff, 360.0 - diff)
    assert (diff < FAST_ATAN2_BOUND_DEG).all(), "angle off by %.3f deg at keypoint %d" % (diff.max(), diff.argmax())


@pytest.mark.parametrize("kind", ["textured", "noise"])
@pytest.mark.parametrize("w,h", [(320, 240), (333, 257), (641, 481)])
def test_pyramid_within_derived_bound(w, h, kind):
    pyr = engine(1000, w, h).pyramid(image(kind, w, h))
    assert np.array_equal(pyr[0], image(kind, w, h))
    check_pyramid(pyr, op.level_sizes(w, h)[0])


def test_scale_tables_and_quotas_by_definition():
    for nf in NFEATURES:
        orb = engine(nf, 320, 240)
        _, tab = op.level_sizes(320, 240)
        for got, k in zip(orb.scale_tables(), ("scale", "inv_scale", "sigma2", "inv_sigma2")):
            assert np.array_equal(got, tab[k]), k
        assert list(orb.quotas()) == op.quotas(nf)


SINGLE = [(k, w, h) for (w, h) in [(320, 240), (333, 257)] for k in synth.ORB_CASE_KINDS] + [("synth", 640, 480)]


@pytest.mark.parametrize("nfeatures", NFEATURES)
@pytest.mark.parametrize("kind,w,h", SINGLE, ids=["%s-%dx%d" % c for c in SINGLE])
def test_extract_matches_definition(kind, w, h, nfeatures):
    gk, gd = engine(nfeatures, w, h).extract(image(kind, w, h))
    if kind == "flat":
        assert len(gk) == 0
    check_extraction(kind, w, h, nfeatures, gk, gd)


def batch_extract(kinds, nfeatures, w, h):
    import torch
    F = len(kinds)
    dev = torch.device("cuda", 0)
    orb = engine(nfeatures, w, h, F)
    cap = orb.cap
    d_fr = torch.from_numpy(np.stack([image(k, w, h) for k in kinds])).to(dev)
    kps = torch.zeros((F, cap, 28), dtype=torch.uint8, device=dev)
    desc = torch.zeros((F, cap, 32), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    orb.extract_batch_device(d_fr.data_ptr(), F, w, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), cap, None)
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), kps.cpu().numpy().view(ea.KP_DTYPE).reshape(F, cap), desc.cpu().numpy()


def check_batch(kinds, nfeatures, w, h):
    n, hk, hd = batch_extract(kinds, nfeatures, w, h)
    first = {}
    for t, kind in enumerate(kinds):
        assert 0 <= n[t] <= hk.shape[1]
        if kind in first:   # the same image again: the same bytes as its first, checked, occurrence
            t0 = first[kind]
            assert n[t] == n[t0] and np.array_equal(hk[t, :n[t]], hk[t0, :n[t]]) and \
                np.array_equal(hd[t, :n[t]], hd[t0, :n[t]]), "frame %d differs from frame %d (%s)" % (t, t0, kind)
            continue
        first[kind] = t
        try:
            check_extraction(kind, w, h, nfeatures, hk[t, :n[t]], hd[t, :n[t]])
        except AssertionError as e:
            raise AssertionError("frame %d (%s): %s" % (t, kind, e)) from None


@pytest.mark.parametrize("nfeatures", NFEATURES)
@pytest.mark.parametrize("w,h", [(320, 240), (333, 257)])
@pytest.mark.parametrize("kinds", [("noise", "lowcontrast", "checker"), ("blocky", "flat", "textured")], ids=["a", "b"])
def test_batch_of_three_matches_definition(kinds, w, h, nfeatures):
    check_batch(kinds, nfeatures, w, h)


@pytest.mark.parametrize("nfeatures", NFEATURES)
def test_batch_of_33_matches_definition(nfeatures):
    # 33 frames x 8 levels > 256 quadtrees: the one-wave k_distribute, not k_distribute_mw
    kinds = tuple(synth.ORB_CASE_KINDS[i % len(synth.ORB_CASE_KINDS)] for i in range(33))
    check_batch(kinds, nfeatures, 320, 240)
