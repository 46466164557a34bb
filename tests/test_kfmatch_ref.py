"""tools/kfmatch_ref.py, the checker of the keyframe matchers (Fuse, Fuse with a Sim3, SearchBySim3,
SearchForTriangulation; reference src/ORBmatcher.cc:140-157, 657-1326), checked on its own. CPU test.

1. brute force: the projection searches equal a search over ALL keyframe keypoints with the same gates
   (ties broken by the (ix, iy, index) walk order); the triangulation search equals a dense loop over all
   (idx1, idx2) sharing a node (the last one winning on equal distance);
2. hand cases of 2-4 keypoints, each answer worked out from the reference's text in the comments;
3. the scenes tests/test_gpu_kfmatch.py uses exercise every gate (a vacuous fixture fails here).
"""
import math

import numpy as np
import pytest

import eao_accel as ea
import pyoracle as orc
from tools import kfmatch_ref as R
from tools import synth

f32 = np.float32
CAM = ea.camera()
SF, SIG, INV, LOGSF = synth.level_tables()
# hand cases: binary-fraction intrinsics, so the projections below are exact in float
HC = ea.Camera(640, 480, 512.0, 512.0, 320.0, 240.0)
EYE = np.eye(4, dtype=np.float32)


def _fuse_args(s, th):
    mp = s["mp"]
    return (CAM, s["T"], th, mp["valid"], mp["pos"], mp["normal"], mp["mind"], mp["maxd"], mp["desc"], LOGSF,
            s["kps"], s["desc"], SF)


def _sim3_args(q, th):
    a, b = q["side1"], q["side2"]
    return (CAM, q["T1"], q["T2"], q["s12"], q["R12"], q["t12"], th, a["kps"], a["desc"], a["valid"], a["pos"],
            a["mind"], a["maxd"], a["mp_desc"], a["already"], b["kps"], b["desc"], b["valid"], b["pos"], b["mind"],
            b["maxd"], b["mp_desc"], b["already"], LOGSF, SF)


@pytest.fixture(scope="module")
def fuse_scene():
    return synth.fuse_scene(0)


@pytest.fixture(scope="module")
def sim3_scene():
    return synth.sim3_scene(0)


def _tri(voc, levelsup, seed=0):
    g = synth.triangulation_scene(voc, seed)
    fv1, fv2 = orc.bow_transform(voc, g["desc1"], levelsup)[2:], orc.bow_transform(voc, g["desc2"], levelsup)[2:]
    return g, fv1, fv2


def _tri_args(g, fv1, fv2, check_ori):
    return (CAM, g["F12"], g["Ow1"], g["T2"], check_ori, g["kps1"], g["desc1"], g["has1"], fv1, g["kps2"], g["desc2"],
            g["has2"], fv2, SF, SIG)


@pytest.fixture(scope="module")
def tri_scenes():
    return {"orb": _tri(synth.vocabulary(K=10, L=6), 4), "coarse": _tri(synth.vocabulary(K=10, L=4), 3)}


# ---------------------------------------------------------------- 1. brute force
class _Brute:
    """every keypoint of the keyframe against a point, without the grid's cell lists: its cell
    (Frame::PosInGrid) inside the cell window, inside the square, the octave gate, the chi-square gate;
    the smallest (distance, ix, iy, index)."""

    def __init__(self, cam, kps, desc):
        self.g = g = R.KeyFrameGrid(cam, kps)
        self.desc = desc
        self.cell = [(R._c_round(f32(f32(g.x[j] - g.minX) * g.invW)), R._c_round(f32(f32(g.y[j] - g.minY) * g.invH)))
                     for j in range(len(kps))]
        self.xy = np.stack([kps["x"], kps["y"]], 1).astype(np.float64)

    def search(self, geo, mdesc, inv_sigma2, th_accept):
        g = self.g
        u, v, r, lvl = geo
        w = g.cell_range(u, v, r)
        best = None
        # a loose square around the exact one only spares the exact tests on keypoints far away
        near = np.nonzero((np.abs(self.xy[:, 0] - float(u)) < float(r) + 1) &
                          (np.abs(self.xy[:, 1] - float(v)) < float(r) + 1))[0]
        for j in near:
            ix, iy = self.cell[j]
            if w is None or not (w[0] <= ix <= w[1] and w[2] <= iy <= w[3]):
                continue
            if not (abs(f32(g.x[j] - u)) < r and abs(f32(g.y[j] - v)) < r):
                continue
            if not (lvl - 1 <= g.octave[j] <= lvl):
                continue
            if inv_sigma2 is not None:
                ex, ey = f32(u - g.x[j]), f32(v - g.y[j])
                if float(f32(f32(f32(ex * ex) + f32(ey * ey)) * inv_sigma2[g.octave[j]])) > 5.99:
                    continue
            key = (R.descriptor_distance(mdesc, self.desc[j]), ix, iy, int(j))
            if best is None or key < best:
                best = key
        if best is None:
            return -1, 256
        return (best[3] if best[0] <= th_accept else -1), best[0]


@pytest.mark.parametrize("th", [3.0, 20.0])
def test_fuse_equals_brute_force(fuse_scene, th):
    s = fuse_scene
    geo = {}
    nf, bi, bd = R.fuse(*_fuse_args(s, th), INV, geo=geo)
    assert nf == int((bi >= 0).sum()) and len(geo) > 400
    b = _Brute(CAM, s["kps"], s["desc"])
    for i in range(len(bi)):
        want = b.search(geo[i], s["mp"]["desc"][i], INV, 50) if i in geo else (-1, 256)
        assert (bi[i], bd[i]) == want, i


def test_fuse_sim3_equals_brute_force(fuse_scene):
    s = fuse_scene
    S = EYE.copy()
    S[:3] = s["T"][:3] * f32(1.7)
    a = list(_fuse_args(s, 4.0))
    a[1] = S
    geo = {}
    nf, bi, bd = R.fuse_sim3(*a, geo=geo)
    assert nf == int((bi >= 0).sum()) and nf > 100
    b = _Brute(CAM, s["kps"], s["desc"])
    for i in range(len(bi)):
        want = b.search(geo[i], s["mp"]["desc"][i], None, 50) if i in geo else (-1, 256)
        assert (bi[i], bd[i]) == want, i


def test_sim3_halves_equal_brute_force(sim3_scene):
    q = sim3_scene
    a, b = q["side1"], q["side2"]
    sR12, sR21, t21 = R.sim3_transforms(q["s12"], q["R12"], q["t12"])
    for own, other, T, sR, t in ((a, b, q["T1"], sR21, t21), (b, a, q["T2"], sR12, q["t12"])):
        geo = {}
        vn = R.sim3_half(CAM, T, sR, t, 7.5, own["valid"], own["already"], own["pos"], own["mind"], own["maxd"],
                         own["mp_desc"], LOGSF, other["kps"], other["desc"], SF, geo=geo)
        assert (vn >= 0).sum() > 100
        br = _Brute(CAM, other["kps"], other["desc"])
        for i in range(len(vn)):
            want = br.search(geo[i], own["mp_desc"][i], None, 100)[0] if i in geo else -1
            assert vn[i] == want, i


def _brute_triangulation(g, fv1, fv2):
    """dense: every (idx1, idx2) without map points whose features sit in the same node; the candidates
    that pass the distance bar and the two epipolar gates; the smallest distance, the last position in
    the node's list on ties."""
    node1 = {int(f): int(fv1[0][k]) for k in range(len(fv1[0])) for f in fv1[2][fv1[1][k]:fv1[1][k + 1]]}
    pos2 = {int(f): (int(fv2[0][k]), p) for k in range(len(fv2[0]))
            for p, f in enumerate(fv2[2][fv2[1][k]:fv2[1][k + 1]])}
    T2 = np.asarray(g["T2"], f32)
    C2 = R._gemm3(T2[:3, :3], T2[:3, 3], g["Ow1"])
    invz = f32(f32(1.0) / C2[2])
    ex = f32(f32(f32(f32(CAM.fx) * C2[0]) * invz) + f32(CAM.cx))
    ey = f32(f32(f32(f32(CAM.fy) * C2[1]) * invz) + f32(CAM.cy))
    k1, k2 = g["kps1"], g["kps2"]
    out = np.full(len(k1), -1, np.int32)
    for i1 in range(len(k1)):
        if g["has1"][i1] or i1 not in node1:
            continue
        best = None
        for i2 in range(len(k2)):
            if g["has2"][i2] or i2 not in pos2 or pos2[i2][0] != node1[i1]:
                continue
            d = R.descriptor_distance(g["desc1"][i1], g["desc2"][i2])
            if d > 50:
                continue
            o = int(k2["octave"][i2])
            dx, dy = f32(ex - k2["x"][i2]), f32(ey - k2["y"][i2])
            if f32(f32(dx * dx) + f32(dy * dy)) < f32(f32(100) * SF[o]):
                continue
            if not R.check_dist_epipolar_line(k1["x"][i1], k1["y"][i1], k2["x"][i2], k2["y"][i2], o, g["F12"], SIG):
                continue
            key = (d, -pos2[i2][1])
            if best is None or key < best[0]:
                best = (key, i2)
        if best is not None:
            out[i1] = best[1]
    return out


@pytest.mark.parametrize("which", ["orb", "coarse"])
def test_triangulation_equals_dense_loop(tri_scenes, which):
    g, fv1, fv2 = tri_scenes[which]
    n, m = R.search_for_triangulation(*_tri_args(g, fv1, fv2, 0))
    want = _brute_triangulation(g, fv1, fv2)
    assert np.array_equal(m, want) and n == int((want >= 0).sum()) and n > 100


# ---------------------------------------------------------------- 2. hand cases
def _kps(rows):
    k = np.zeros(len(rows), synth._KP_DT)
    for i, (x, y, o) in enumerate(rows):
        k[i]["x"], k[i]["y"], k[i]["octave"] = x, y, o
    return k


def _desc(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(d, nbits):
    """d with exactly nbits distinct bits flipped: Hamming distance nbits."""
    out = d.copy()
    for b in range(nbits):
        out[b >> 3] ^= 1 << (b & 7)
    return out


def _pt(u, v, z=2.0):
    """the camera-frame (= world, identity pose) point that HC projects to (u, v): exact for the
    binary-fraction offsets used below."""
    return [(u - 320.0) / 512.0 * z, (v - 240.0) / 512.0 * z, z]


def _hand_fuse(points, kps, kdesc, mdesc, level=0, sf=SF, logsf=LOGSF, inv=INV, maxd=None, counters=None, th=3.0):
    """Fuse at the identity pose (Ow = 0, PO = P): normals along the viewing ray, the distance range put
    half a level under `level` so PredictScale gives it."""
    P = np.array(points, np.float32)
    d = np.linalg.norm(P.astype(np.float64), axis=1)
    nrm = (P / np.maximum(d, 1e-9)[:, None]).astype(np.float32)
    mx = (d * float(sf[1]) ** (level - 0.5)).astype(np.float32) if maxd is None else np.array(maxd, np.float32)
    mn = (np.full(len(P), 0.01)).astype(np.float32)
    return R.fuse(HC, EYE, th, np.ones(len(P), np.uint8), P, nrm, mn, mx, mdesc, logsf, kps, kdesc, sf, inv, counters)


def test_hand_fuse_tie_takes_first_in_walk_order():
    # The point projects to u = 325, v = 240, level 0, radius 3. Keypoint 0 at x = 326 lies in cell
    # round(32.6) = 33, keypoint 1 at x = 324 in cell round(32.4) = 32; both are inside the square, both
    # have the same descriptor. GetFeaturesInArea walks ix = 32 first (KeyFrame.cc:633), `dist < bestDist`
    # (ORBmatcher.cc:945) keeps the first: keypoint 1, although its index is the larger.
    d = _desc(1)
    nf, bi, bd = _hand_fuse([_pt(325, 240)], _kps([(326, 240, 0), (324, 240, 0)]), np.repeat(d, 2, 0), d)
    assert (nf, bi[0], bd[0]) == (1, 1, 0)
    # both in one cell (x = 324, 323 -> cell 32): index order inside the cell, keypoint 0
    nf, bi, bd = _hand_fuse([_pt(325, 240)], _kps([(324, 240, 0), (323, 240, 0)]), np.repeat(d, 2, 0), d)
    assert (nf, bi[0]) == (1, 0)


def test_hand_image_bounds_and_depth():
    d = _desc(1)
    k = _kps([(634, 240, 0)])  # the last grid column: round(63.4) = 63 (x >= 635 falls outside the grid)
    # x / z = 0.625 exactly, u = 512 * 0.625 + 320 = 640 = w: IsInImage needs u < mnMaxX (KeyFrame.cc:655)
    c = {}
    assert _hand_fuse([[1.25, 0.0, 2.0]], k, d, d, counters=c)[0] == 0 and c == {"image_bounds": 1}
    # five pixel columns further in (u = 635) the point passes and finds the keypoint 1 px away
    assert _hand_fuse([_pt(635, 240)], k, d, d)[1][0] == 0
    # z < 0 (ORBmatcher.cc:855): rejected before the projection
    c = {}
    assert _hand_fuse([[0.0, 0.0, -2.0]], _kps([(320, 240, 0)]), d, d, counters=c)[0] == 0 and c == {"depth_sign": 1}


def test_hand_predicted_level_is_clamped():
    sf, sig, inv, logsf = synth.level_tables(8, 1.1)
    d = _desc(1)
    # dist3D = 2, mfMaxDistance = 1.8: inside the range (1.2 * 1.8 >= 2), ratio 0.9,
    # log(0.9) / log(1.1) = -1.105, ceil = -1 -> clamped to 0: radius 3 * sf[0] = 3 and octaves [-1, 0], so
    # the level-0 keypoint 2 px away is found (unclamped, no octave in [-2, -1] exists)
    nf, bi, _ = _hand_fuse([_pt(320, 240)], _kps([(322, 240, 0)]), d, d, sf=sf, logsf=logsf, inv=inv, maxd=[1.8])
    assert (nf, bi[0]) == (1, 0)
    assert math.ceil(math.log(0.9) / math.log(1.1)) == -1
    # mfMaxDistance = 2 * 1.1^9.5: level 10 -> clamped to nlevels - 1 = 7: octaves [6, 7] pass, 5 does not
    mx = [2.0 * 1.1 ** 9.5]
    assert _hand_fuse([_pt(320, 240)], _kps([(321, 240, 7)]), d, d, sf=sf, logsf=logsf, inv=inv, maxd=mx)[1][0] == 0
    assert _hand_fuse([_pt(320, 240)], _kps([(321, 240, 5)]), d, d, sf=sf, logsf=logsf, inv=inv, maxd=mx)[1][0] == -1


def test_hand_octave_gate_and_distance_bar():
    d = _desc(1)
    # predicted level 3: octaves 2 and 3 pass (ORBmatcher.cc:911), 4 does not
    c = {}
    nf, bi, bd = _hand_fuse([_pt(320, 240)], _kps([(321, 240, 4)]), d, d, level=3, counters=c)
    assert (nf, bi[0], bd[0]) == (0, -1, 256) and c == {"octave": 1}
    assert _hand_fuse([_pt(320, 240)], _kps([(321, 240, 2)]), d, d, level=3)[1][0] == 0
    # bestDist <= TH_LOW (ORBmatcher.cc:951): 50 is accepted, 51 is not (its distance is still reported)
    k = _kps([(321, 240, 0)])
    nf, bi, bd = _hand_fuse([_pt(320, 240)], k, d, _flip(d[0], 50)[None])
    assert (nf, bi[0], bd[0]) == (1, 0, 50)
    nf, bi, bd = _hand_fuse([_pt(320, 240)], k, d, _flip(d[0], 51)[None])
    assert (nf, bi[0], bd[0]) == (0, -1, 51)


def _hand_sim3(k1, d1, pos1, md1, k2, d2, pos2, md2, valid2=None, counters=None):
    """identity poses and identity Sim3: a point's camera coordinates are its world coordinates in both
    keyframes; distance range around level 0."""
    def side(pos):
        P = np.array(pos, np.float32).reshape(-1, 3)
        dd = np.linalg.norm(P.astype(np.float64), axis=1)
        return P, np.full(len(P), 0.01, np.float32), (dd * 1.2 ** -0.5).astype(np.float32)
    P1, mn1, mx1 = side(pos1)
    P2, mn2, mx2 = side(pos2)
    v2 = np.ones(len(P2), np.uint8) if valid2 is None else np.array(valid2, np.uint8)
    z = lambda n: np.zeros(n, np.uint8)
    return R.search_by_sim3(HC, EYE, EYE, 1.0, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 7.5, k1, d1,
                            np.ones(len(P1), np.uint8), P1, mn1, mx1, md1, z(len(P1)), k2, d2, v2, P2, mn2, mx2, md2,
                            z(len(P2)), LOGSF, SF, counters)


def test_hand_sim3_distance_bar_and_agreement():
    d = _desc(2)
    A, B = d[0:1], d[1:2]
    k = _kps([(320, 240, 0)])
    # one feature per keyframe, the same point: both halves find each other. bestDist <= TH_HIGH
    # (ORBmatcher.cc:1221, :1300): a descriptor 100 bits away is accepted, 101 is not
    far = _flip(A[0], 100)[None]
    assert _hand_sim3(k, A, [_pt(320, 240)], far, k, A, [_pt(320, 240)], far)[0] == 1
    far = _flip(A[0], 101)[None]
    assert _hand_sim3(k, A, [_pt(320, 240)], far, k, A, [_pt(320, 240)], far)[0] == 0
    # agreement (:1306-1323): KF1 feature 0's point lands on KF2 feature 0 (vnMatch1[0] = 0), but KF2
    # feature 0's point projects between KF1's two features and carries the descriptor of feature 1:
    # vnMatch2[0] = 1 != 0, so no match although each half found one
    k1 = _kps([(320, 240, 0), (322, 240, 0)])
    c, halves = {}, []
    a = _hand_sim3(k1, np.concatenate([A, B]), [_pt(320, 240), _pt(400, 100)], np.concatenate([A, _desc(1, 9)]), k, A,
                   [_pt(321, 240)], B, counters=c)
    assert a[0] == 0 and list(a[1]) == [-1, -1] and c.get("sim3_agreement") == 1


# the epipolar lines of F = [[0,0,0],[0,0,1],[0,-1,0]] are horizontal: l = x1' F = [0, -1, y1], so
# num = y1 - y2, den = 1 and dsqr = (y1 - y2)^2 (ORBmatcher.cc:143-156)
F_HORIZONTAL = np.array([[0, 0, 0], [0, 0, 1], [0, -1, 0]], np.float32)


def _hand_tri(k1, d1, k2, d2, feats2, F=F_HORIZONTAL, t2=(-0.5, 0.0, 0.25), check_ori=0, counters=None):
    """one vocabulary node (id 5) holding every feature; camera 1 at the origin, so the epipole is the
    projection of t2w."""
    T2 = EYE.copy()
    T2[:3, 3] = t2
    fv1 = (np.array([5], np.int32), np.array([0, len(k1)], np.int32), np.arange(len(k1), dtype=np.int32))
    fv2 = (np.array([5], np.int32), np.array([0, len(feats2)], np.int32), np.array(feats2, np.int32))
    none1, none2 = np.zeros(len(k1), np.uint8), np.zeros(len(k2), np.uint8)
    return R.search_for_triangulation(HC, F, np.zeros(3, np.float32), T2, check_ori, k1, d1, none1, fv1, k2, d2, none2,
                                      fv2, SF, SIG, counters)


def test_hand_triangulation_tie_takes_last():
    d = _desc(1)
    k1 = _kps([(100, 200, 0)])
    k2 = _kps([(150, 200, 0), (250, 200, 0)])
    d2 = np.repeat(d, 2, 0)
    # both KF2 features lie on the line y = 200 with distance 0; `dist > bestDist -> continue`
    # (ORBmatcher.cc:734) lets an equal distance through, so the later one in the node's list replaces
    n, m = _hand_tri(k1, d, k2, d2, [0, 1])
    assert (n, m[0]) == (1, 1)
    n, m = _hand_tri(k1, d, k2, d2, [1, 0])
    assert (n, m[0]) == (1, 0)
    # two pixels off the line at octave 0: dsqr = 4 > 3.84 * sigma2[0] = 3.84 -> rejected
    c = {}
    assert _hand_tri(k1, d, _kps([(150, 202, 0)]), d, [0], counters=c)[0] == 0 and c == {"epipolar_distance": 1}
    assert _hand_tri(k1, d, _kps([(150, 201.5, 0)]), d, [0])[0] == 1  # 2.25 < 3.84


def test_hand_triangulation_zero_f_and_epipole():
    d = _desc(1)
    k1 = _kps([(100, 240, 0)])
    # F12 = 0: a = b = 0, den == 0 -> CheckDistEpipolarLine returns false (:151-152): no match
    assert _hand_tri(k1, d, _kps([(150, 240, 0)]), d, [0], F=np.zeros((3, 3), np.float32))[0] == 0
    # t2w = (0, 0, 1): C2 = (0, 0, 1), the epipole is (cx, cy) = (320, 240). A KF2 feature there has
    # distex^2 + distey^2 = 0 < 100 * scale_factors[0] (:741-743): skipped although it is on the line;
    # the one 80 px along the line is taken. 9 px away (81 < 100) is still too near, 11 px (121) is not
    c = {}
    n, m = _hand_tri(k1, d, _kps([(400, 240, 0), (320, 240, 0)]), np.repeat(d, 2, 0), [0, 1], t2=(0, 0, 1), counters=c)
    assert (n, m[0]) == (1, 0) and c == {"epipole_proximity": 1}
    assert _hand_tri(k1, d, _kps([(329, 240, 0)]), d, [0], t2=(0, 0, 1))[0] == 0
    assert _hand_tri(k1, d, _kps([(331, 240, 0)]), d, [0], t2=(0, 0, 1))[0] == 1


# ---------------------------------------------------------------- 3. the GPU test's scenes are not vacuous
def _covered(c, gates, matches):
    assert matches >= 100, matches
    for g in gates:
        assert c.get(g, 0) >= 10, (g, c)
    assert c.get("ties", 0) >= 5, c


def test_scene_coverage_fuse(fuse_scene):
    c = {}
    nf = R.fuse(*_fuse_args(fuse_scene, 3.0), INV, counters=c)[0]
    _covered(c, ["depth_sign", "image_bounds", "distance_range", "viewing_angle", "octave", "chi_square"], nf)
    S = EYE.copy()
    S[:3] = fuse_scene["T"][:3] * f32(0.5)
    a = list(_fuse_args(fuse_scene, 4.0))
    a[1] = S
    c = {}
    nf = R.fuse_sim3(*a, counters=c)[0]
    _covered(c, ["depth_sign", "image_bounds", "distance_range", "viewing_angle", "octave"], nf)


def test_scene_coverage_sim3(sim3_scene):
    c = {}
    nf = R.search_by_sim3(*_sim3_args(sim3_scene, 7.5), counters=c)[0]
    _covered(c, ["depth_sign", "image_bounds", "distance_range", "octave", "sim3_agreement"], nf)


@pytest.mark.parametrize("which", ["orb", "coarse"])
def test_scene_coverage_triangulation(tri_scenes, which):
    g, fv1, fv2 = tri_scenes[which]
    c = {}
    n = R.search_for_triangulation(*_tri_args(g, fv1, fv2, 1), counters=c)[0]
    _covered(c, ["epipole_proximity", "epipolar_distance", "rotation_histogram"], n)
    if which == "coarse":
        assert np.diff(fv2[1]).max() > 64  # nodes hold more than a wave of features
