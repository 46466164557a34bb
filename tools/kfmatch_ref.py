"""Checker for the keyframe matchers: a numpy restatement of ORBmatcher::SearchForTriangulation,
Fuse, Fuse with a Sim3 and SearchBySim3 (reference src/ORBmatcher.cc:140-157, 657-1326), with
KeyFrame::GetFeaturesInArea / IsInImage (src/KeyFrame.cc:612-656), the Frame grid the keyframe copies
(src/Frame.cc:351-366, 503-513) and MapPoint::PredictScale (src/MapPoint.cc:373-394).

Written from the reference's text, not from the kernels: sequential Python loops in the reference's
order, np.float32 scalars where the reference computes in float, Python floats (double) where it
promotes. The cv::Mat arithmetic follows the rules the project records:
a 3x3 . 3x1 + t product is a float dot, then (float)((double)dot + t); a product with a transposed
operand accumulates in double; Mat / scalar and scalar * Mat are float multiplies by (float)alpha;
cv::norm and Mat::dot accumulate in double. PredictScale is clamped to [0, nlevels - 1] (Q13).
Monocular only (mvuRight < 0 everywhere). Parity with OpenCV's own arithmetic is not pinned by
this file (no OpenCV build here); it pins the engine to the stated rules.

Every function takes an optional `counters` dict: each named gate counts the candidates it rejected
among those that passed the earlier gates (tests/test_kfmatch_ref.py uses it to show that the test
scenes exercise every branch).
"""
import math

import numpy as np

f32 = np.float32
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30  # ORBmatcher.cc:37-39
GRID_COLS, GRID_ROWS = 64, 48                # FRAME_GRID_COLS / FRAME_GRID_ROWS, include/Frame.h:54-55
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _count(counters, key, n=1):
    if counters is not None:
        counters[key] = counters.get(key, 0) + n


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance: the Hamming distance of two 32-byte rows."""
    return int(_POP[np.bitwise_xor(a, b)].sum())


def _c_round(v):
    """C round(): half away from zero."""
    v = float(v)
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def _gemm3(R, t, P):
    """R * P + t for a 3x3 and 3x1 cv::Mat: float dot, the sum with t in double."""
    out = np.zeros(3, f32)
    for r in range(3):
        dot = f32(f32(f32(R[r][0] * P[0]) + f32(R[r][1] * P[1])) + f32(R[r][2] * P[2]))
        out[r] = f32(float(dot) + float(t[r]))
    return out


def _camera_center(Rcw, tcw):
    """Ow = -Rcw.t() * tcw: transposed operand, double accumulation, alpha = -1."""
    Ow = np.zeros(3, f32)
    for c in range(3):
        s = float(Rcw[0][c]) * float(tcw[0])
        s = s + float(Rcw[1][c]) * float(tcw[1])
        s = s + float(Rcw[2][c]) * float(tcw[2])
        Ow[c] = f32(s * -1.0)
    return Ow


def _norm3(a):
    """cv::norm of a 3x1 float Mat: double accumulation, the result assigned to a float."""
    s = 0.0
    for k in range(3):
        s = s + float(a[k]) * float(a[k])
    return f32(math.sqrt(s))


def _dot3(a, b):
    s = 0.0
    for k in range(3):
        s = s + float(a[k]) * float(b[k])
    return s


class KeyFrameGrid:
    """mGrid of a keyframe (Frame::AssignFeaturesToGrid, copied by the KeyFrame constructor) and
    KeyFrame::GetFeaturesInArea / IsInImage. cam: anything with img_w, img_h (k1 == 0: the image
    bounds are 0..w, 0..h)."""

    def __init__(self, cam, kps):
        self.minX, self.maxX, self.minY, self.maxY = f32(0), f32(cam.img_w), f32(0), f32(cam.img_h)
        self.invW = f32(f32(GRID_COLS) / f32(self.maxX - self.minX))
        self.invH = f32(f32(GRID_ROWS) / f32(self.maxY - self.minY))
        self.x = [f32(v) for v in kps["x"]]
        self.y = [f32(v) for v in kps["y"]]
        self.octave = [int(v) for v in kps["octave"]]
        self.grid = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
        for i in range(len(kps)):
            px = _c_round(f32(f32(self.x[i] - self.minX) * self.invW))
            py = _c_round(f32(f32(self.y[i] - self.minY) * self.invH))
            if px < 0 or px >= GRID_COLS or py < 0 or py >= GRID_ROWS:
                continue
            self.grid[px][py].append(i)

    def is_in_image(self, x, y):
        return bool(x >= self.minX and x < self.maxX and y >= self.minY and y < self.maxY)

    def cell_range(self, x, y, r):
        """the cell window of GetFeaturesInArea, None when it returns early."""
        x0 = max(0, int(math.floor(f32(f32(f32(x - self.minX) - r) * self.invW))))
        if x0 >= GRID_COLS:
            return None
        x1 = min(GRID_COLS - 1, int(math.ceil(f32(f32(f32(x - self.minX) + r) * self.invW))))
        if x1 < 0:
            return None
        y0 = max(0, int(math.floor(f32(f32(f32(y - self.minY) - r) * self.invH))))
        if y0 >= GRID_ROWS:
            return None
        y1 = min(GRID_ROWS - 1, int(math.ceil(f32(f32(f32(y - self.minY) + r) * self.invH))))
        if y1 < 0:
            return None
        return x0, x1, y0, y1

    def features_in_area(self, x, y, r):
        w = self.cell_range(x, y, r)
        out = []
        if w is None:
            return out
        x0, x1, y0, y1 = w
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for j in self.grid[ix][iy]:
                    distx = f32(self.x[j] - x)
                    disty = f32(self.y[j] - y)
                    if abs(distx) < r and abs(disty) < r:
                        out.append(j)
        return out


def predict_scale(max_dist, dist, log_scale_factor, nlevels):
    """MapPoint::PredictScale with the Q13 clamp."""
    ratio = f32(f32(max_dist) / f32(dist))
    lvl = int(math.ceil(f32(f32(math.log(float(ratio))) / f32(log_scale_factor))))
    return min(max(lvl, 0), nlevels - 1)


def _search_area(grid, kf_desc, u, v, radius, level, dMP, chi2_inv_sigma2, counters):
    """the candidate loop the four projection searches share: GetFeaturesInArea, the octave gate, Fuse's
    chi-square gate, strict-< best distance. -> (bestDist or None, bestIdx)."""
    bestDist, bestIdx = None, -1
    for idx in grid.features_in_area(u, v, radius):
        kpLevel = grid.octave[idx]
        if kpLevel < level - 1 or kpLevel > level:
            _count(counters, "octave")
            continue
        if chi2_inv_sigma2 is not None:
            ex = f32(u - grid.x[idx])
            ey = f32(v - grid.y[idx])
            e2 = f32(f32(ex * ex) + f32(ey * ey))
            if float(f32(e2 * f32(chi2_inv_sigma2[kpLevel]))) > 5.99:
                _count(counters, "chi_square")
                continue
        dist = descriptor_distance(dMP, kf_desc[idx])
        if bestDist is not None and dist == bestDist:
            _count(counters, "ties")
        if bestDist is None or dist < bestDist:
            bestDist, bestIdx = dist, idx
    return bestDist, bestIdx


def _fuse_core(cam, Rcw, tcw, th, mp_valid, mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc,
               log_scale_factor, kf_kps, kf_desc, nlevels, scale_factors, inv_level_sigma2, double_invz, counters,
               geo=None):
    n_mp = len(mp_valid)
    best_idx = np.full(n_mp, -1, np.int32)
    best_dist = np.full(n_mp, 256, np.int32)
    grid = KeyFrameGrid(cam, kf_kps)
    fx, fy, cx, cy = f32(cam.fx), f32(cam.fy), f32(cam.cx), f32(cam.cy)
    Ow = _camera_center(Rcw, tcw)
    nFused = 0
    with np.errstate(all="ignore"):
        for i in range(n_mp):
            if not mp_valid[i]:
                continue
            p3Dw = np.asarray(mp_pos[i], f32)
            p3Dc = _gemm3(Rcw, tcw, p3Dw)
            if p3Dc[2] < f32(0.0):
                _count(counters, "depth_sign")
                continue
            invz = f32(1.0 / float(p3Dc[2])) if double_invz else f32(f32(1) / p3Dc[2])
            x = f32(p3Dc[0] * invz)
            y = f32(p3Dc[1] * invz)
            u = f32(f32(fx * x) + cx)
            v = f32(f32(fy * y) + cy)
            if not grid.is_in_image(u, v):
                _count(counters, "image_bounds")
                continue
            maxDistance = f32(f32(1.2) * f32(mp_max_dist[i]))
            minDistance = f32(f32(0.8) * f32(mp_min_dist[i]))
            PO = np.array([f32(p3Dw[k] - Ow[k]) for k in range(3)], f32)
            dist3D = _norm3(PO)
            if dist3D < minDistance or dist3D > maxDistance:
                _count(counters, "distance_range")
                continue
            if _dot3(PO, mp_normal[i]) < 0.5 * float(dist3D):
                _count(counters, "viewing_angle")
                continue
            level = predict_scale(mp_max_dist[i], dist3D, log_scale_factor, nlevels)
            radius = f32(f32(th) * f32(scale_factors[level]))
            if geo is not None:
                geo[i] = (u, v, radius, level)
            bd, bi = _search_area(grid, kf_desc, u, v, radius, level, mp_desc[i], inv_level_sigma2, counters)
            if bd is None:
                continue
            best_dist[i] = bd
            if bd <= TH_LOW:
                best_idx[i] = bi
                nFused += 1
    return nFused, best_idx, best_dist


def fuse(cam, Tcw, th, mp_valid, mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc, log_scale_factor, kf_kps,
         kf_desc, scale_factors, inv_level_sigma2, counters=None, geo=None):
    """ORBmatcher::Fuse(pKF, vpMapPoints, th), :825-975 -> (nFused, best_idx, best_dist). geo: an optional
    dict that receives {i: (u, v, radius, level)} for the points that reach the area search."""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    return _fuse_core(cam, T[:3, :3], T[:3, 3], th, mp_valid, mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc,
                      log_scale_factor, kf_kps, kf_desc, len(scale_factors), scale_factors, inv_level_sigma2, False,
                      counters, geo)


def decompose_sim3(Scw):
    """:985-989: scw = sqrt(row0 . row0), Rcw = sRcw / scw, tcw = t / scw."""
    S = np.asarray(Scw, f32).reshape(4, 4)
    scw = f32(math.sqrt(_dot3(S[0, :3], S[0, :3])))
    inv = f32(1.0 / float(scw))
    R = np.array([[f32(S[r][c] * inv) for c in range(3)] for r in range(3)], f32)
    t = np.array([f32(S[r][3] * inv) for r in range(3)], f32)
    return R, t


def fuse_sim3(cam, Scw, th, mp_valid, mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc, log_scale_factor,
              kf_kps, kf_desc, scale_factors, counters=None, geo=None):
    """ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint), :977-1100 -> (nFused, best_idx, best_dist)."""
    R, t = decompose_sim3(Scw)
    return _fuse_core(cam, R, t, th, mp_valid, mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc,
                      log_scale_factor, kf_kps, kf_desc, len(scale_factors), scale_factors, None, True, counters, geo)


def sim3_transforms(s12, R12, t12):
    """:1119-1121 -> (sR12, sR21, t21)."""
    R12 = np.asarray(R12, f32).reshape(3, 3)
    t12 = np.asarray(t12, f32).reshape(3)
    s12 = f32(s12)
    inv = f32(1.0 / float(s12))
    sR12 = np.array([[f32(R12[r][c] * s12) for c in range(3)] for r in range(3)], f32)
    sR21 = np.array([[f32(R12[c][r] * inv) for c in range(3)] for r in range(3)], f32)
    t21 = np.zeros(3, f32)
    for r in range(3):
        dot = f32(f32(f32(sR21[r][0] * t12[0]) + f32(sR21[r][1] * t12[1])) + f32(sR21[r][2] * t12[2]))
        t21[r] = f32(float(dot) * -1.0)
    return sR12, sR21, t21


def sim3_half(cam, Tcw_own, sR, t, th, mp_valid, already, mp_pos, mp_min_dist, mp_max_dist, mp_desc,
              log_scale_factor, kps_other, desc_other, scale_factors, counters=None, geo=None):
    """one of the two loops of SearchBySim3 (:1146-1224 / :1226-1303): the points of one keyframe through
    their own pose and the Sim3 into the other keyframe -> vnMatch."""
    n = len(mp_valid)
    vnMatch = np.full(n, -1, np.int32)
    T = np.asarray(Tcw_own, f32).reshape(4, 4)
    grid = KeyFrameGrid(cam, kps_other)
    fx, fy, cx, cy = f32(cam.fx), f32(cam.fy), f32(cam.cx), f32(cam.cy)
    nlevels = len(scale_factors)
    with np.errstate(all="ignore"):
        for i in range(n):
            if not mp_valid[i] or already[i]:
                continue
            p3Dw = np.asarray(mp_pos[i], f32)
            p3Dc_own = _gemm3(T[:3, :3], T[:3, 3], p3Dw)
            p3Dc = _gemm3(sR, t, p3Dc_own)
            if float(p3Dc[2]) < 0.0:
                _count(counters, "depth_sign")
                continue
            invz = f32(1.0 / float(p3Dc[2]))
            x = f32(p3Dc[0] * invz)
            y = f32(p3Dc[1] * invz)
            u = f32(f32(fx * x) + cx)
            v = f32(f32(fy * y) + cy)
            if not grid.is_in_image(u, v):
                _count(counters, "image_bounds")
                continue
            maxDistance = f32(f32(1.2) * f32(mp_max_dist[i]))
            minDistance = f32(f32(0.8) * f32(mp_min_dist[i]))
            dist3D = _norm3(p3Dc)
            if dist3D < minDistance or dist3D > maxDistance:
                _count(counters, "distance_range")
                continue
            level = predict_scale(mp_max_dist[i], dist3D, log_scale_factor, nlevels)
            radius = f32(f32(th) * f32(scale_factors[level]))
            if geo is not None:
                geo[i] = (u, v, radius, level)
            bd, bi = _search_area(grid, desc_other, u, v, radius, level, mp_desc[i], None, counters)
            if bd is not None and bd <= TH_HIGH:
                vnMatch[i] = bi
    return vnMatch


def search_by_sim3(cam, Tcw1, Tcw2, s12, R12, t12, th, kps1, desc1, mp_valid1, mp_pos1, mp_min_dist1,
                   mp_max_dist1, mp_desc1, already_matched1, kps2, desc2, mp_valid2, mp_pos2, mp_min_dist2,
                   mp_max_dist2, mp_desc2, already_matched2, log_scale_factor, scale_factors, counters=None,
                   halves=None):
    """ORBmatcher::SearchBySim3, :1102-1326 -> (nFound, match12). halves: an optional list that
    receives (vnMatch1, vnMatch2)."""
    sR12, sR21, t21 = sim3_transforms(s12, R12, t12)
    t12 = np.asarray(t12, f32).reshape(3)
    vnMatch1 = sim3_half(cam, Tcw1, sR21, t21, th, mp_valid1, already_matched1, mp_pos1, mp_min_dist1,
                         mp_max_dist1, mp_desc1, log_scale_factor, kps2, desc2, scale_factors, counters)
    vnMatch2 = sim3_half(cam, Tcw2, sR12, t12, th, mp_valid2, already_matched2, mp_pos2, mp_min_dist2,
                         mp_max_dist2, mp_desc2, log_scale_factor, kps1, desc1, scale_factors, counters)
    if halves is not None:
        halves.append((vnMatch1, vnMatch2))
    match12 = np.full(len(mp_valid1), -1, np.int32)
    nFound = 0
    for i1 in range(len(vnMatch1)):
        idx2 = int(vnMatch1[i1])
        if idx2 >= 0:
            idx1 = int(vnMatch2[idx2])
            if idx1 == i1:
                match12[i1] = idx2
                nFound += 1
            else:
                _count(counters, "sim3_agreement")
    return nFound, match12


def check_dist_epipolar_line(x1, y1, x2, y2, octave2, F12, level_sigma2):
    """ORBmatcher::CheckDistEpipolarLine, :140-157. -> (ok, den_is_zero)."""
    a = f32(f32(f32(x1 * F12[0][0]) + f32(y1 * F12[1][0])) + F12[2][0])
    b = f32(f32(f32(x1 * F12[0][1]) + f32(y1 * F12[1][1])) + F12[2][1])
    c = f32(f32(f32(x1 * F12[0][2]) + f32(y1 * F12[1][2])) + F12[2][2])
    num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
    den = f32(f32(a * a) + f32(b * b))
    if den == 0:
        return False
    dsqr = f32(f32(num * num) / den)
    return bool(float(dsqr) < 3.84 * float(f32(level_sigma2[octave2])))


def compute_three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima, :1601-1642, on the bin sizes."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3 = s
            ind3 = i
    if max2 < f32(f32(0.1) * f32(max1)):
        ind2 = ind3 = -1
    elif max3 < f32(f32(0.1) * f32(max1)):
        ind3 = -1
    return ind1, ind2, ind3


def search_for_triangulation(cam2, F12, Ow1, Tcw2, check_ori, kps1, desc1, has_mp1, fv1, kps2, desc2, has_mp2,
                             fv2, scale_factors, level_sigma2, counters=None):
    """ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, false), :657-823.
    fv = (node_ids, node_start, node_feats) -> (nmatches, match12)."""
    F12 = np.asarray(F12, f32).reshape(3, 3)
    T2 = np.asarray(Tcw2, f32).reshape(4, 4)
    fx, fy, cx, cy = f32(cam2.fx), f32(cam2.fy), f32(cam2.cx), f32(cam2.cy)
    n1 = len(kps1)
    vMatches12 = np.full(n1, -1, np.int32)
    x1, y1, a1 = [f32(v) for v in kps1["x"]], [f32(v) for v in kps1["y"]], [f32(v) for v in kps1["angle"]]
    x2, y2, a2 = [f32(v) for v in kps2["x"]], [f32(v) for v in kps2["y"]], [f32(v) for v in kps2["angle"]]
    oct2 = [int(v) for v in kps2["octave"]]
    ids1, st1, ft1 = [np.asarray(a) for a in fv1]
    ids2, st2, ft2 = [np.asarray(a) for a in fv2]
    nmatches = 0
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    factor = f32(f32(1.0) / f32(HISTO_LENGTH))
    with np.errstate(all="ignore"):
        C2 = _gemm3(T2[:3, :3], T2[:3, 3], np.asarray(Ow1, f32).reshape(3))
        invz = f32(f32(1.0) / C2[2])
        ex = f32(f32(f32(fx * C2[0]) * invz) + cx)
        ey = f32(f32(f32(fy * C2[1]) * invz) + cy)
        i, j = 0, 0
        while i < len(ids1) and j < len(ids2):
            if ids1[i] == ids2[j]:
                for p in range(int(st1[i]), int(st1[i + 1])):
                    idx1 = int(ft1[p])
                    if has_mp1[idx1]:
                        continue
                    bestDist = TH_LOW
                    bestIdx2 = -1
                    for q in range(int(st2[j]), int(st2[j + 1])):
                        idx2 = int(ft2[q])
                        if has_mp2[idx2]:
                            continue
                        dist = descriptor_distance(desc1[idx1], desc2[idx2])
                        if dist > TH_LOW or dist > bestDist:
                            continue
                        distex = f32(ex - x2[idx2])
                        distey = f32(ey - y2[idx2])
                        near = f32(f32(100) * f32(scale_factors[oct2[idx2]]))
                        if f32(f32(distex * distex) + f32(distey * distey)) < near:
                            _count(counters, "epipole_proximity")
                            continue
                        if check_dist_epipolar_line(x1[idx1], y1[idx1], x2[idx2], y2[idx2], oct2[idx2], F12,
                                                    level_sigma2):
                            if bestIdx2 >= 0 and dist == bestDist:
                                _count(counters, "ties")
                            bestIdx2 = idx2
                            bestDist = dist
                        else:
                            _count(counters, "epipolar_distance")
                    if bestIdx2 >= 0:
                        vMatches12[idx1] = bestIdx2
                        nmatches += 1
                        if check_ori:
                            rot = f32(a1[idx1] - a2[bestIdx2])
                            if rot < 0.0:
                                rot = f32(rot + f32(360.0))
                            b = _c_round(f32(rot * factor))
                            if b == HISTO_LENGTH:
                                b = 0
                            rotHist[b].append(idx1)
                i += 1
                j += 1
            elif ids1[i] < ids2[j]:
                i = int(np.searchsorted(ids1, ids2[j], side="left"))  # lower_bound
            else:
                j = int(np.searchsorted(ids2, ids1[i], side="left"))
    if check_ori:
        ind1, ind2, ind3 = compute_three_maxima([len(h) for h in rotHist])
        for b in range(HISTO_LENGTH):
            if b == ind1 or b == ind2 or b == ind3:
                continue
            for idx1 in rotHist[b]:
                vMatches12[idx1] = -1
                nmatches -= 1
                _count(counters, "rotation_histogram")
    return nmatches, vMatches12
