"""orb_py.py -- a second, independent restatement of ORB extraction
(TEST INFRASTRUCTURE ONLY: imported by tests/ alone, never by the product).

Written in numpy from the reference text (src/ORBextractor.cc) and from the textbook
definitions of the primitives it calls, not from oracle/orb_ref.cpp and not from OpenCV's
loop structure, so that a misreading shared by the C++ oracle and the kernels (an NMS rule, a
cell fallback, an octree tie-break, a pattern rotation) cannot pass unnoticed.
tests/test_oracle_orb_py.py runs the oracle against it stage by stage, and
tests/test_gpu_orb_definition.py the engine.

Stages (each takes the previous stage's output, so each can be checked alone):
  level_sizes    ORBextractor::ORBextractor :415-431, ComputePyramid :1111-1112
  quotas         :435-446
  umax_table     :454-469
  resize_float   bilinear interpolation by definition (pixel centres, source size over
                 destination size, border clamped), double precision, unrounded (:1120)
  fast_cells     the cell loop of ComputeKeyPointsOctTree :769-829 over a definitional
                 FAST-9/16 (Rosten & Drummond): response = the largest threshold at which the
                 pixel is still a corner, kept only if strictly above its 8 neighbours
  distribute     DivideNode :481-537 and DistributeOctTree :539-763 on plain lists
  moments        IC_Angle :77-101 (integer m10, m01)
  blur_int       the 8-bit 7x7 sigma-2 blur :1086: taps 18 34 49 55 49 34 18 (/256, sum 257), two
                 passes, one rounding (+2^15 >> 16), reflect-101 borders
  blur_float     the true Gaussian the taps approximate
  describe       computeOrbDescriptor :108-147 in float32, one rounding per operation
  extract        operator() :1043-1105

The two fixed-point stages of the reference's OpenCV (resize, fastAtan2) have no definition
to restate exactly: resize_float and the double-precision atan2 bound them, and `extract`
takes a pyramid and angles from outside so that everything downstream is checked exactly.

Documented decisions shared with the oracle: Q14 (equal-size nodes in the sorted
last expansion are ordered by creation, standing in for the reference's heap addresses) and
Q26 (cos / sin of the descriptor angle are the float32 of the double-precision values).
"""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATTERN_INC = os.path.join(os.path.dirname(HERE), "eao-slam_amd", "csrc", "orb_pattern.inc")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

PATCH_SIZE = 31       # :72
HALF_PATCH = 15       # :73
EDGE = 19             # :74
CELL = 30.0           # :769
F32 = np.float32

# the Bresenham circle of radius 3 FAST tests, in circular order (dx, dy)
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
BLUR_TAPS = (18, 34, 49, 55, 49, 34, 18)


def _rint(v):
    """cvRound: round half to even."""
    return int(np.rint(v))


# ------------------------------------------------------------------ tables
def level_sizes(w, h, scale_factor=1.2, nlevels=8):
    """-> ([(w_l, h_l)], dict of float32 tables scale / inv_scale / sigma2 / inv_sigma2).
    The scale factor arrives as a float and is kept in a double member (ORBextractor.h:98),
    so scale[i] = float(double(scale[i-1]) * double(float(1.2))) (:421)."""
    sf = float(F32(scale_factor))
    scale = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        scale[i] = F32(float(scale[i - 1]) * sf)
    sigma2 = scale * scale                      # :422, float product
    inv_scale = F32(1.0) / scale                # :429
    inv_sigma2 = F32(1.0) / sigma2              # :430
    sizes = [(_rint(F32(w) * inv_scale[l]), _rint(F32(h) * inv_scale[l])) for l in range(nlevels)]  # :1112
    return sizes, dict(scale=scale, inv_scale=inv_scale, sigma2=sigma2, inv_sigma2=inv_sigma2)


def quotas(nfeatures, scale_factor=1.2, nlevels=8):
    """Features per level, :435-446."""
    factor = F32(1.0 / float(F32(scale_factor)))
    n = F32(F32(nfeatures) * (F32(1) - factor)) / (F32(1) - F32(math.pow(float(factor), float(nlevels))))
    q, total = [], 0
    for _ in range(nlevels - 1):
        q.append(_rint(n))
        total += q[-1]
        n = F32(n * factor)
    q.append(max(nfeatures - total, 0))
    return q


def umax_table():
    """End of each row of the circular patch, :454-469."""
    umax = [0] * (HALF_PATCH + 1)
    root2 = float(F32(math.sqrt(2.0)))
    vmax = int(math.floor(float(F32(F32(HALF_PATCH * root2) / F32(2)) + F32(1))))
    vmin = int(math.ceil(float(F32(HALF_PATCH * root2) / F32(2))))
    for v in range(vmax + 1):
        umax[v] = _rint(math.sqrt(HALF_PATCH * HALF_PATCH - v * v))
    v0 = 0
    for v in range(HALF_PATCH, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


# ------------------------------------------------------------------ pyramid
def resize_float(prev, dw, dh):
    """Bilinear resize of prev [sh][sw] to [dh][dw] in double precision, unrounded: destination
    pixel centre (d + 0.5) maps to source coordinate (d + 0.5) * s / d_size - 0.5, samples
    outside the image take the border pixel."""
    src = np.asarray(prev, np.float64)
    sh, sw = src.shape

    def axis(dn, sn):
        c = (np.arange(dn, dtype=np.float64) + 0.5) * (sn / dn) - 0.5
        i0 = np.floor(c)
        f = c - i0
        i0 = i0.astype(np.int64)
        return np.clip(i0, 0, sn - 1), np.clip(i0 + 1, 0, sn - 1), f

    x0, x1, fx = axis(dw, sw)
    y0, y1, fy = axis(dh, sh)
    top = src[y0][:, x0] * (1 - fx) + src[y0][:, x1] * fx
    bot = src[y1][:, x0] * (1 - fx) + src[y1][:, x1] * fx
    return top * (1 - fy)[:, None] + bot * fy[:, None]


def resize_delta(sw, sh):
    """How far from a rounding half the exact bilinear value must lie for an 11-bit fixed-point
    resize of an [sh][sw] image (the reference's cv::resize) to be bound to round the same way.
    Each of the four weights (two per axis) is rounded to a multiple of 1/2048, so it is off
    by at most 1/4096; the value sum_ij ax_i ay_j p_ij with p <= 255 then moves by at most
    255 * (2/4096 + 2/4096 + 4/4096^2). The source coordinate is rounded to float32 before its
    fraction is taken: an error of at most half an ulp of a number below max(sw, sh), and the
    bilinear surface has slope at most 255 per pixel along each axis. The fixed-point products
    and the final (+2^21 >> 22) are exact integer arithmetic and add nothing."""
    coef = 255.0 * (4.0 / 4096 + 4.0 / 4096 ** 2)
    ulp_half = 2.0 ** (math.ceil(math.log2(max(sw, sh))) - 25)
    return coef + 2 * 255.0 * ulp_half


def pyramid_float(img, sizes):
    """The pyramid by definition: each level the rounded resize_float of the level above."""
    levels = [np.ascontiguousarray(img, np.uint8)]
    for (lw, lh) in sizes[1:]:
        levels.append(np.clip(np.rint(resize_float(levels[-1], lw, lh)), 0, 255).astype(np.uint8))
    return levels


# ------------------------------------------------------------------ FAST
def fast_response(level):
    """FAST-9/16 response of every pixel of `level` whose radius-3 circle lies inside it (0
    elsewhere): the largest t such that 9 contiguous circle pixels are all brighter than the
    centre by more than t, or all darker by more than t; negative where no t >= 0 qualifies.
    A pixel is a corner at threshold t exactly when response >= t."""
    img = np.asarray(level, np.int16)
    h, w = img.shape
    out = np.zeros((h, w), np.int16)
    if h < 7 or w < 7:
        return out
    c = img[3:h - 3, 3:w - 3]
    d = np.stack([c - img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE])  # centre - circle
    best = None
    for s in (d, -d):
        m2 = np.minimum(s, np.roll(s, -1, 0))
        m4 = np.minimum(m2, np.roll(m2, -2, 0))
        m8 = np.minimum(m4, np.roll(m4, -4, 0))
        m9 = np.minimum(m8, np.roll(s, -8, 0))       # min over circle[k .. k+8], every start k
        arc = m9.max(0)
        best = arc if best is None else np.maximum(best, arc)
    out[3:h - 3, 3:w - 3] = best - 1                 # differences must exceed t strictly
    return out


def fast_nms(resp, th):
    """Corners of one sub-image at threshold th, non-maximum suppressed: a corner stays only
    if its response is strictly greater than that of each of its 8 neighbours (a neighbour that
    is no corner at th counts as 0). resp: fast_response of the sub-image ALONE. Returns
    (x, y, response) row by row, left to right."""
    h, w = resp.shape
    s = np.zeros((h + 2, w + 2), np.int16)
    s[1:-1, 1:-1] = np.where(resp >= th, resp, 0)
    c = s[1:-1, 1:-1]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= c > s[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
    ys, xs = np.nonzero(keep)
    return [(int(x), int(y), int(c[y, x])) for y, x in zip(ys, xs)]


def cell_grid(cols, rows):
    """The cells of one level, :773-806: [(i, j, x0, x1, y0, y1)] in loop order, plus
    (wCell, hCell). Cells overlap by 6 pixels, the detector's two 3-pixel margins."""
    min_b = EDGE - 3
    max_bx, max_by = cols - EDGE + 3, rows - EDGE + 3
    width, height = F32(max_bx - min_b), F32(max_by - min_b)
    n_cols, n_rows = int(width / F32(CELL)), int(height / F32(CELL))
    w_cell, h_cell = int(math.ceil(width / F32(n_cols))), int(math.ceil(height / F32(n_rows)))
    cells = []
    for i in range(n_rows):
        y0 = min_b + i * h_cell
        y1 = y0 + h_cell + 6
        if y0 >= max_by - 3:
            continue
        y1 = min(y1, max_by)
        for j in range(n_cols):
            x0 = min_b + j * w_cell
            x1 = x0 + w_cell + 6
            if x0 >= max_bx - 6:
                continue
            x1 = min(x1, max_bx)
            cells.append((i, j, x0, x1, y0, y1))
    return cells, (w_cell, h_cell)


def fast_cells(level, ini_th=20, min_th=7):
    """Candidates of one level in the reference's emission order, [(x, y, response)] with x, y
    relative to the (16, 16) border corner: each cell detected and suppressed as its own
    sub-image at ini_th, again at min_th if that left nothing (:808-826).
    The response of a pixel depends only on its own circle, so the level's response map is
    computed once and each cell takes its window of it, zeroed on the cell's 3-pixel rim where
    the circle would leave the cell."""
    level = np.asarray(level, np.uint8)
    rows, cols = level.shape
    resp = fast_response(level)
    cells, (w_cell, h_cell) = cell_grid(cols, rows)
    out = []
    for i, j, x0, x1, y0, y1 in cells:
        sub = np.zeros((y1 - y0, x1 - x0), np.int16)
        if sub.shape[0] >= 7 and sub.shape[1] >= 7:
            sub[3:-3, 3:-3] = resp[y0 + 3:y1 - 3, x0 + 3:x1 - 3]
        kps = fast_nms(sub, ini_th)
        if not kps:
            kps = fast_nms(sub, min_th)
        out.extend((x + j * w_cell, y + i * h_cell, r) for x, y, r in kps)
    return out


# ------------------------------------------------------------------ octree
class _Node:
    __slots__ = ("x0", "x1", "y0", "y1", "keys", "no_more", "born")

    def __init__(self, x0, x1, y0, y1):
        self.x0, self.x1, self.y0, self.y1 = x0, x1, y0, y1
        self.keys = []
        self.no_more = False
        self.born = 0


def _divide(n, cands):
    """DivideNode :481-537: children in the order n1 (upper left), n2 (upper right), n3 (lower
    left), n4 (lower right); the split lines are the rounded-up halves."""
    hx = -((n.x0 - n.x1) // 2)
    hy = -((n.y0 - n.y1) // 2)
    mx, my = n.x0 + hx, n.y0 + hy
    kids = [_Node(n.x0, mx, n.y0, my), _Node(mx, n.x1, n.y0, my), _Node(n.x0, mx, my, n.y1), _Node(mx, n.x1, my, n.y1)]
    for k in n.keys:
        x, y = cands[k][0], cands[k][1]
        kids[(0 if x < mx else 1) + (0 if y < my else 2)].keys.append(k)
    for c in kids:
        c.no_more = len(c.keys) == 1
    return kids


def distribute(cands, min_x, max_x, min_y, max_y, n_want):
    """DistributeOctTree :539-763. cands: [(x, y, response)] relative to (min_x, min_y).
    Returns the indices of the survivors in the order of the final node list.
    The node list is a plain Python list whose index 0 is the std::list's front."""
    if not cands:
        return []
    n_ini = int(math.floor(float(F32(max_x - min_x) / F32(max_y - min_y)) + 0.5))   # round(), :543
    h_x = F32(max_x - min_x) / F32(n_ini)
    born = 0
    nodes = []
    for i in range(n_ini):
        nd = _Node(int(h_x * F32(i)), int(h_x * F32(i + 1)), 0, max_y - min_y)
        nd.born = born
        born += 1
        nodes.append(nd)
    for k, c in enumerate(cands):
        nodes[int(F32(c[0]) / h_x)].keys.append(k)                                 # :569
    nodes = [nd for nd in nodes if nd.keys]
    for nd in nodes:
        nd.no_more = len(nd.keys) == 1

    def push_children(parent, expandable):
        nonlocal born
        for c in _divide(parent, cands):
            if c.keys:
                c.born = born
                born += 1
                nodes.insert(0, c)                                                 # push_front
                if len(c.keys) > 1:
                    expandable.append(c)

    finish = False
    while not finish:
        prev = len(nodes)
        expandable = []
        for nd in list(nodes):           # children go to the front: this pass never visits them
            if nd.no_more:
                continue
            push_children(nd, expandable)
            nodes.remove(nd)
        if len(nodes) >= n_want or len(nodes) == prev:
            finish = True
        elif len(nodes) + 3 * len(expandable) > n_want:
            while not finish:
                prev = len(nodes)
                # sort ascending by (size, pointer) and walk from the back, :684-685; the pointer
                # order is the creation order (Q14)
                order = sorted(expandable, key=lambda c: (len(c.keys), c.born))
                expandable = []
                for nd in reversed(order):
                    push_children(nd, expandable)
                    nodes.remove(nd)
                    if len(nodes) >= n_want:
                        break
                if len(nodes) >= n_want or len(nodes) == prev:
                    finish = True
    out = []
    for nd in nodes:                      # :744-760: the first strictly largest response
        best = nd.keys[0]
        for k in nd.keys[1:]:
            if cands[k][2] > cands[best][2]:
                best = k
        out.append(best)
    return out


# ------------------------------------------------------------------ orientation
def moments(level, x, y, umax=None):
    """IC_Angle's integer moments (m10, m01) over the circular patch around (x, y), :77-101."""
    umax = umax_table() if umax is None else umax
    img = np.asarray(level, np.int64)
    m10 = m01 = 0
    for v in range(-HALF_PATCH, HALF_PATCH + 1):
        d = umax[abs(v)]
        u = np.arange(-d, d + 1)
        row = img[y + v, x - d:x + d + 1]
        m10 += int((u * row).sum())
        m01 += v * int(row.sum())
    return m10, m01


def angle_deg(m10, m01):
    """The orientation by definition: atan2(m01, m10) in degrees, [0, 360)."""
    return math.degrees(math.atan2(m01, m10)) % 360.0


# ------------------------------------------------------------------ blur
def _pad101(a, r):
    return np.pad(a, r, mode="reflect")          # numpy 'reflect' repeats no edge pixel: reflect-101


def blur_int(level):
    """The 8-bit 7x7 blur exactly: integer taps (sum 257 of 256), rows then columns without an
    intermediate rounding, then (sum + 2^15) >> 16."""
    a = np.asarray(level, np.int64)
    h, w = a.shape
    p = _pad101(a, 3)
    rows = sum(t * p[:, i:i + w] for i, t in enumerate(BLUR_TAPS))
    both = sum(t * rows[i:i + h, :] for i, t in enumerate(BLUR_TAPS))
    return np.clip((both + (1 << 15)) >> 16, 0, 255).astype(np.uint8)


def gauss_taps():
    """The normalised 7-tap Gaussian of sigma 2."""
    g = np.exp(-0.5 * (np.arange(7) - 3.0) ** 2 / 4.0)
    return g / g.sum()


def blur_float(level):
    """The true 7x7 Gaussian (sigma 2) with reflect-101 borders, double precision, unrounded."""
    a = np.asarray(level, np.float64)
    h, w = a.shape
    g = gauss_taps()
    p = _pad101(a, 3)
    rows = sum(t * p[:, i:i + w] for i, t in enumerate(g))
    return sum(t * rows[i:i + h, :] for i, t in enumerate(g))


def blur_bound():
    """max |blur_int - blur_float| from the two kernels: the 2-D taps differ by
    k_i k_j / 65536 - g_i g_j on pixels of at most 255, plus the final rounding half."""
    k = np.array(BLUR_TAPS, np.float64)
    g = gauss_taps()
    return 255.0 * np.abs(np.outer(k, k) / 65536.0 - np.outer(g, g)).sum() + 0.5


# ------------------------------------------------------------------ descriptor
_pattern = None


def pattern():
    """The 512 rBRIEF points [(x, y)] parsed from the engine's table (generated from :150-408)."""
    global _pattern
    if _pattern is None:
        txt = "\n".join(l.split("//")[0] for l in open(PATTERN_INC).read().splitlines())
        v = np.array([int(t) for t in txt.replace(",", " ").split()], np.int32)
        assert v.size == 1024
        _pattern = v.reshape(512, 2)
    return _pattern


def describe(blurred, kp_x, kp_y, angle_f32):
    """rBRIEF bits of keypoints at integer level positions (kp_x, kp_y) with angles in degrees,
    :108-147 -> [n][32] u8. Float32 throughout, every product and sum rounded once (no fused
    multiply-add); a, b are the float32 of the double cosine / sine of the float32 angle in
    radians (Q26); coordinates round half to even."""
    img = np.asarray(blurred, np.uint8)
    n = len(kp_x)
    if n == 0:
        return np.zeros((0, 32), np.uint8)
    factor_pi = F32(math.pi / float(F32(180.0)))                                   # :107
    ang = np.asarray(angle_f32, F32) * factor_pi
    a = np.cos(ang.astype(np.float64)).astype(F32)[:, None]
    b = np.sin(ang.astype(np.float64)).astype(F32)[:, None]
    px = pattern()[:, 0].astype(F32)[None, :]
    py = pattern()[:, 1].astype(F32)[None, :]
    ry = np.rint((px * b).astype(F32) + (py * a).astype(F32)).astype(np.int64)     # row offset, :119
    rx = np.rint((px * a).astype(F32) - (py * b).astype(F32)).astype(np.int64)     # column offset, :120
    cy = np.rint(np.asarray(kp_y, F32)).astype(np.int64)[:, None]
    cx = np.rint(np.asarray(kp_x, F32)).astype(np.int64)[:, None]
    val = img[cy + ry, cx + rx].astype(np.int32)                                   # [n][512]
    bits = (val[:, 0::2] < val[:, 1::2]).astype(np.uint8)                          # [n][256]
    return np.packbits(bits.reshape(n, 32, 8), axis=2, bitorder="little").reshape(n, 32)


# ------------------------------------------------------------------ composition
def detect(pyr, nfeatures=1000, ini_th=20, min_th=7, scale_factor=1.2):
    """ComputeKeyPointsOctTree :765-848 without the orientation: per level the surviving
    (x, y, response) in level coordinates (border added), in the reference's order."""
    q = quotas(nfeatures, scale_factor, len(pyr))
    out = []
    for l, lev in enumerate(pyr):
        rows, cols = lev.shape
        min_b, max_bx, max_by = EDGE - 3, cols - EDGE + 3, rows - EDGE + 3
        cands = fast_cells(lev, ini_th, min_th)
        sel = distribute(cands, min_b, max_bx, min_b, max_by, q[l])
        out.append([(cands[k][0] + min_b, cands[k][1] + min_b, cands[k][2]) for k in sel])
    return out


def finish(pyr, det, angles=None, scale_factor=1.2):
    """Orientation, blur, descriptors and the output scaling of operator() :1059-1104 for the
    per-level keypoints of detect(). angles: float32 degrees in output order, else the
    double-precision atan2 of the moments rounded to float32."""
    _, tab = level_sizes(1, 1, scale_factor, len(pyr))
    total = sum(len(d) for d in det)
    kps = np.zeros(total, KP_DTYPE)
    desc = np.zeros((total, 32), np.uint8)
    umax = umax_table()
    o = 0
    for l, (lev, d) in enumerate(zip(pyr, det)):
        n = len(d)
        if n == 0:
            continue
        x = np.array([c[0] for c in d], F32)
        y = np.array([c[1] for c in d], F32)
        if angles is None:
            ang = np.array([angle_deg(*moments(lev, c[0], c[1], umax)) for c in d], F32)
        else:
            ang = np.asarray(angles[o:o + n], F32)
        desc[o:o + n] = describe(blur_int(lev), x, y, ang)
        k = kps[o:o + n]
        sc = tab["scale"][l]
        k["x"] = x * sc if l else x                                                # :1095-1100
        k["y"] = y * sc if l else y
        k["size"] = F32(int(F32(PATCH_SIZE) * sc))                                 # :837
        k["angle"] = ang
        k["response"] = [c[2] for c in d]
        k["octave"] = l
        k["class_id"] = -1
        o += n
    return kps, desc


def extract(img, nfeatures=1000, ini_th=20, min_th=7, pyramid=None, angles=None, scale_factor=1.2, nlevels=8):
    """operator() :1043-1105 -> (keypoints KP_DTYPE, descriptors [n][32]) in the reference's
    order. pyramid / angles given: used in place of this module's own (the two stages whose
    fixed-point arithmetic is bounded, not restated)."""
    img = np.ascontiguousarray(img, np.uint8)
    if pyramid is None:
        sizes, _ = level_sizes(img.shape[1], img.shape[0], scale_factor, nlevels)
        pyramid = pyramid_float(img, sizes)
    det = detect(pyramid, nfeatures, ini_th, min_th, scale_factor)
    return finish(pyramid, det, angles, scale_factor)
