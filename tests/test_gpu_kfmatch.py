"""GPU keyframe matchers (k_kf_project / k_sim3_agree in match.hip, k_bow_triang in bow.hip) vs
tools/kfmatch_ref.py, the numpy restatement of ORBmatcher::Fuse, Fuse with a Sim3, SearchBySim3 and
SearchForTriangulation (reference src/ORBmatcher.cc:140-157, 657-1326).

Bar: bit-exact -- every index, every distance, every returned count. The scenes are the ones
tests/test_kfmatch_ref.py shows to exercise every gate (tools/synth.py: fuse_scene, sim3_scene,
triangulation_scene), 640x480, at most 1024 keypoints and 640 map points per search.
"""
import ctypes

import numpy as np
import pytest

import eao_accel as ea
import pyoracle as orc
from tools import kfmatch_ref as R
from tools import synth

pytestmark = pytest.mark.gpu

f32 = np.float32
CAM = ea.camera()
SF, SIG, INV, LOGSF = synth.level_tables()


@pytest.fixture(scope="module")
def M():
    return ea.Matcher(max_kps=1024, max_batch=6)


@pytest.fixture(scope="module")
def fuse_scene():
    return synth.fuse_scene(0)


@pytest.fixture(scope="module")
def sim3_scene():
    return synth.sim3_scene(0)


def _mp(s, n=None, valid=None):
    mp = s["mp"]
    v = mp["valid"] if valid is None else valid
    return [a[:n] for a in (v, mp["pos"], mp["normal"], mp["mind"], mp["maxd"], mp["desc"])]


def _same(g, o):
    assert g[0] == o[0], (g[0], o[0])
    for a, b in zip(g[1:], o[1:]):
        assert a.shape == b.shape and np.array_equal(a, b), int((a != b).sum())


# ---------------------------------------------------------------- Fuse
@pytest.mark.parametrize("n_kf", [0, 1, 1000])
@pytest.mark.parametrize("n_mp", [0, 1, 63, 65, 600])
def test_fuse_sizes(M, fuse_scene, n_mp, n_kf):
    s = fuse_scene
    kps, desc = s["kps"][:n_kf], s["desc"][:n_kf]
    assert len(kps) == n_kf
    g = M.fuse(CAM, s["T"], 3.0, *_mp(s, n_mp), LOGSF, kps, desc, SF, INV)
    o = R.fuse(CAM, s["T"], 3.0, *_mp(s, n_mp), LOGSF, kps, desc, SF, INV)
    _same(g, o)
    _same(M.fuse(CAM, s["T"], 3.0, *_mp(s, n_mp), LOGSF, kps, desc, SF, INV), g)  # the same handle again
    if n_mp == 600 and n_kf == 1000:
        assert o[0] > 100


def test_fuse_large_radius_and_borders(M, fuse_scene):
    """th = 2.5 * the coarsest scale factor (windows of hundreds of cells), with points added within one
    radius of every image border and corner (windows clipped at the grid's edge)."""
    s = fuse_scene
    th = float(f32(2.5) * SF[-1])
    T = np.asarray(s["T"], np.float64)
    K = synth.TUM3_K
    uv = np.array([(1.5, 240), (638.5, 240), (320, 1.5), (320, 478.5), (1.5, 1.5), (638.5, 1.5), (1.5, 478.5),
                   (638.5, 478.5), (0.0, 100.0), (639.99, 479.99)])
    z = 3.0
    Xc = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, np.full(len(uv), z)], 1)
    Xw = (Xc - T[:3, 3]) @ T[:3, :3]
    Ow = -T[:3, :3].T @ T[:3, 3]
    d = np.linalg.norm(Xw - Ow, axis=1)
    rng = np.random.default_rng(3)
    lvl = rng.integers(0, 8, len(uv))
    mp = s["mp"]
    ext = [np.concatenate([a[:300], b]) for a, b in zip(
        (mp["valid"], mp["pos"], mp["normal"], mp["mind"], mp["maxd"], mp["desc"]),
        (np.ones(len(uv), np.uint8), Xw.astype(f32), ((Xw - Ow) / d[:, None]).astype(f32),
         (0.05 * d).astype(f32), (d * 1.2 ** (lvl - 0.5)).astype(f32), s["desc"][rng.integers(0, 1000, len(uv))]))]
    for t in (3.0, th):
        geo = {}
        o = R.fuse(CAM, s["T"], t, *ext, LOGSF, s["kps"], s["desc"], SF, INV, geo=geo)
        assert sum(1 for i in range(300, 300 + len(uv)) if i in geo) >= 8  # the border points reach the search
        _same(M.fuse(CAM, s["T"], t, *ext, LOGSF, s["kps"], s["desc"], SF, INV), o)


def test_fuse_no_valid_point(M, fuse_scene):
    s = fuse_scene
    none = np.zeros_like(s["mp"]["valid"])
    nf, bi, bd = M.fuse(CAM, s["T"], 3.0, *_mp(s, None, none), LOGSF, s["kps"], s["desc"], SF, INV)
    assert nf == 0 and (bi == -1).all() and (bd == 256).all()


@pytest.mark.parametrize("scale", [0.5, 1.0, 1.7])
def test_fuse_sim3(M, fuse_scene, scale):
    s = fuse_scene
    S = np.eye(4, dtype=np.float32)
    S[:3] = s["T"][:3] * f32(scale)
    o = R.fuse_sim3(CAM, S, 4.0, *_mp(s), LOGSF, s["kps"], s["desc"], SF)
    _same(M.fuse_sim3(CAM, S, 4.0, *_mp(s), LOGSF, s["kps"], s["desc"], SF), o)
    _same(M.fuse_sim3(CAM, S, 4.0, *_mp(s), LOGSF, s["kps"], s["desc"], SF), o)
    assert o[0] > 100


# ---------------------------------------------------------------- SearchBySim3
def _side(s, n=None):
    return tuple(s[k][:n] for k in ("kps", "desc", "valid", "pos", "mind", "maxd", "mp_desc", "already"))


def _sim3_ref(q, a, b, th=7.5):
    return R.search_by_sim3(CAM, q["T1"], q["T2"], q["s12"], q["R12"], q["t12"], th, *a, *b, LOGSF, SF)


@pytest.mark.parametrize("n1,n2", [(None, None), (500, None), (None, 300), (None, 0), (0, None)])
def test_sim3(M, sim3_scene, n1, n2):
    q = sim3_scene
    a, b = _side(q["side1"], n1), _side(q["side2"], n2)
    o = _sim3_ref(q, a, b)
    g = M.sim3(CAM, q["T1"], q["T2"], q["s12"], q["R12"], q["t12"], 7.5, a, b, LOGSF, SF)
    _same(g, o)
    _same(M.sim3(CAM, q["T1"], q["T2"], q["s12"], q["R12"], q["t12"], 7.5, a, b, LOGSF, SF), o)
    if n1 is None and n2 is None:
        assert len(a[0]) != len(b[0]) and a[7].sum() > 10 and b[7].sum() > 10 and o[0] > 100
    if n1 == 0 or n2 == 0:
        assert o[0] == 0


# ---------------------------------------------------------------- SearchForTriangulation
@pytest.fixture(scope="module")
def vocs():
    return {"orb": (synth.vocabulary(K=10, L=6), 4), "coarse": (synth.vocabulary(K=10, L=4), 3)}


def _tri(voc, levelsup, seed=0, n=None, n_clutter=120):
    g = synth.triangulation_scene(voc, seed, n_clutter=n_clutter)
    if n is not None:
        for k in ("kps1", "desc1", "has1", "kps2", "desc2", "has2"):
            g[k] = g[k][:n]
    fv1, fv2 = orc.bow_transform(voc, g["desc1"], levelsup)[2:], orc.bow_transform(voc, g["desc2"], levelsup)[2:]
    return g, fv1, fv2


def _tri_args(g, fv1, fv2, check_ori, has1=None):
    return (CAM, g["F12"], g["Ow1"], g["T2"], check_ori, g["kps1"], g["desc1"], g["has1"] if has1 is None else has1,
            fv1, g["kps2"], g["desc2"], g["has2"], fv2, SF, SIG)


@pytest.mark.parametrize("check_ori", [0, 1])
@pytest.mark.parametrize("which", ["orb", "coarse"])
def test_triangulation(vocs, which, check_ori):
    voc, levelsup = vocs[which]
    g, fv1, fv2 = _tri(voc, levelsup)
    if which == "coarse":
        assert np.diff(fv2[1]).max() > 64
    V = ea.Vocab(voc, max_kps=1024)
    o = R.search_for_triangulation(*_tri_args(g, fv1, fv2, check_ori))
    _same(V.search_triangulation(*_tri_args(g, fv1, fv2, check_ori)), o)
    _same(V.search_triangulation(*_tri_args(g, fv1, fv2, check_ori)), o)
    assert o[0] > 100


def test_triangulation_edges(vocs):
    voc, levelsup = vocs["coarse"]
    g, fv1, fv2 = _tri(voc, levelsup)
    V = ea.Vocab(voc, max_kps=1024)
    n, m = V.search_triangulation(*_tri_args(g, fv1, fv2, 1, has1=np.ones_like(g["has1"])))
    assert n == 0 and (m == -1).all()  # every KF1 feature holds a map point
    e = (np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    assert V.search_triangulation(*_tri_args(g, e, fv2, 1))[0] == 0  # empty FeatureVector
    assert V.search_triangulation(*_tri_args(g, fv1, e, 1))[0] == 0


def _one_node_pair(n2):
    """KF2 with n2 features in one vocabulary node, all on the image row y = 200; KF1 with 16 features
    on that row carrying descriptors of KF2 features; horizontal epipolar lines."""
    rng = np.random.default_rng(n2)
    k2 = np.zeros(n2, ea.KP_DTYPE)
    k2["x"], k2["y"], k2["octave"] = rng.uniform(5, 630, n2), 200.0, rng.integers(0, 8, n2)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    k1 = np.zeros(16, ea.KP_DTYPE)
    k1["x"], k1["y"] = rng.uniform(5, 630, 16), 200.0
    src = rng.permutation(n2)[:16]
    src[0] = n2 - 1  # the last feature of the node takes part
    d1 = synth._flip_bits(d2[src].copy(), 5, rng)
    d2[src[1]] = d2[src[2]]  # a tie between two KF2 features
    F = np.array([[0, 0, 0], [0, 0, 1], [0, -1, 0]], np.float32)
    T2 = np.eye(4, dtype=np.float32)
    T2[:3, 3] = (-0.5, 0.0, 0.25)
    fv1 = (np.array([5], np.int32), np.array([0, 16], np.int32), np.arange(16, dtype=np.int32))
    fv2 = (np.array([5], np.int32), np.array([0, n2], np.int32), rng.permutation(n2).astype(np.int32))
    return (CAM, F, np.zeros(3, np.float32), T2, 0, k1, d1, np.zeros(16, np.uint8), fv1, k2, d2,
            np.zeros(n2, np.uint8), fv2, SF, SIG)


def _csr(fvs, F, cap):
    ids, st, ft, nn = np.zeros((F, cap), np.int32), np.zeros((F, cap + 1), np.int32), \
        np.zeros((F, cap), np.int32), np.zeros(F, np.int32)
    for f, (a, b, c) in enumerate(fvs):
        nn[f] = len(a)
        ids[f, :len(a)], st[f, :len(b)], ft[f, :len(c)] = a, b, c
    return ids, st, ft, nn


def _tri_batch(V, cases, cap, check_ori):
    """cases: argument tuples of R.search_for_triangulation; -> (match [F][cap], nmatches [F]) of the
    batched call, the output pre-filled with a sentinel."""
    import torch
    dev = torch.device("cuda", 0)
    F = len(cases)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kps = [np.zeros((F, cap), ea.KP_DTYPE) for _ in range(2)]
    desc = [np.zeros((F, cap, 32), np.uint8) for _ in range(2)]
    has = [np.zeros((F, cap), np.uint8) for _ in range(2)]
    F12, Ow1, T2 = np.zeros((F, 9), f32), np.zeros((F, 3), f32), np.zeros((F, 16), f32)
    n1 = np.zeros(F, np.int32)
    for f, c in enumerate(cases):
        F12[f], Ow1[f], T2[f] = np.ravel(c[1]), np.ravel(c[2]), np.ravel(c[3])
        n1[f] = len(c[5])
        for k, (kk, dd, hh) in enumerate(((c[5], c[6], c[7]), (c[9], c[10], c[11]))):
            kps[k][f, :len(kk)], desc[k][f, :len(kk)], has[k][f, :len(kk)] = kk, dd, hh
    i1, s1, f1, nn1 = _csr([c[8] for c in cases], F, cap)
    i2, s2, f2, nn2 = _csr([c[12] for c in cases], F, cap)
    keep = [t(F12), t(Ow1), t(T2), t(n1), t(kps[0].view(np.uint8).reshape(F, cap, 28)), t(desc[0]), t(has[0]), t(nn1),
            t(i1), t(s1), t(f1), t(kps[1].view(np.uint8).reshape(F, cap, 28)), t(desc[1]), t(has[1]), t(nn2), t(i2),
            t(s2), t(f2)]
    match = torch.full((F, cap), -7, dtype=torch.int32, device=dev)
    nm = torch.full((F,), -7, dtype=torch.int32, device=dev)
    p = [x.data_ptr() for x in keep]
    V.search_triangulation_batch_device(CAM, check_ori, F, cap, p[0], p[1], p[2], p[3], tuple(p[4:11]),
                                        tuple(p[11:18]), SF, SIG, match.data_ptr(), nm.data_ptr())
    torch.cuda.synchronize()
    return match.cpu().numpy(), nm.cpu().numpy()


def test_triangulation_node_capacity(vocs):
    """a node of exactly 1024 KF2 features works; 1025 is reported (EAO_E_CAPACITY), single and batched"""
    voc, _ = vocs["coarse"]
    V = ea.Vocab(voc, max_kps=2048, max_batch=2)
    ok, over = _one_node_pair(1024), _one_node_pair(1025)
    o = R.search_for_triangulation(*ok)
    assert o[0] >= 8
    _same(V.search_triangulation(*ok), o)
    with pytest.raises(ea.EaoError, match="1024"):
        V.search_triangulation(*over)
    hm, hn = _tri_batch(V, [ok, over], 2048, 0)
    assert hn[0] == o[0] and np.array_equal(hm[0, :16], o[1]) and hn[1] == ea.EAO_E_CAPACITY


# ---------------------------------------------------------------- batched forms
SIZES = [1000, 0, 1, 64, 333, 1024]


def test_triangulation_batch_device(vocs):
    voc, levelsup = vocs["orb"]
    cap = 1024
    cases = []
    for f, n in enumerate(SIZES):
        g, fv1, fv2 = _tri(voc, levelsup, seed=f, n=n, n_clutter=260)
        assert len(g["kps1"]) == n and len(g["kps2"]) == n
        cases.append(_tri_args(g, fv1, fv2, 1))
    V = ea.Vocab(voc, max_kps=cap, max_batch=len(SIZES))
    hm, hn = _tri_batch(V, cases, cap, 1)
    hm2, hn2 = _tri_batch(V, cases, cap, 1)
    assert np.array_equal(hm, hm2) and np.array_equal(hn, hn2)
    for f, n in enumerate(SIZES):
        no, mo = R.search_for_triangulation(*cases[f])
        assert hn[f] == no and np.array_equal(hm[f, :n], mo), f
        assert (hm[f, n:] == -1).all()  # the whole slot is initialised to "unmatched"
        if n > 0:
            _same(V.search_triangulation(*cases[f]), (no, mo))
    assert hn.max() > 100


def test_fuse_batch_device(M):
    import torch
    dev = torch.device("cuda", 0)
    F, cap, mp_cap = len(SIZES), 1024, 640
    n_mp = [600, 17, 1, 64, 333, 640]
    scenes = [synth.fuse_scene(10 + f, n_mp=n_mp[f], n_kf=SIZES[f]) for f in range(F)]
    kps, desc = np.zeros((F, cap), ea.KP_DTYPE), np.zeros((F, cap, 32), np.uint8)
    T = np.zeros((F, 16), f32)
    valid, pos, nrm = np.zeros((F, mp_cap), np.uint8), np.zeros((F, mp_cap, 3), f32), np.zeros((F, mp_cap, 3), f32)
    mind, maxd, md = np.zeros((F, mp_cap), f32), np.zeros((F, mp_cap), f32), np.zeros((F, mp_cap, 32), np.uint8)
    for f, s in enumerate(scenes):
        n, m = SIZES[f], n_mp[f]
        assert len(s["kps"]) == n and len(s["mp"]["valid"]) == m
        kps[f, :n], desc[f, :n], T[f] = s["kps"], s["desc"], np.ravel(s["T"])
        for dst, src in zip((valid, pos, nrm, mind, maxd, md), _mp(s)):
            dst[f, :m] = src
    # past the count: valid points that would match if they were read
    valid[1, 17:40], pos[1, 17:40], md[1, 17:40] = 1, pos[0, :23], md[0, :23]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keep = [t(T), t(np.array(n_mp, np.int32)), t(valid), t(pos), t(nrm), t(mind), t(maxd), t(md),
            t(np.array(SIZES, np.int32)), t(kps.view(np.uint8).reshape(F, cap, 28)), t(desc)]
    p = [x.data_ptr() for x in keep]
    outs = []
    for _ in range(2):
        bi = torch.full((F, mp_cap), -7, dtype=torch.int32, device=dev)
        bd = torch.full((F, mp_cap), -7, dtype=torch.int32, device=dev)
        nf = torch.full((F,), -7, dtype=torch.int32, device=dev)
        s_ = torch.cuda.Stream(dev)
        s_.wait_stream(torch.cuda.current_stream())
        M.fuse_batch_device(CAM, F, p[0], 3.0, mp_cap, p[1], p[2], p[3], p[4], p[5], p[6], p[7], float(LOGSF), cap,
                            p[8], p[9], p[10], SF, INV, bi.data_ptr(), bd.data_ptr(), nf.data_ptr(), s_.cuda_stream)
        torch.cuda.synchronize()
        outs.append((bi.cpu().numpy(), bd.cpu().numpy(), nf.cpu().numpy()))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    hi, hd, hn = outs[0]
    for f, s in enumerate(scenes):
        m = n_mp[f]
        o = R.fuse(CAM, s["T"], 3.0, *_mp(s), LOGSF, s["kps"], s["desc"], SF, INV)
        assert hn[f] == o[0] and np.array_equal(hi[f, :m], o[1]) and np.array_equal(hd[f, :m], o[2]), f
        assert (hi[f, m:] == -7).all() and (hd[f, m:] == -7).all()  # entries past the count are left untouched
        _same(M.fuse(CAM, s["T"], 3.0, *_mp(s), LOGSF, s["kps"], s["desc"], SF, INV), o)
    assert hn.max() > 100


# ---------------------------------------------------------------- bad arguments
def test_bad_arguments(M, fuse_scene, sim3_scene, vocs):
    s, q = fuse_scene, sim3_scene
    lib = ea.lib()
    bad = (ea.EAO_E_ARG, ea.EAO_E_CAPACITY)
    c = ctypes
    P, cam, fl = ea.P, c.byref(CAM), c.c_float
    v, pos, nrm, mn, mx, md = [np.ascontiguousarray(a) for a in _mp(s)]
    kps, desc, T = np.ascontiguousarray(s["kps"]), np.ascontiguousarray(s["desc"]), np.ascontiguousarray(s["T"])
    n, nk = len(v), len(kps)
    bi, bd = np.zeros(2048, np.int32), np.zeros(2048, np.int32)

    def fuse(n_mp=n, n_kf=nk, pos_=pos, kps_=kps, nlevels=8, T_=T, out=bi):
        return lib.eao_match_fuse(M.h, cam, P(T_), fl(3.0), n_mp, P(v), P(pos_), P(nrm), P(mn), P(mx), P(md),
                                  fl(LOGSF), n_kf, P(kps_), P(desc), nlevels, P(SF), P(INV), P(out), P(bd))
    assert fuse() >= 0
    assert fuse(pos_=None) in bad and fuse(kps_=None) in bad and fuse(T_=None) in bad and fuse(out=None) in bad
    assert fuse(n_mp=-1) in bad and fuse(n_kf=-1) in bad
    assert fuse(nlevels=33) in bad and fuse(nlevels=0) in bad
    big = np.zeros(1025, ea.KP_DTYPE)
    assert lib.eao_match_fuse(M.h, cam, P(T), fl(3.0), n, P(v), P(pos), P(nrm), P(mn), P(mx), P(md), fl(LOGSF), 1025,
                              P(big), P(np.zeros((1025, 32), np.uint8)), 8, P(SF), P(INV), P(bi), P(bd)) in bad
    assert lib.eao_match_fuse_sim3(M.h, cam, None, fl(4.0), n, P(v), P(pos), P(nrm), P(mn), P(mx), P(md), fl(LOGSF),
                                   nk, P(kps), P(desc), 8, P(SF), P(bi), P(bd)) in bad
    assert lib.eao_match_fuse_sim3(M.h, cam, P(T), fl(4.0), n, P(v), P(pos), P(nrm), P(mn), P(mx), P(md), fl(LOGSF),
                                   nk, P(kps), P(desc), 33, P(SF), P(bi), P(bd)) in bad
    a, b = _side(q["side1"]), _side(q["side2"])
    with pytest.raises(ea.EaoError):
        M.sim3(CAM, q["T1"], q["T2"], q["s12"], q["R12"], q["t12"], 7.5, a, b, LOGSF, np.ones(33, f32))
    small = ea.Matcher(max_kps=256, max_batch=2)
    with pytest.raises(ea.EaoError):  # n > max_kps
        small.sim3(CAM, q["T1"], q["T2"], q["s12"], q["R12"], q["t12"], 7.5, a, b, LOGSF, SF)
    with pytest.raises(ea.EaoError):
        small.fuse(CAM, s["T"], 3.0, *_mp(s), LOGSF, s["kps"], s["desc"], SF, INV)
    # batched: the argument checks come before any pointer is used
    one = c.c_void_p(16)
    args = lambda nsearch, mp_cap, cap, nlevels, T_=one: (
        M.h, cam, nsearch, T_, fl(3.0), mp_cap, one, one, one, one, one, one, one, fl(LOGSF), cap, one, one, one,
        nlevels, P(SF), P(INV), one, one, one, None)
    assert lib.eao_match_fuse_batch_device(*args(7, 640, 1024, 8)) in bad     # nsearch > max_batch
    assert lib.eao_match_fuse_batch_device(*args(0, 640, 1024, 8)) in bad
    assert lib.eao_match_fuse_batch_device(*args(6, 2048, 1024, 8)) in bad    # slots larger than max_kps
    assert lib.eao_match_fuse_batch_device(*args(6, 640, 2048, 8)) in bad
    assert lib.eao_match_fuse_batch_device(*args(6, 640, 1024, 33)) in bad
    assert lib.eao_match_fuse_batch_device(*args(6, 640, 1024, 8, T_=None)) in bad
    voc, levelsup = vocs["coarse"]
    V = ea.Vocab(voc, max_kps=512, max_batch=2)
    g, fv1, fv2 = _tri(voc, levelsup)
    with pytest.raises(ea.EaoError):  # n > max_kps
        V.search_triangulation(*_tri_args(g, fv1, fv2, 1))
    g, fv1, fv2 = _tri(voc, levelsup, n=400)
    assert V.search_triangulation(*_tri_args(g, fv1, fv2, 1))[0] >= 0
    with pytest.raises(ea.EaoError):
        V.search_triangulation(*_tri_args(g, fv1, fv2, 1)[:13], np.ones(33, f32), np.ones(33, f32))
    targs = lambda nsearch, cap, nlevels, F_=one: (
        V.h, cam, 1, nsearch, cap, F_, one, one, one, *([one] * 14), nlevels, P(SF), P(SIG), one, one, None)
    tb = lib.eao_search_for_triangulation_batch_device
    assert tb(*targs(3, 512, 8)) in bad      # nsearch > max_batch
    assert tb(*targs(2, 1024, 8)) in bad     # cap > max_kps
    assert tb(*targs(2, 512, 33)) in bad
    assert tb(*targs(2, 512, 8, F_=None)) in bad
