"""The texture atlas without a GPU: known answers of the numpy restatement (tests/atlas_ref.py), then f2n_atlas_classify / _place / _texels and
f2n_texture_sample (csrc/octree.hip) under the wavefront emulator (tests/wave_emul) against that restatement, bit for bit (both builds use
-ffp-contract=off); the layout's properties (disjoint blocks, texel ownership, corner texels, the clamp), the exactness of bilinear
filtering for a linear function, independence of face order and wave schedule, the halving loop, the contract cases, and the PNG / OBJ
writers.  The bodies take an `Atlas` and run against the device as well (tests/test_gpu_mesh_texture.py)."""
import ctypes
import os
import struct
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import atlas_ref as ar  # noqa: E402
import mesh_ref as mr  # noqa: E402
import mesh_simplify_ref as msr  # noqa: E402

F32 = np.float32
INVALID = -1  # F2N_ERR_INVALID_ARG
_f, _i = ctypes.c_float, ctypes.c_int
# Linear exactness (check_linear): the largest |sample - c| of the RESTATEMENT against c in fp64 over all the meshes below was 9.61e-7
# (the 17^3 sphere, 249 984 lookups; colours of magnitude <= 2; measured once on the CPU); the bar is 4 times that.
LINEAR_BOUND = 3.9e-6


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


class EmulError(RuntimeError):
    def __init__(self, name, rc):
        RuntimeError.__init__(self, "%s failed with status %d" % (name, rc))
        self.rc = rc


def _mesh(verts, faces):
    return np.ascontiguousarray(verts, F32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


def emul_classify(L, verts, faces, density, max_log=7):
    v, f = _mesh(verts, faces)
    log_s, rot = np.full(len(f), -9, np.int32), np.full(len(f), -9, np.int32)
    rc = L.f2n_atlas_classify(None, len(v), len(f), _vp(v), _vp(f), _f(density), max_log, _vp(log_s), _vp(rot))
    if rc != 0:
        raise EmulError("f2n_atlas_classify", rc)
    return log_s, rot


def emul_place(L, log_s, rot, lay):
    nf = len(log_s)
    uv = np.full((nf, 3, 2), -9, F32)
    off = np.ascontiguousarray(lay["offsets"], np.int64)
    rc = L.f2n_atlas_place(None, nf, len(lay["block_log"]), int(lay["size"]), _vp(np.ascontiguousarray(log_s, np.int32)),
                           _vp(np.ascontiguousarray(rot, np.int32)), _vp(np.ascontiguousarray(lay["slot"], np.int32)), _vp(off), _vp(uv))
    if rc != 0:
        raise EmulError("f2n_atlas_place", rc)
    return uv


def emul_texels(L, verts, faces, blocks, size, clamp, bands=None):
    """MeshAtlasTexels of csrc/host/RendererQuery.cpp; bands: the row ranges of the launches (default: one)"""
    v, f = _mesh(verts, faces)
    S, B = int(size), len(blocks["block_log"])
    tf, tb, tp = np.full((S, S), -9, np.int32), np.full((S, S, 3), -9, F32), np.full((S, S, 3), -9, F32)
    off, bl = np.ascontiguousarray(blocks["offsets"], np.int64), np.ascontiguousarray(blocks["block_log"], np.int32)
    bf, rot = np.ascontiguousarray(blocks["block_faces"], np.int32), np.ascontiguousarray(blocks["rot"], np.int32)
    for y0, y1 in bands or [(0, S)]:
        rc = L.f2n_atlas_texels(None, len(v), len(f), _vp(v), _vp(f), B, S, _vp(off), _vp(bl), _vp(bf), _vp(rot), int(clamp), y0, y1, _vp(tf), _vp(tb),
                                _vp(tp))
        if rc != 0:
            raise EmulError("f2n_atlas_texels", rc)
    return tf, tb, tp


def emul_sample(L, tex, uv):
    tex = np.ascontiguousarray(tex, F32)
    uv = np.ascontiguousarray(uv, F32).reshape(-1, 2)
    out = np.full((len(uv), tex.shape[2]), -9, F32)
    rc = L.f2n_texture_sample(None, tex.shape[0], tex.shape[2], _vp(tex), ctypes.c_int64(len(uv)), _vp(uv), _vp(out))
    if rc != 0:
        raise EmulError("f2n_texture_sample", rc)
    return out


class Atlas:
    """atlas(v, f, density, max_size=8192, max_log=7) -> (uv, size, blocks, density_used) with blocks a dict of numpy arrays (offsets,
    block_log, block_faces, log_s, rot, slot); texels(v, f, blocks, size, clamp) -> (tex_face, tex_bary, tex_pos); sample(tex, uv)"""
    def __init__(self, atlas, texels, sample):
        self.atlas, self.texels, self.sample = atlas, texels, sample


def ref_atlas():
    def atlas(v, f, density, max_size=8192, max_log=7):
        uv, size, lay, d = ar.atlas(v, f, density, max_size, max_log)
        return uv, size, lay, d
    return Atlas(atlas, lambda v, f, b, size, clamp: ar.texels(v, f, b["rot"], dict(b, size=size), clamp), ar.sample)


def emul_atlas(L):
    """MeshAtlas of csrc/host/RendererQuery.cpp call for call, numpy (atlas_ref.layout) in the place of its torch plumbing"""
    def atlas(v, f, density, max_size=8192, max_log=7):
        return ar.atlas(v, f, density, max_size, max_log, classify_fn=lambda *a: emul_classify(L, *a), place_fn=lambda *a: emul_place(L, *a))
    return Atlas(atlas, lambda v, f, b, size, clamp: emul_texels(L, v, f, b, size, clamp), lambda t, uv: emul_sample(L, t, uv))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all()


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
_cache = {}


def right_triangles(legs, seed=0):
    """separate right isosceles triangles of the given legs, each rotated and shifted at random: at density 1 a leg L gives l = L"""
    rng = np.random.default_rng(seed)
    v, f = [], []
    for k, leg in enumerate(legs):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        tri = np.array([[0, 0, 0], [leg, 0, 0], [0, leg, 0]], np.float64) @ q.T + rng.uniform(-5, 5, 3)
        v.append(np.roll(tri, k % 3, axis=0))  # (the right angle sits at corner k % 3)
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    return np.concatenate(v).astype(F32), np.array(f, np.int32)


def make_mesh(name):
    """(verts, faces, density, max_log)"""
    if name in _cache:
        return _cache[name]
    if name == "octahedron":
        v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1.5, 0], [0, -1.5, 0], [0, 0, 2], [0, 0, -2]], F32) * F32(3)
        f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
        out = (v, f, 2.0, 7)
    elif name == "single":
        out = (np.array([[0.1, 0.2, 0.3], [4.0, 0.5, 0.1], [1.0, 3.0, 2.0]], F32), np.array([[0, 1, 2]], np.int32), 3.0, 7)
    elif name == "empty":
        out = (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), 1.0, 7)
    elif name in ("sphere17", "sphere17_s2"):
        v, f = mr.marching_tets(mr.sphere_grid(17, 6.4), 0.0)
        v, f = _mesh(v, f)
        if name == "sphere17_s2":
            v, f, _ = msr.simplify(v, f, 2.0, lo=(0.0, 0.0, 0.0))
        out = (v, f, 1.0 if name == "sphere17" else 2.0, 7)
    elif name == "strip":  # 2 x 24 quads, stretched so that the longest edge is not always the diagonal
        gx, gy = np.meshgrid(np.arange(25), np.arange(3), indexing="xy")
        v = np.stack([gx.reshape(-1) * 0.7, gy.reshape(-1) * 1.9, 0.1 * gx.reshape(-1) ** 1.5], 1).astype(F32)
        q = np.array([[r * 25 + c, r * 25 + c + 1, (r + 1) * 25 + c, (r + 1) * 25 + c + 1] for r in range(2) for c in range(24)])
        f = np.concatenate([q[:, [0, 1, 2]], q[:, [1, 3, 2]]]).astype(np.int32)
        out = (v, f, 4.0, 7)
    elif name == "odd":  # classes 2^3, 2^4 and 2^5 with odd counts (3, 5, 1), class 2^2 with an even one
        v, f = right_triangles([4.9] * 3 + [12.9] * 5 + [28.9] + [0.9] * 4, seed=1)
        rng = np.random.default_rng(2)
        out = (v, f[rng.permutation(len(f))], 1.0, 7)
    elif name == "degenerate":
        v, f = right_triangles([5.0, 13.0, 5.0, 2.0, 7.0, 3.0], seed=3)
        v[6] = np.nan                      # face 2: a vertex that is not finite
        v[10] = v[9]                       # face 3: zero area
        f[4] = [12, 13, 99]                # face 4: an index out of range
        f = np.concatenate([f, [[0, 0, 1]]]).astype(np.int32)  # a repeated index: zero area
        out = (v, f, 1.0, 7)
    elif name == "classes":  # block sides 4 ... 128 and one face beyond the cap
        v, f = right_triangles([0.9, 4.9, 12.9, 28.9, 60.9, 124.9, 300.0, 0.2, 4.1, 12.95], seed=4)
        out = (v, f, 1.0, 7)
    else:
        raise KeyError(name)
    for a in out[:2]:
        a.setflags(write=False)
    _cache[name] = out
    return out


MESHES = ["octahedron", "single", "empty", "sphere17", "sphere17_s2", "strip", "odd", "degenerate", "classes"]
_ref_cache = {}


def reference(name):
    """the restatement's atlas and both texel maps of a mesh, computed once"""
    if name not in _ref_cache:
        v, f, density, max_log = make_mesh(name)
        uv, size, lay, d = ar.atlas(v, f, density, 8192, max_log)
        t0, t1 = ar.texels(v, f, lay["rot"], lay, 0), ar.texels(v, f, lay["rot"], lay, 1)
        for a in (uv,) + t0 + t1:
            a.setflags(write=False)
        _ref_cache[name] = (uv, size, lay, d, t0, t1)
    return _ref_cache[name]


# ---- known answers of the restatement ---------------------------------------------------------------------------------------------
def test_restatement_known_answers():
    v, f = np.array([[1, 2, 3], [6, 2, 3], [1, 7, 3]], F32), np.array([[0, 1, 2]], np.int32)  # corner 0 is the right angle: BC is longest
    assert [x.tolist() for x in ar.classify(v, f, 1.0)] == [[3], [0]]
    assert [x.tolist() for x in ar.classify(np.roll(v, 1, 0), f, 1.0)] == [[3], [1]]
    assert [x.tolist() for x in ar.classify(np.roll(v, 2, 0), f, 1.0)] == [[3], [2]]
    eq = np.array([[0, 0, 0], [1, 0, 0], [0.5, np.sqrt(0.75), 0]], F32) * F32(8)  # ties go to the lowest corner
    assert ar.classify(np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 0]], F32) * 2, [[0, 1, 2]], 1.0)[1].tolist() == [0]
    assert ar.classify(eq, [[0, 1, 2]], 1.0)[1][0] in (0, 1, 2)
    # l = 5 -> need 8 -> 2^3; l = 5.0001 -> 9 -> 2^4; the cap
    assert ar.classify(v, f, 1.0)[0][0] == 3 and ar.classify(v, f, 1.001)[0][0] == 4 and ar.classify(v, f, 100.0, 5)[0][0] == 5
    assert [a.tolist() for a in ar.morton_decode(np.array([0, 1, 2, 3, 4, 16, 0b110110]))] == [[0, 1, 0, 1, 2, 4, 6], [0, 0, 1, 1, 0, 0, 5]]
    x, y = np.meshgrid(np.arange(37), np.arange(41))
    dx, dy = ar.morton_decode(ar.morton_encode(x, y))
    assert (dx == x).all() and (dy == y).all() and ar.morton_encode(3, 5) == 0b100111
    # three faces of class 3, one of class 2: blocks (3: f0 f1), (3: f2 -), (2: f3 -) at offsets 0, 64, 128, total 144 -> S = 16
    lay = ar.layout(np.array([3, 3, 2, 3], np.int32))
    assert lay["block_log"].tolist() == [3, 3, 2] and lay["block_faces"].tolist() == [[0, 1], [3, -1], [2, -1]]
    assert lay["offsets"].tolist() == [0, 64, 128, 144] and lay["size"] == 16 and lay["slot"].tolist() == [0, 1, 4, 2]
    uv = ar.place(np.array([3, 3, 2, 3], np.int32), np.array([0, 1, 0, 2], np.int32), lay) * 16
    assert uv[0].tolist() == [[0.5, 0.5], [5.5, 0.5], [0.5, 5.5]]           # lower chart of block 0
    assert uv[1].tolist() == [[7.5, 2.5], [7.5, 7.5], [2.5, 7.5]]           # upper chart, rot 1: corner 1 at the right angle
    assert uv[3].tolist() == [[13.5, 0.5], [8.5, 5.5], [8.5, 0.5]]          # block 1 at (8, 0), rot 2: corner 2 at the right angle
    assert uv[2].tolist() == [[0.5, 8.5], [1.5, 8.5], [0.5, 9.5]]           # block 2 at (0, 8)
    tex = np.arange(25, dtype=F32).reshape(5, 5, 1)
    assert ar.sample(tex, [[0.5, 0.5], [0.3, 0.1], [0.0, 0.0], [2.0, 0.5], [np.nan, 0.5]])[:, 0].tolist() == [12.0, 1.0, 0.0, 14.0, 0.0]


# ---- the bodies ---------------------------------------------------------------------------------------------------------------------
def check_against_restatement(A, name):
    """the atlas and both texel maps of a mesh, bit for bit with the restatement; returns them"""
    v, f, density, max_log = make_mesh(name)
    uv, size, lay, d, t0, t1 = reference(name)
    guv, gsize, gb, gd = A.atlas(v, f, density, 8192, max_log)
    assert gsize == size and gd == d and same(guv, uv)
    for k in ("offsets", "block_log", "block_faces", "log_s", "rot", "slot"):
        assert same(np.asarray(gb[k]).reshape(lay[k].shape), lay[k]), k
    g0, g1 = A.texels(v, f, gb, gsize, 0), A.texels(v, f, gb, gsize, 1)
    for got, ref in ((g0, t0), (g1, t1)):
        for a, b in zip(got, ref):
            assert same(a, b)
    return guv, gsize, gb, g0, g1


def check_properties(name, uv, S, b, t0, t1):
    """(a) - (e) on any implementation's outputs"""
    v, f, density, max_log = make_mesh(name)
    nf, B = len(f), len(b["block_log"])
    offsets, block_log, block_faces = np.asarray(b["offsets"]), np.asarray(b["block_log"]), np.asarray(b["block_faces"]).reshape(-1, 2)
    log_s, rot = np.asarray(b["log_s"]), np.asarray(b["rot"])
    total = int(offsets[B])
    # (b) the atlas side
    assert S >= 4 and S & (S - 1) == 0 and S * S >= total and (S == 4 or (S // 2) ** 2 < total)
    # (a) every texel below the total lies in exactly one block; blocks are disjoint and inside the atlas
    x0, y0 = ar.morton_decode(offsets[:B])
    s = 1 << block_log.astype(np.int64)
    paint = np.zeros((S, S), np.int64)
    for k in range(B):
        assert x0[k] + s[k] <= S and y0[k] + s[k] <= S and offsets[k] % (s[k] * s[k]) == 0
        paint[y0[k]:y0[k] + s[k], x0[k]:x0[k] + s[k]] += 1
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    assert (paint == (ar.morton_encode(xx, yy) < total)).all()
    assert (np.diff(block_log) <= 0).all() and sorted(block_faces[block_faces >= 0].tolist()) == list(range(nf))
    good = (rot & ar.DEGENERATE) == 0
    tf0, bary0, pos0 = t0
    tf1, bary1, pos1 = t1
    assert (tf0 == tf1).all() and (tf0[paint == 0] == -1).all()
    # (d) owned texels per face
    counts = np.bincount(tf0[tf0 >= 0], minlength=nf) if nf else np.zeros(0, np.int64)
    side = 1 << log_s.astype(np.int64)
    upper = (np.asarray(b["slot"]) & 1) != 0
    assert (counts == np.where(good, np.where(upper, side * (side - 1) // 2, side * (side + 1) // 2), 0)).all()
    for k in range(nf):
        assert log_s[k] == block_log[b["slot"][k] >> 1] and block_faces[b["slot"][k] >> 1, b["slot"][k] & 1] == k
    # (c) the uv corners are texel centres of the face's own block; there the map names the face with a one-hot weight
    t = uv.astype(np.float64) * S - 0.5
    assert (t == np.round(t)).all()
    t = t.astype(np.int64)
    bx, by = x0[np.asarray(b["slot"]) >> 1], y0[np.asarray(b["slot"]) >> 1]
    assert ((t[:, :, 0] >= bx[:, None]) & (t[:, :, 0] < (bx + side)[:, None]) & (t[:, :, 1] >= by[:, None]) & (t[:, :, 1] < (by + side)[:, None])).all()
    for j in range(3):
        at = (t[good, j, 1], t[good, j, 0])
        assert (tf0[at] == np.nonzero(good)[0]).all()
        for bary in (bary0, bary1):
            assert (bary[at] == np.eye(3, dtype=F32)[j]).all()
        assert same(pos0[at], v[f[good, j]]) and same(pos1[at], v[f[good, j]])
    # (the orientation is kept: uv triangles all turn the same way in the image)
    e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    assert ((e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) > 0).all()
    # (e) the clamp
    own = tf0 >= 0
    inside = (bary0 >= 0).all(-1) & own
    assert (bary1[own] >= 0).all() and same(bary1[inside], bary0[inside]) and same(pos1[inside], pos0[inside])
    ssum = bary1[own].astype(np.float64).sum(-1)
    assert (np.abs(ssum - 1.0) <= 2 * np.finfo(F32).eps).all()
    assert ((bary0[own & ~inside] < 0).any(-1)).all() and (bary0[~own] == 0).all() and (pos1[~own] == 0).all()
    if good.any():  # a clamped gutter texel lies on the face: within its bounding box
        P = v[f[good]]
        lo_f, hi_f = np.full((nf, 3), -np.inf), np.full((nf, 3), np.inf)
        lo_f[good], hi_f[good] = P.min(1), P.max(1)
        tol = 1e-5 * np.abs(P).max()
        assert (pos1[own] >= lo_f[tf0[own]] - tol).all() and (pos1[own] <= hi_f[tf0[own]] + tol).all()
    return good


def sample_points(name, uv, good, n_random=50, seed=7):
    """barycentrics per good face: its corners, its edge midpoints and n_random interior points -> (face ids, weights [N,3], uv [N,2])"""
    rng = np.random.default_rng(seed)
    fixed = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]])
    ids = np.nonzero(good)[0]
    w = rng.dirichlet([1.0, 1.0, 1.0], (len(ids), n_random))
    w = np.concatenate([np.broadcast_to(fixed, (len(ids), 6, 3)), w], 1)  # [G, 6 + n, 3]
    face = np.repeat(ids, w.shape[1])
    w = w.reshape(-1, 3)
    at = (uv.astype(np.float64)[face] * w[:, :, None]).sum(1)
    return face, w, at.astype(F32)


def linear_colour(name):
    v = make_mesh(name)[0]
    fin = v[np.isfinite(v).all(1)].astype(np.float64) if len(v) else np.zeros((1, 3))
    mid, ext = (fin.max(0) + fin.min(0)) / 2, max(float((fin.max(0) - fin.min(0)).max()), 1e-3)
    a = np.array([[0.9, -0.5, 0.3], [-0.4, 0.8, 0.6], [0.7, 0.2, -0.9]]) / ext
    return lambda p: (np.asarray(p, np.float64) - mid) @ a + np.array([0.5, 0.4, 0.6])


def check_linear(A, name, uv, S, good, t0, n_random=50):
    """(f) the texture of c(P) = a.P + b baked from tex_pos (clamp 0), looked up at points of every face: the implementation equals the
    restatement bit for bit, and the restatement equals c in fp64 within LINEAR_BOUND = 3.9e-6, four times the largest error observed
    (9.61e-7, on the 17^3 sphere).  Returns the largest error of the restatement."""
    v, f = make_mesh(name)[:2]
    c = linear_colour(name)
    tex = np.where(t0[0][..., None] >= 0, c(t0[2]), 0.0).astype(F32)
    face, w, at = sample_points(name, uv, good, n_random)
    if not len(face):
        return 0.0
    ref = ar.sample(tex, at)
    assert same(A.sample(tex, at), ref)
    want = c((v[f[face]].astype(np.float64) * w[:, :, None]).sum(1))
    err = float(np.abs(ref.astype(np.float64) - want).max())
    print("%s: linear colour, %d lookups, atlas %d, max error %.3g" % (name, len(face), S, err))
    assert err <= LINEAR_BOUND, err
    return err


def check_mesh_case(A, name, n_random=50):
    uv, S, b, t0, t1 = check_against_restatement(A, name)
    good = check_properties(name, uv, S, b, t0, t1)
    return check_linear(A, name, uv, S, good, t0, n_random)


def check_face_order(A, name, seed=5):
    """(g) a permutation of the faces: classes and rotations follow it, every property holds again and the same points of the surface
    carry the same linear colour"""
    v, f, density, max_log = make_mesh(name)
    perm = np.random.default_rng(seed).permutation(len(f))
    ref = reference(name)
    uv, S, b, d = A.atlas(v, f[perm], density, 8192, max_log)
    assert same(np.asarray(b["log_s"]), ref[2]["log_s"][perm]) and same(np.asarray(b["rot"]), ref[2]["rot"][perm]) and S == ref[1] and d == ref[3]
    # the chart of a face keeps its shape: the corner offsets from the right angle agree up to the lower / upper flip
    shape = lambda u, r: np.abs(u - np.take_along_axis(u, (r & 3)[:, None, None].astype(np.int64).repeat(2, 2), 1))  # noqa: E731
    assert same(shape(uv, np.asarray(b["rot"])), shape(ref[0], ref[2]["rot"])[perm])
    key = name + "@perm"
    _cache[key] = (v, np.ascontiguousarray(f[perm]), density, max_log)
    try:
        t0, t1 = A.texels(v, f[perm], b, S, 0), A.texels(v, f[perm], b, S, 1)
        good = check_properties(key, uv, S, b, t0, t1)
        check_linear(A, key, uv, S, good, t0, 8)
    finally:
        del _cache[key]


def check_halving(A):
    """(i) the 17^3 sphere at density 4 into 64 x 64: the density is halved the fewest times that fit"""
    v, f, _, max_log = make_mesh("sphere17_s2")
    uv, S, b, d = A.atlas(v, f, 4.0, 64, max_log)
    n = int(round(np.log2(4.0 / d)))
    assert d == 4.0 / 2 ** n and n >= 1 and S <= 64
    assert ar.layout(ar.classify(v, f, d * 2, max_log)[0], max_log)["size"] > 64 and ar.layout(ar.classify(v, f, d, max_log)[0], max_log)["size"] <= 64
    assert same(uv, ar.atlas(v, f, 4.0, 64, max_log)[0])
    return n, d, S


def check_contract(A):
    """(j) the ValueErrors of the fit"""
    v, f, density, max_log = make_mesh("octahedron")
    for bad in (100, 0, 3, -8):
        with pytest.raises(ValueError):
            A.atlas(v, f, density, bad, max_log)
    with pytest.raises(ValueError):
        A.atlas(v, f, density, 4, max_log)  # 8 faces: four blocks of 4 x 4 need 8 x 8
    uv, S, b, d = A.atlas(v, f, 1000.0, 8, max_log)  # all-minimum fits exactly
    assert S == 8 and d < 1000.0 and (np.asarray(b["log_s"]) == 2).all()
    uv, S, b, d = A.atlas(v[:0], f[:0], 1.0, 4, max_log)
    assert S == 4 and len(uv) == 0 and np.asarray(b["offsets"]).tolist() == [0]
    t = A.texels(v[:0], f[:0], b, S, 1)
    assert (t[0] == -1).all() and (t[1] == 0).all() and (t[2] == 0).all()


def check_sample(A):
    """(m) clamp to the edge, uv that are not finite, a side that is no power of two, several channels"""
    rng = np.random.default_rng(9)
    for S, C in ((5, 1), (5, 3), (1, 2), (8, 4), (33, 3)):
        tex = rng.standard_normal((S, S, C)).astype(F32)
        uv = np.concatenate([rng.uniform(-0.3, 1.3, (200, 2)), [[0, 0], [1, 1], [0, 1], [-5, 0.5], [0.5, 7], [np.nan, 0.5], [0.5, np.inf],
                                                                  [-np.inf, np.nan], [0.5, 0.5], [1e30, -1e30]]]).astype(F32)
        out = A.sample(tex, uv)
        assert same(out, ar.sample(tex, uv))
        assert (out[-5:-2] == 0).all() and same(out[200], tex[0, 0]) and same(out[201], tex[S - 1, S - 1]) and same(out[202], tex[S - 1, 0])
        assert same(out[-1], tex[0, S - 1])
        centres = (np.stack(np.meshgrid(np.arange(S), np.arange(S)), -1).reshape(-1, 2).astype(np.float64) + 0.5) / S
        if S & (S - 1) == 0:  # (a power of two: u S is exact, the texel centres give the texels)
            assert same(A.sample(tex, centres.astype(F32)), tex.reshape(-1, C))
    assert A.sample(np.zeros((4, 4, 3), F32), np.zeros((0, 2), F32)).shape == (0, 3)


# ---- the restatement and the emulated wavefront -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_restatement_properties(name):
    check_mesh_case(ref_atlas(), name)


@pytest.mark.parametrize("name", MESHES)
def test_emulated_against_restatement(emul, name):
    check_mesh_case(emul_atlas(emul), name)


def test_classes_span_the_range():
    assert sorted(set(reference("classes")[2]["log_s"].tolist())) == [2, 3, 4, 5, 6, 7]
    lay = reference("odd")[2]
    assert np.bincount(lay["log_s"]).tolist() == [0, 0, 4, 3, 5, 1] and (lay["block_faces"][:, 1] < 0).sum() == 3
    deg = reference("degenerate")[2]  # faces 2, 3, 4 and 6 are degenerate; face k of right_triangles has its right angle at corner k % 3
    assert deg["rot"].tolist() == [0, 1, 4, 4, 4, 2, 4] and (deg["log_s"][[2, 3, 4, 6]] == 2).all()


@pytest.mark.parametrize("name", ["strip", "odd", "sphere17_s2"])
def test_face_order(emul, name):
    check_face_order(ref_atlas(), name)
    check_face_order(emul_atlas(emul), name)


def test_wave_schedule_and_row_bands(emul):
    """(h) schedules 1 and 2 give the bits of schedule 0; the texel map in row bands equals the map in one launch"""
    A = emul_atlas(emul)
    try:
        for sched in (1, 2):
            emul.wemu_set_schedule(sched)
            for name in ("strip", "odd", "degenerate"):
                check_against_restatement(A, name)
            check_sample(A)
    finally:
        emul.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    v, f = make_mesh("strip")[:2]
    uv, S, lay, d, t0, t1 = reference("strip")
    for bands in ([(0, 16), (16, S)], [(24, S), (0, 24)], [(0, 5), (5, 6), (6, S)]):
        for a, b in zip(emul_texels(emul, v, f, lay, S, 1, bands), t1):
            assert same(a, b)
    part = emul_texels(emul, v, f, lay, S, 1, [(16, 32)])  # the other rows are not touched
    assert (part[0][:16] == -9).all() and (part[0][32:] == -9).all() and same(part[0][16:32], t1[0][16:32])


def test_halving_loop(emul):
    assert check_halving(ref_atlas()) == check_halving(emul_atlas(emul))


def test_contract(emul):
    check_contract(ref_atlas())
    check_contract(emul_atlas(emul))
    L = emul
    v, f, density, max_log = make_mesh("octahedron")
    for d in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(EmulError) as e:
            emul_classify(L, v, f, d)
        assert e.value.rc == INVALID
    for ml in (1, 14, -3):
        with pytest.raises(EmulError) as e:
            emul_classify(L, v, f, 1.0, ml)
        assert e.value.rc == INVALID
    uv, S, lay, d = ar.atlas(v, f, density)
    for size in (0, 3, 12, 16384):
        with pytest.raises(EmulError) as e:
            emul_place(L, lay["log_s"], lay["rot"], dict(lay, size=size))
        assert e.value.rc == INVALID
        with pytest.raises(EmulError) as e:
            emul_texels(L, v, f, lay, size, 1, [(0, 1)])
        assert e.value.rc == INVALID
    for clamp, band in ((2, (0, S)), (-1, (0, S)), (1, (-1, S)), (1, (0, S + 1)), (1, (5, 4))):
        with pytest.raises(EmulError) as e:
            emul_texels(L, v, f, lay, S, clamp, [band])
        assert e.value.rc == INVALID
    assert L.f2n_atlas_classify(None, 6, 8, None, _vp(f), _f(1.0), 7, None, None) == INVALID
    assert L.f2n_atlas_classify(None, 0, 0, None, None, _f(1.0), 7, None, None) == 0
    assert L.f2n_texture_sample(None, 0, 3, None, ctypes.c_int64(0), None, None) == INVALID
    assert L.f2n_texture_sample(None, 4, 0, None, ctypes.c_int64(0), None, None) == INVALID
    assert L.f2n_texture_sample(None, 4, 3, None, ctypes.c_int64(5), None, None) == INVALID
    assert L.f2n_texture_sample(None, 4, 3, None, ctypes.c_int64(0), None, None) == 0
    # a slot that names no block: zeros, no read out of bounds
    assert (emul_place(L, lay["log_s"], lay["rot"], dict(lay, slot=np.full(8, 2 * len(lay["block_log"]), np.int32))) == 0).all()
    bad = dict(lay, block_faces=np.where(lay["block_faces"] == 3, 77, lay["block_faces"]))  # a face index outside [0, F): unowned
    assert (emul_texels(L, v, f, bad, S, 1)[0] != 77).all() and (emul_texels(L, v, f, bad, S, 1)[0] != 3).all()


def test_texture_sample(emul):
    check_sample(ref_atlas())
    check_sample(emul_atlas(emul))


# ---- the writers --------------------------------------------------------------------------------------------------------------------
def _mesh_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("f2n_mesh_py", os.path.join(ROOT, "f2-nerf_amd", "mesh.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def decode_png(data):
    """8-bit RGB, filter 0 rows only (what write_png writes): [H,W,3] uint8; every chunk's CRC is checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        at += 12 + n
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


def test_write_png_round_trip(tmp_path):
    """(k)"""
    mesh = _mesh_module()
    rng = np.random.default_rng(4)
    for h, w in ((1, 1), (7, 5), (64, 64)):
        col = rng.uniform(-0.2, 1.2, (h, w, 3)).astype(F32)
        q = mesh.quantize_colors(col)
        path = mesh.write_png(str(tmp_path / "sub" / ("t%d.png" % h)), q)
        assert (decode_png(open(path, "rb").read()) == q).all()
        try:
            from PIL import Image
        except ImportError:
            continue
        im = Image.open(path)
        assert im.mode == "RGB" and (np.asarray(im) == q).all()
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), F32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            mesh.write_png(str(tmp_path / "bad.png"), bad)


def parse_obj(path):
    out = {"v": [], "vn": [], "vt": [], "f": [], "mtllib": None, "usemtl": None}
    for line in open(path):
        p = line.split()
        if not p:
            continue
        if p[0] in ("v", "vn", "vt"):
            out[p[0]].append([float(x) for x in p[1:]])
        elif p[0] == "f":
            out["f"].append([[int(x) for x in c.split("/")] for c in p[1:]])
        elif p[0] in ("mtllib", "usemtl"):
            out[p[0]] = p[1]
    return out


def test_write_obj(tmp_path):
    """(l)"""
    mesh = _mesh_module()
    v, f = make_mesh("octahedron")[:2]
    uv = reference("octahedron")[0]
    n = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    for normals in (None, n):
        path = mesh.write_obj(str(tmp_path / "o" / "m_tex.obj"), v, f, uv, normals, texture_name="m_tex.png")
        o = parse_obj(path)
        assert same(np.array(o["v"], F32), v) and len(o["vt"]) == 3 * len(f) and len(o["vn"]) == (0 if normals is None else len(v))
        vt = np.array(o["vt"], F32).reshape(-1, 3, 2)
        assert same(vt[:, :, 0], uv[:, :, 0]) and same(vt[:, :, 1], F32(1.0) - uv[:, :, 1])
        ff = np.array(o["f"])
        assert ff.shape == (len(f), 3, 2 if normals is None else 3) and ff.min() == 1
        assert (ff[:, :, 0] - 1 == f).all() and (ff[:, :, 1] - 1 == np.arange(3 * len(f)).reshape(-1, 3)).all()
        if normals is not None:
            assert (ff[:, :, 2] == ff[:, :, 0]).all() and same(np.array(o["vn"], F32), n)
        assert o["mtllib"] == "m_tex.mtl" and o["usemtl"] == "baked"
        mtl = open(str(tmp_path / "o" / "m_tex.mtl")).read()
        assert "newmtl baked" in mtl and "map_Kd m_tex.png" in mtl
    with pytest.raises(ValueError):
        mesh.write_obj(str(tmp_path / "bad.obj"), v, f, uv[:3])


def test_texture_options():
    mesh = _mesh_module()
    o = mesh.texture_options({})
    assert o == {"texture": False, "texels_per_step": 2.0, "max_size": 8192, "max_block_log2": 7, "source": "point", "ray_steps": 4.0}
    assert mesh.texture_options({"mesh": {"texture": "true"}, "texture": {"source": "RAY", "max_size": 1024}})["source"] == "ray"
    for bad in ({"texels_per_step": 0}, {"texels_per_step": float("nan")}, {"max_size": 1000}, {"max_size": 16384}, {"max_size": 2},
                {"max_block_log2": 1}, {"max_block_log2": 14}, {"source": "mesh"}, {"ray_steps": -1}, {"ray_steps": float("inf")}):
        with pytest.raises(ValueError):
            mesh.texture_options({"texture": bad})
