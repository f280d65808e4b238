"""Mesh-to-mesh distance without a GPU: the known answers of the numpy restatement (tests/mesh_distance_ref.py), then
f2n_mesh_closest_point / f2n_mesh_face_weights / f2n_mesh_sample_surface (csrc/octree.hip) under the wavefront emulator (tests/wave_emul)
against that restatement, bit for bit on dist, face, bary and the samples (both builds use -ffp-contract=off); the independence of the
grid, point order, face order and wave schedule; the cut-off; the contract cases; mesh.mesh_distance through the emulated library;
read_ply; the distance.* options.  The bodies that take a `Closer` run against the device as well (tests/test_gpu_mesh_distance.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import mesh_distance_ref as dr  # noqa: E402
import mesh_raycast_ref as rr  # noqa: E402
import test_mesh_raycast_cpu as rc_cpu  # noqa: E402

F32 = np.float32
INF = float("inf")
_f, _i = ctypes.c_float, ctypes.c_int
_vp, _lo3, _dims3, EmulError = rc_cpu._vp, rc_cpu._lo3, rc_cpu._dims3, rc_cpu.EmulError


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


def emul_closest(L, verts, faces, accel, points, max_dist=INF):
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    N = len(p)
    dist, face, bary = np.full(N, -7, F32), np.full(N, -7, np.int32), np.full((N, 3), -7, F32)
    lo = cell = dims = cs = cf = None
    if accel is not None:
        lo, cell, dims, cs, cf = accel
        if not dr.in_domain(lo, cell, dims, p):
            raise ValueError("a point lies outside the walk's domain")
        cs, cf = np.ascontiguousarray(cs, np.int32), np.ascontiguousarray(cf, np.int32)
    rc = L.f2n_mesh_closest_point(None, len(v), len(f), _vp(v), _vp(f), None if lo is None else _lo3(lo), _f(cell or 0.0),
                                  None if dims is None else _dims3(dims), None if cs is None else cs.ctypes.data_as(ctypes.c_void_p),
                                  None if cf is None else _vp(cf), N, _vp(p), _f(max_dist), _vp(dist), _vp(face), _vp(bary))
    if rc != 0:
        raise EmulError("f2n_mesh_closest_point", rc)
    return dist, face, bary


def emul_sample(L, verts, faces, n, seed=0):
    """MeshSampleSurface of csrc/host/RendererQuery.cpp call for call, numpy in the place of its torch plumbing (max, prefix sum)"""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nv, nf = len(v), len(f)
    area2, w = np.zeros(nf, np.float64), np.zeros(nf, np.int64)
    if nf:
        rc = L.f2n_mesh_face_weights(None, nv, nf, _vp(v), _vp(f), ctypes.c_double(0.0), _vp(area2), None)
        if rc != 0:
            raise EmulError("f2n_mesh_face_weights", rc)
    if not (nf and area2.max() > 0):
        raise ValueError("the mesh has no face with an area")
    rc = L.f2n_mesh_face_weights(None, nv, nf, _vp(v), _vp(f), ctypes.c_double(area2.max() * 2.0 ** -31), None, _vp(w))
    if rc != 0:
        raise EmulError("f2n_mesh_face_weights", rc)
    cum = np.cumsum(w, dtype=np.int64)
    pts, face, bary = np.full((n, 3), -7, F32), np.full(n, -7, np.int32), np.full((n, 3), -7, F32)
    rc = L.f2n_mesh_sample_surface(None, nv, nf, _vp(v), _vp(f), _vp(cum), n, ctypes.c_uint64(dr.sample_key(seed)), _vp(pts), _vp(face), _vp(bary))
    if rc != 0:
        raise EmulError("f2n_mesh_sample_surface", rc)
    return pts, face, bary


class Closer:
    """build(v, f, cell=None, lo=None) -> accel; closest(v, f, accel or None, points, max_dist=inf) -> (dist, face, bary) and
    sample(v, f, n, seed=0) -> (points, face, bary) as numpy arrays; error: what a status code of the library raises.  It is also the
    `backend` of mesh.mesh_distance (sample -> points, distances)."""
    def __init__(self, build, closest, sample, error):
        self.build, self.closest, self._sample, self.error = build, closest, sample, error

    def sample3(self, v, f, n, seed=0):
        return self._sample(v, f, n, seed)

    def sample(self, v, f, n, seed):
        return self._sample(v, f, n, seed)[0]

    def distances(self, v, f, points, max_dist):
        return self.closest(v, f, self.build(v, f), points, max_dist)[0]


def emul_closer(L):
    return Closer(lambda *a, **k: rc_cpu.emul_build(L, *a, **k), lambda *a, **k: emul_closest(L, *a, **k), lambda *a, **k: emul_sample(L, *a, **k),
                  EmulError)


# ---- meshes and points ---------------------------------------------------------------------------------------------------------------
def latlong_sphere(n_lat=14, n_lon=28):
    """the unit sphere as n_lat rings of n_lon vertices (the poles are rings too: their faces are degenerate): 392 vertices, 728 faces"""
    th = np.linspace(0.0, np.pi, n_lat)
    ph = np.arange(n_lon) * (2.0 * np.pi / n_lon)
    v = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon))], -1).reshape(-1, 3)
    f = []
    for i in range(n_lat - 1):
        for j in range(n_lon):
            a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
            f += [[a, a + n_lon, b], [b, a + n_lon, b + n_lon]]
    return v.astype(F32), np.array(f, np.int32)


CELLS = (5.0, 0.7, 0.3, 0.11, None)  # dims 1^3, 3^3, 7^3, 19^3 and the default cell
_cache = {}


def sphere_case():
    """(v, f, points [257,3]): the centre first (the deepest walk), a point with a NaN coordinate and one outside the grid on every side
    among the first 63, then random points of [-1.6, 1.6]^3, vertices, edge midpoints and points near the surface"""
    if "sphere" not in _cache:
        v, f = latlong_sphere()
        rng = np.random.default_rng(7)
        e = rc_cpu.edges_of(f)[::29]
        special = np.array([[0, 0, 0], [0.3, -0.2, 0.9], [np.nan, 0.1, 0.2], [-3, 0.1, 0.2], [3, 0.1, 0.2], [0.1, -3, 0.2], [0.1, 3, 0.2],
                            [0.1, 0.2, -3], [0.1, 0.2, 3], [2.5, 2.5, -2.5], [0.2, np.inf, 0.1]], np.float64)
        near = rng.standard_normal((60, 3))
        near = near / np.linalg.norm(near, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (60, 1))
        p = np.concatenate([special, rng.uniform(-1.6, 1.6, (257 - 11 - 40 - len(e) - 60, 3)), v[::10][:40], 0.5 * (v[e[:, 0]].astype(np.float64) + v[e[:, 1]]),
                            near]).astype(F32)
        assert p.shape == (257, 3) and len(v) == 392 and len(f) == 728
        for a in (v, f, p):
            a.setflags(write=False)
        _cache["sphere"] = (v, f, p)
    return _cache["sphere"]


def sphere_table(n_faces=728):
    """the restatement's pair table of the sphere case: computed once per process, shared, never written to"""
    if "table" not in _cache:
        v, f, p = sphere_case()
        t = dr.pair_table(v, f, p)
        for a in t:
            a.setflags(write=False)
        _cache["table"] = t
    dd, bary = _cache["table"]
    return dd[:, :n_faces], bary[:, :n_faces]


def sphere_reference(n_faces=728, max_dist=INF):
    key = ("ref", n_faces, max_dist)
    if key not in _cache:
        v, f, p = sphere_case()
        _cache[key] = dr.closest_point(v, f[:n_faces], p, max_dist, table=sphere_table(n_faces))
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


def same(out, ref):
    return all(rr.same_bits(a, b) for a, b in zip(out, ref))


def rows(ref, sel):
    return tuple(a[sel] for a in ref)


def two_triangles(ratio=1000.0):
    """two triangles in the plane z = 0.5 whose areas are 1 : ratio"""
    v = np.array([[0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.5], [2, 0, 0.5], [2 + ratio, 0, 0.5], [2, 1, 0.5]], F32)
    return v, np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def square(side=1.0, z=0.0, x0=0.0):
    v = np.array([[x0, x0, z], [x0 + side, x0, z], [x0 + side, x0 + side, z], [x0, x0 + side, z]], F32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


# ---- the bodies (emulator and device) ------------------------------------------------------------------------------------------------------
def check_against_restatement(cl, counts=(1, 63, 257), cells=CELLS, brute_faces=(255, 256, 257, 728)):
    """grid mode at every cell size and brute force at face counts that straddle the LDS tile, bit for bit against the restatement"""
    v, f, p = sphere_case()
    ref = sphere_reference()
    assert 150 < (ref[1] >= 0).sum() == len(p) - 2 and ref[1][2] == -1 and ref[1][10] == -1 and np.isinf(ref[0][2])
    for n in counts:
        for nf in brute_faces:
            assert same(cl.closest(v, f[:nf], None, p[:n]), rows(sphere_reference(nf), slice(0, n))), (n, nf)
        for cell in cells:
            assert same(cl.closest(v, f, cl.build(v, f, cell), p[:n]), rows(ref, slice(0, n))), (n, cell)


def check_independence(cl):
    """the same bits for permuted points and, in dist, for permuted faces (the winning face is then the lowest NEW index among equals)"""
    v, f, p = sphere_case()
    ref = sphere_reference()
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(p))
    accel = cl.build(v, f, 0.3)
    out = cl.closest(v, f, accel, p[perm])
    assert same(out, rows(ref, perm))
    fp = rng.permutation(len(f))
    for a in (None, cl.build(v, f[fp], 0.3)):
        d2, face2, _ = cl.closest(v, f[fp], a, p)
        assert rr.same_bits(d2, ref[0]) and (face2 >= 0).sum() == (ref[1] >= 0).sum()


def check_cutoff(cl):
    """a max_dist that cuts about half the points: the others keep their bits, the rest get the miss values, grid equals brute force"""
    v, f, p = sphere_case()
    ref = sphere_reference()
    md = float(np.median(ref[0][np.isfinite(ref[0])]))
    cut = sphere_reference(max_dist=md)
    far = ~(ref[0] <= F32(md))
    assert 100 < far.sum() < 160 and same(rows(cut, ~far), rows(ref, ~far))
    assert (cut[1][far] == -1).all() and np.isinf(cut[0][far]).all() and (cut[2][far] == 0).all()
    for cell in (None, 0.11, 0.7):
        assert same(cl.closest(v, f, cl.build(v, f, cell), p, md), cut), cell
    assert same(cl.closest(v, f, None, p, md), cut)
    none = cl.closest(v, f, cl.build(v, f, 0.11), p, 0.0)  # only points ON the mesh are within 0
    assert ((none[1] >= 0) == (ref[0] == 0)).all()


def check_contract(cl):
    """N = 0 and F = 0; a face index out of range is F2N_ERR_INVALID_ARG, a vertex outside the grid box F2N_ERR_UNSUPPORTED; a point outside
    the walk's domain is a ValueError of the host layer"""
    v, f, p = sphere_case()
    e3f, e3i = np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
    accel = cl.build(v, f, 0.3)
    for a in (None, accel):
        d, face, bary = cl.closest(v, f, a, e3f)
        assert d.shape == (0,) and face.shape == (0,) and bary.shape == (0, 3)
    for vv, a in ((v, None), (v, cl.build(v, e3i)), (e3f, cl.build(e3f, e3i))):
        d, face, bary = cl.closest(vv, e3i, a, p[:16])
        assert (face == -1).all() and np.isinf(d).all() and (bary == 0).all()
    for bad in ([0, 1, len(v)], [0, -1, 2]):
        fb = np.concatenate([f, [bad]]).astype(np.int32)
        for a in (None, accel):
            with pytest.raises(cl.error) as e:
                cl.closest(v, fb, a, p[:16])
            assert "-1" in str(e.value)
    v2 = np.array(v)
    v2[100] = [0.5, 7.0, 0.5]
    with pytest.raises(cl.error) as e:
        cl.closest(v2, f, accel, p[:16])
    assert "-2" in str(e.value)
    assert same(cl.closest(v2, f, None, p[:16]), dr.closest_point(v2, f, p[:16]))  # (brute force has no grid and no such domain)
    with pytest.raises(ValueError):
        cl.closest(v, f, accel, np.array([[0.0, 0.3 * 40000.0, 0.0]], F32))
    with pytest.raises((ValueError, cl.error)):
        cl.closest(v, f, accel, p[:4], -1.0)


def sample_error_bar(v, f, n, seed=0):
    """8 x the largest distance between the restatement's float32 samples and their float64 evaluation"""
    p32, _, _ = dr.sample_surface(v, f, n, seed)
    p64, _, _ = dr.sample_surface(v, f, n, seed, exact=True)
    return 8.0 * float(np.linalg.norm(p32.astype(np.float64) - p64, axis=1).max())


def check_sampling(cl, counts=(1, 64, 1000)):
    """Samples against the restatement bit for bit; |count_f - n w_f / T| < 2 on every face; seeds; every sample on its face: the closest
    point distance of a sample to its own mesh is at most 8 x the restatement's own float32-against-float64 error (measured at
    n = 1000: the largest distance is 8.9e-8 on the sphere against a bar of 7.7e-7, and 6.0e-8 on the 1 : 1000 triangles -- coordinates
    up to 1002, but the distance to their plane z = 0.5 only sees the rounding of z -- against a bar of 8.5e-4)."""
    for name, (v, f) in (("sphere", sphere_case()[:2]), ("two", two_triangles())):
        w, cum, T = dr.face_weights(v, f)
        for n in counts:
            out = cl.sample3(v, f, n)
            ref = dr.sample_surface(v, f, n)
            assert same(out, ref), (name, n)
            pts, face, bary = out
            cnt = np.bincount(face, minlength=len(f))
            assert (np.abs(cnt - n * w.astype(np.float64) / T) < 2).all() and cnt.sum() == n and (cnt[w == 0] == 0).all()
            assert (bary >= 0).all() and (np.abs(bary.astype(np.float64).sum(1) - 1.0) <= 2 * 2.0 ** -23).all()
            bar = sample_error_bar(v, f, n)
            d, _, _ = cl.closest(v, f, cl.build(v, f), pts)
            print("%s n=%d: largest distance of a sample to its mesh %.3g, bar %.3g" % (name, n, d.max(), bar))
            assert d.max() <= bar, (name, n, d.max(), bar)
        a, b = cl.sample3(v, f, 64, 5), cl.sample3(v, f, 64, 5)
        assert same(a, b) and not rr.same_bits(a[0], cl.sample3(v, f, 64, 6)[0]) and same(a, dr.sample_surface(v, f, 64, 5))
    v, f = two_triangles()
    cnt = np.bincount(cl.sample3(v, f, 1000)[1], minlength=2)
    assert cnt.tolist() in ([0, 1000], [1, 999], [2, 998])  # n w_0 / T = 0.999
    flat = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], F32)
    with pytest.raises(ValueError):
        cl.sample3(flat, np.array([[0, 1, 2]], np.int32), 4)


def check_mesh_distance(cl, n=1000):
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    keys = {"a_to_b", "b_to_a", "chamfer", "hausdorff", "thresholds", "precision", "recall", "fscore", "unit", "seed", "n_faces_a", "n_faces_b",
            "max_dist"}
    stat_keys = {"n", "missed", "mean", "rms", "median", "p90", "p95", "max"}
    v, f = sphere_case()[:2]
    res = mesh.mesh_distance(v, f, v, f, n=n, backend=cl)
    bar = sample_error_bar(v, f, n)
    assert set(res) == keys and set(res["a_to_b"]) == stat_keys == set(res["b_to_a"]) and res["thresholds"] == [0.5, 1.0, 2.0]
    for side in ("a_to_b", "b_to_a"):
        assert res[side]["n"] == n and res[side]["missed"] == 0 and all(0.0 <= res[side][k] <= bar for k in stat_keys - {"n", "missed"})
    assert res["fscore"] == [1.0, 1.0, 1.0] == res["precision"] == res["recall"] and res["hausdorff"] <= bar and res["chamfer"] <= bar
    assert res == mesh.mesh_distance(v, f, v, f, n=n, backend=cl)
    # a square and its copy shifted by h along its normal
    h = 0.25
    (va, fa), (vb, fb) = square(1.0, 0.0), square(1.0, h)
    res = mesh.mesh_distance(va, fa, vb, fb, n=n, thresholds=(0.5 * h, 2.0 * h), backend=cl)
    for side in ("a_to_b", "b_to_a"):
        assert all(abs(res[side][k] - h) <= 1e-6 * h for k in ("mean", "rms", "median", "p90", "p95", "max")), res[side]
    assert abs(res["hausdorff"] - h) <= 1e-6 * h and abs(res["chamfer"] - h) <= 1e-6 * h and res["fscore"] == [0.0, 1.0]
    scaled = mesh.mesh_distance(va, fa, vb, fb, n=n, thresholds=(0.5, 2.0), unit=h, backend=cl)
    assert abs(scaled["hausdorff"] - 1.0) <= 1e-6 and scaled["fscore"] == [0.0, 1.0] and scaled["unit"] == h
    gone = mesh.mesh_distance(va, fa, vb, fb, n=n, max_dist=0.5 * h, backend=cl)
    assert gone["a_to_b"]["missed"] == n == gone["b_to_a"]["missed"] and gone["a_to_b"]["max"] == 0.0 and gone["fscore"] == [0.0, 0.0, 0.0]
    # a square against a larger coplanar one: A strays nowhere, parts of B are far from A
    vb, fb = square(3.0, 0.0, -1.0)
    res = mesh.mesh_distance(va, fa, vb, fb, n=n, thresholds=(0.25,), backend=cl)
    assert res["a_to_b"]["max"] <= 1e-6 and res["b_to_a"]["max"] > 1.0 and res["hausdorff"] == res["b_to_a"]["max"]
    assert res["precision"] == [1.0] and 0.1 < res["recall"][0] < 0.5 and abs(res["chamfer"] - 0.5 * (res["a_to_b"]["mean"] + res["b_to_a"]["mean"])) < 1e-12
    d = cl.distances(va, fa, cl.sample(vb, fb, n, 0), INF)
    cut = mesh.mesh_distance(va, fa, vb, fb, n=n, max_dist=0.5, backend=cl)
    assert cut["b_to_a"]["missed"] == int((d > F32(0.5)).sum()) > 0 and cut["a_to_b"]["missed"] == 0
    assert cut["b_to_a"]["max"] <= 0.5 and cut["b_to_a"]["n"] == n
    for bad in (dict(unit=0.0), dict(n=0), dict(max_dist=-1.0)):
        with pytest.raises(ValueError):
            mesh.mesh_distance(va, fa, vb, fb, backend=cl, **bad)


# ---- the restatement alone ------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_restatement():
    """one triangle with a point in each of the seven regions; the height above a plane of two triangles, exact for dyadic numbers"""
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], F32)
    f = np.array([[0, 1, 2]], np.int32)
    p = np.array([[-1, -1, 2], [6, -1, 2], [-1, 6, 2], [2, -3, 0], [-3, 2, 0], [4, 4, 0], [1, 1, 0.5]], F32)
    want_q = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0], [1, 1, 0]], np.float64)
    want_b = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5], [0.5, 0.25, 0.25]], F32)
    dist, face, bary = dr.closest_point(v, f, p)
    assert (face == 0).all() and rr.same_bits(bary, want_b)
    assert rr.same_bits(dist, np.linalg.norm(p.astype(np.float64) - want_q, axis=1).astype(F32))
    v, f = square(8.0, 0.25, -4.0)
    rng = np.random.default_rng(1)
    p = np.concatenate([rng.integers(-24, 24, (64, 2)) / 8.0, 0.25 + rng.integers(-40, 40, (64, 1)) / 16.0], 1).astype(F32)
    lo = np.array([-4.0, -4.0, 0.0], F32)
    for accel in (None, (lo, 1.0, [8, 8, 1], *rr.bin_faces(v, f, lo, 1.0, [8, 8, 1]))):
        fn = dr.closest_point if accel is None else (lambda a, b, c: dr.closest_point_grid(a, b, accel, c))
        dist, face, bary = fn(v, f, p)
        assert rr.same_bits(dist, np.abs(p[:, 2] - F32(0.25))) and (face >= 0).all()
    # a degenerate face and a face with a vertex that is not finite never win unless their walk stays finite
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [np.nan, 0, 0], [0, 0, 5], [1, 0, 5], [0, 1, 5]], F32)
    f = np.array([[0, 1, 2], [0, 1, 3], [4, 5, 6]], np.int32)
    dist, face, _ = dr.closest_point(v, f, np.array([[0.25, 0.25, 4.0], [0.5, 3.0, 0.0]], F32))
    assert face.tolist()[0] == 2 and dist[0] == 1.0


def test_the_shell_walk_of_the_restatement_equals_its_brute_force():
    """the prototype of the LB rule: every cell size, every point; the deepest walk is the centre's at the smallest cell"""
    v, f, p = sphere_case()
    ref = sphere_reference()
    for cell in CELLS:
        cell = rr.default_cell(v, f) if cell is None else cell
        lo, dims = rr.grid_for(v, cell)
        shells = []
        out = dr.closest_point_grid(v, f, (lo, cell, dims, *rr.bin_faces(v, f, lo, cell, dims)), p, table=sphere_table(), shells=shells)
        assert same(out, ref), cell
        if cell == 0.11:
            inside = (np.abs(p) <= 1).all(1)
            assert dims == [19, 19, 19] and max(np.array(shells)[inside[np.isfinite(p).all(1)]]) == shells[0] >= 9 and max(shells) <= 19
    assert [rr.grid_for(v, c)[1][0] for c in CELLS[:4]] == [1, 3, 7, 19]


# ---- the emulator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 257])
def test_device_code_matches_the_restatement_on_the_emulator(emul, count):
    check_against_restatement(emul_closer(emul), counts=(count,))


def test_point_and_face_order_on_the_emulator(emul):
    check_independence(emul_closer(emul))


def test_the_cut_off_on_the_emulator(emul):
    check_cutoff(emul_closer(emul))


def test_results_do_not_depend_on_the_wave_schedule(emul):
    emul.wemu_set_schedule(1)
    try:
        cl = emul_closer(emul)
        check_against_restatement(cl, counts=(63,), cells=(0.3, 0.11), brute_faces=(257,))
        check_sampling(cl, counts=(64,))
    finally:
        emul.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))


def test_contract_cases_on_the_emulator(emul):
    check_contract(emul_closer(emul))


def test_error_codes_of_the_entry_points(emul):
    L = emul
    v, f, p = sphere_case()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    v, f, p = np.array(v), np.array(f), np.array(p[:4])
    dist, face, bary = np.zeros(4, F32), np.zeros(4, np.int32), np.zeros((4, 3), F32)
    cs, cf = np.zeros(28, np.int32), np.zeros(1, np.int32)
    lo, dims = _lo3((-1.0, -1.0, -1.0)), _dims3((3, 3, 3))
    call = lambda **k: L.f2n_mesh_closest_point(None, k.get("nv", 392), k.get("nf", 728), k.get("v", P(v)), k.get("f", P(f)), k.get("lo", lo),  # noqa: E731
                                                _f(k.get("cell", 0.7)), k.get("dims", dims), k.get("cs", P(cs)), P(cf), k.get("N", 4),
                                                k.get("p", P(p)), _f(k.get("md", INF)), k.get("dist", P(dist)), k.get("face", P(face)),
                                                k.get("bary", P(bary)))
    for cell in (0.0, -2.0, float("nan"), INF):
        assert call(cell=cell) == rc_cpu.INVALID
    for md in (-1.0, float("nan")):
        assert call(md=md) == rc_cpu.INVALID and call(md=md, cs=None) == rc_cpu.INVALID
    assert call(dims=_dims3((0, 3, 3))) == rc_cpu.INVALID and call(lo=None) == rc_cpu.INVALID and call(dims=None) == rc_cpu.INVALID
    assert call(v=None) == rc_cpu.INVALID and call(f=None) == rc_cpu.INVALID and call(p=None) == rc_cpu.INVALID and call(N=-1) == rc_cpu.INVALID
    assert call(dist=None) == rc_cpu.INVALID and call(face=None) == rc_cpu.INVALID and call(bary=None) == rc_cpu.INVALID
    assert call(N=0, p=None, dist=None, face=None, bary=None) == 0 and (dist == 0).all() and (face == 0).all()  # nothing was written
    assert call(lo=_lo3((-1.0, -1.0, 30000.0))) == rc_cpu.UNSUPPORTED and call(cs=None, lo=_lo3((-1.0, -1.0, 30000.0))) == 0
    assert (face[[0, 1, 3]] >= 0).all() and face[2] == -1  # (that last call was the brute-force mode: it ran)
    a2, w = np.zeros(728, np.float64), np.zeros(728, np.int64)
    fw = lambda **k: L.f2n_mesh_face_weights(None, k.get("nv", 392), k.get("nf", 728), P(v), k.get("f", P(f)), ctypes.c_double(k.get("q", 1e-9)),  # noqa: E731
                                             k.get("a2", P(a2)), k.get("w", P(w)))
    assert fw(q=0.0) == rc_cpu.INVALID and fw(q=INF) == rc_cpu.INVALID and fw(q=float("nan")) == rc_cpu.INVALID and fw(q=0.0, w=None) == 0
    assert fw(a2=None, w=None) == rc_cpu.INVALID and fw(f=None) == rc_cpu.INVALID and fw(nf=-1) == rc_cpu.INVALID and fw(nf=0, f=None) == 0
    assert rr.same_bits(a2, dr.face_area2(v, f)) and (a2[0:56:2] == 0).all() and (a2[1:56:2] > 0).all()  # every other pole face is degenerate
    cum, pts, sf, sb = np.cumsum(dr.face_weights(v, f)[0]), np.zeros((4, 3), F32), np.zeros(4, np.int32), np.zeros((4, 3), F32)
    ss = lambda **k: L.f2n_mesh_sample_surface(None, k.get("nv", 392), k.get("nf", 728), P(v), P(f), k.get("cum", P(cum)), k.get("n", 4),  # noqa: E731
                                               ctypes.c_uint64(dr.sample_key(9)), k.get("pts", P(pts)), P(sf), P(sb))
    assert ss(n=-1) == rc_cpu.INVALID and ss(cum=None) == rc_cpu.INVALID and ss(pts=None) == rc_cpu.INVALID and ss(nf=0) == rc_cpu.INVALID
    assert ss(n=0, cum=None, pts=None) == 0 and (pts == 0).all() and ss() == 0 and same((pts, sf, sb), dr.sample_surface(v, f, 4, 9))


def test_sampling_on_the_emulator(emul):
    check_sampling(emul_closer(emul))


def test_mesh_distance_through_the_emulator(emul):
    check_mesh_distance(emul_closer(emul))


# ---- read_ply, options, the launcher ---------------------------------------------------------------------------------------------------
def test_read_ply(tmp_path):
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    v, f = latlong_sphere(5, 7)
    rng = np.random.default_rng(0)
    nrm, col = rng.standard_normal(v.shape).astype(F32), rng.uniform(0, 1, v.shape).astype(F32)
    for k, (n, c) in enumerate(((None, None), (nrm, None), (None, col), (nrm, col))):
        path = mesh.write_ply(str(tmp_path / ("m%d.ply" % k)), v, f, n, c)
        rv, rf = mesh.read_ply(path)
        assert rv.dtype == F32 and rf.dtype == np.int32 and rr.same_bits(rv, v) and rr.same_bits(rf, f)
    ascii_ply = ("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                 "property uchar red\nelement face 2\nproperty list uchar uint vertex_index\nend_header\n"
                 "0 0 0 255\n1 0 0 0\n1 1 0.5 7\n0 1 0 9\n3 0 1 2\n3 0 2 3\n")
    (tmp_path / "a.ply").write_text(ascii_ply)
    rv, rf = mesh.read_ply(str(tmp_path / "a.ply"))
    assert rv.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0]] and rf.tolist() == [[0, 1, 2], [0, 2, 3]]
    bad = {"quad": ascii_ply.replace("element face 2", "element face 1").replace("3 0 1 2\n3 0 2 3\n", "4 0 1 2 3\n"),
           "big_endian": ascii_ply.replace("format ascii", "format binary_big_endian"),
           "double": ascii_ply.replace("property float x", "property double x"),
           "no_z": ascii_ply.replace("property float z\n", "property float w\n"),
           "index": ascii_ply.replace("3 0 2 3\n", "3 0 2 4\n"),
           "element": ascii_ply.replace("element face 2", "element edge 2"),
           "short": ascii_ply.replace("3 0 2 3\n", ""),
           "not_ply": "solid\n"}
    for name, text in bad.items():
        (tmp_path / "bad.ply").write_text(text)
        with pytest.raises(ValueError):
            mesh.read_ply(str(tmp_path / "bad.ply"))
    head = "ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n" \
           "property list uchar int vertex_indices\nend_header\n"
    with open(tmp_path / "q.ply", "wb") as fh:  # a binary quad
        fh.write(head.encode() + np.zeros(12, "<f4").tobytes() + b"\x04" + np.arange(4, dtype="<i4").tobytes())
    with pytest.raises(ValueError):
        mesh.read_ply(str(tmp_path / "q.ply"))


def test_distance_options_parse_and_default():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    assert mesh.distance_options(config.preset("wanjinyou", [])) == {"distance": False, "distance_to": None, "samples": 200000, "seed": 0,
                                                                      "thresholds": [0.5, 1.0, 2.0], "max_dist_steps": None}
    o = mesh.distance_options(config.preset("wanjinyou", ["mesh.distance=true", "mesh.simplify=2", "distance.samples=5000", "distance.seed=3",
                                                           "distance.thresholds=[0.25,1]", "distance.max_dist_steps=8"]))
    assert o == {"distance": True, "distance_to": None, "samples": 5000, "seed": 3, "thresholds": [0.25, 1.0], "max_dist_steps": 8.0}
    o = mesh.distance_options(config.preset("wanjinyou", ["mesh.distance_to=/some/scan.ply"]))
    assert o["distance_to"] == "/some/scan.ply" and not o["distance"]
    for bad in (["mesh.distance=true"], ["mesh.distance=true", "mesh.simplify=1"], ["distance.samples=0"], ["distance.seed=-1"],
                ["distance.thresholds=[]"], ["distance.thresholds=[0.5,-1]"], ["distance.max_dist_steps=0"], ["distance.samples=x"],
                ["mesh.distance=true", "mesh.simplify=2", "mesh.distance_to=/some/scan.ply"]):
        with pytest.raises(ValueError):
            mesh.distance_options(config.preset("wanjinyou", bad))
    assert "distance" not in config.GROUP_DEFAULTS
    # options, check_options and texture_options do not know the new keys
    cfg = config.preset("wanjinyou", ["mesh.distance=true", "mesh.simplify=2"])
    assert "distance" not in mesh.options(cfg) and "distance" not in mesh.check_options(cfg) and "distance" not in mesh.texture_options(cfg)


def test_the_launcher_refuses_a_distance_without_something_to_compare_with(tmp_path, capsys):
    import torch
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    v, f = rc_cpu.octahedron()

    class Runner:
        iter_step = 60

        def extract_mesh(self, lo, hi, res, level):
            return torch.from_numpy(v), torch.from_numpy(f)

    scene = {"center": np.zeros(3, F32), "radius": 1.0}
    with pytest.raises(ValueError) as e:
        mesh.extract(Runner(), config.preset("wanjinyou", ["mesh.resolution=16", "mesh.distance=true"]), scene, str(tmp_path))
    assert "mesh.simplify" in str(e.value) and not os.path.exists(tmp_path / "meshes")  # refused before anything is written
    path = mesh.extract(Runner(), config.preset("wanjinyou", ["mesh.resolution=16"]), scene, str(tmp_path))
    assert sorted(os.listdir(os.path.dirname(path))) == ["60_16.ply"]
