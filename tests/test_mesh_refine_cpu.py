"""Mesh refinement without a GPU: the known answers on the numpy restatement alone (tests/mesh_refine_ref.py), then f2n_mesh_ring_keys /
_fill, f2n_mesh_smooth, f2n_mesh_move_clamp, f2n_level_step and f2n_mesh_face_quality (csrc/octree.hip) under the wavefront emulator
(tests/wave_emul) against that restatement, bit for bit (both builds use -ffp-contract=off); the contract cases; the mesh.refine
options.  The bodies that take an `impl` run against the device as well (tests/test_gpu_mesh_refine.py).

An `impl` is an object with
  ring(faces, n_verts) -> (ring_start_end, ring, pinned, [boundary_edges, nonmanifold_edges])
  smooth(verts, faces, passes, lam, mu, max_move) -> verts
  quality(verts, faces) -> [F] float64
  level_step(first, propose, p0, sigma, grad, h, tol, max_step, max_move, state) -> state   (the dict of mesh_refine_ref.level_state)
on numpy arrays."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import mesh_ref as mr  # noqa: E402
import mesh_refine_ref as rr  # noqa: E402

F32 = np.float32
INF = float("inf")
INVALID = -1  # F2N_ERR_INVALID_ARG
_f, _i, _d = ctypes.c_float, ctypes.c_int, ctypes.c_double
STATE_KEYS = ("cand", "best", "h_best", "g_best", "scale", "status", "evals")


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size > 0 else None


class EmulError(RuntimeError):
    def __init__(self, name, rc):
        RuntimeError.__init__(self, "%s failed with status %d" % (name, rc))
        self.rc = rc


def _ck(rc, name):
    if rc != 0:
        raise EmulError(name, rc)


def emul_impl(L):
    """MeshRing / MeshSmooth / MeshFaceQuality / LevelStep of csrc/host/RendererQuery.cpp call for call, numpy in the place of the torch
    plumbing (the sort and the run lengths)."""
    def ring_arrays(faces, n_verts):
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        nf = len(f)
        keys = np.full((nf, 6), -7, np.int64)
        _ck(L.f2n_mesh_ring_keys(None, n_verts, nf, _vp(f), _vp(keys)), "f2n_mesh_ring_keys")
        ek, uses = rr.edges_of(keys)
        ek, uses = np.ascontiguousarray(ek), np.ascontiguousarray(uses)
        se, ring = np.full((n_verts, 2), -7, np.int32), np.full(len(ek), -7, np.int32)
        pinned, counts = np.full(n_verts, 7, np.uint8), np.full(2, 7, np.int32)
        _ck(L.f2n_mesh_ring_fill(None, n_verts, len(ek), _vp(ek), _vp(uses), _vp(se), _vp(ring), _vp(pinned), _vp(counts)), "f2n_mesh_ring_fill")
        return se, ring, pinned, counts

    def ring(faces, n_verts):
        se, rg, pinned, counts = ring_arrays(faces, n_verts)
        return se, rg, pinned, [int(c) for c in counts]

    def smooth(verts, faces, passes, lam=0.5, mu=-0.53, max_move=INF):
        if passes < 0 or not (np.isfinite(lam) and np.isfinite(mu)) or not max_move > 0:
            raise ValueError("mesh_smooth: bad argument")
        v0 = np.ascontiguousarray(verts, F32).reshape(-1, 3)
        nv = len(v0)
        a = v0.copy()
        if nv == 0 or passes == 0:
            return a
        se, rg, pinned, _ = ring_arrays(faces, nv)
        b = np.full_like(a, np.nan)
        for _ in range(passes):
            for src, dst, factor in ((a, b, lam), (b, a, mu)):
                _ck(L.f2n_mesh_smooth(None, nv, len(rg), _vp(src), _vp(se), _vp(rg), _vp(pinned), _d(factor), _vp(dst)), "f2n_mesh_smooth")
        if np.isfinite(max_move):
            _ck(L.f2n_mesh_move_clamp(None, nv, _vp(v0), _f(max_move), _vp(a)), "f2n_mesh_move_clamp")
        return a

    def quality(verts, faces):
        v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        q = np.full(len(f), -7.0, np.float64)
        _ck(L.f2n_mesh_face_quality(None, len(v), len(f), _vp(v), _vp(f), _vp(q)), "f2n_mesh_face_quality")
        return q

    def level_step(first, propose, p0, sigma, grad, h, tol, max_step, max_move, st):
        p0, sigma, grad, h = (np.ascontiguousarray(a, F32) for a in (p0, sigma, grad, h))
        _ck(L.f2n_level_step(None, len(p0), int(first), int(propose), _vp(p0), _vp(sigma), _vp(grad), _vp(h), _f(tol), _f(max_step), _f(max_move),
                             *(_vp(st[k]) for k in STATE_KEYS)), "f2n_level_step")
        return st

    return types.SimpleNamespace(ring=ring, smooth=smooth, quality=quality, level_step=level_step)


def _ref_ring(faces, n_verts):
    se, rg, pinned, counts = rr.ring(faces, n_verts)
    return se, rg, pinned, [int(c) for c in counts]


REF = types.SimpleNamespace(ring=_ref_ring, smooth=rr.smooth, quality=rr.face_quality, level_step=rr.level_step)


# ---- the meshes --------------------------------------------------------------------------------------------------------------------
def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def plane(n=9, jitter=0.0, seed=4):
    """the n x n grid of integer points in z = 0, every cell cut along the same diagonal; jitter: the interior z by a seeded +-jitter"""
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), np.zeros(n * n)], 1).astype(F32)
    i = (y[:-1, :-1] * n + x[:-1, :-1]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + n + 1], 1), np.stack([i, i + n + 1, i + n], 1)]).astype(np.int32)
    if jitter:
        inner = ((x > 0) & (x < n - 1) & (y > 0) & (y < n - 1)).ravel()
        v[inner, 2] = np.random.default_rng(seed).uniform(-jitter, jitter, inner.sum()).astype(F32)
    return v, f


def two_triangles():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.25]], F32)
    return v, np.array([[0, 1, 2], [2, 1, 3]], np.int32)


def fan():
    """three triangles on the edge (0, 1), and a closed tetrahedron on vertices of its own beside them (its vertices may move)"""
    v = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [-0.5, 0.8, 0.5], [-0.5, -0.8, 0.5],
                  [3, 0, 0], [4, 0, 0], [3, 1, 0], [3, 0.25, 1.5]], F32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [5, 7, 6], [5, 6, 8], [6, 7, 8], [7, 5, 8]], np.int32)
    return v, f


SPHERE_N, SPHERE_R = 33, 0.4 * 32
_meshes = {}


def sphere(mesh_fn, n=SPHERE_N):
    """the marching-tetrahedra mesh of mesh_ref.sphere_grid(n, 0.4 (n - 1)); mesh_fn(grid, level) -> (verts, faces); made once per mesher"""
    key = (n, id(mesh_fn))
    if key not in _meshes:
        _meshes[key] = mesh_fn(mr.sphere_grid(n, 0.4 * (n - 1)), 0.0)
    return _meshes[key]


def emul_mesher(L):
    from test_tsdf_cpu import emul_mesh as em

    def fn(g, level):
        o = em(L, g, None, level, (0.0, 0.0, 0.0), 1.0)
        return o["verts"], o["faces"]
    return fn


def sphere_error(v, n=SPHERE_N):
    c = (n - 1) / 2.0
    return float(np.mean(np.abs(np.linalg.norm(v.astype(np.float64) - c, axis=1) - 0.4 * (n - 1))))


_refs = {}


def reference(name, fn):
    """a result of the restatement: computed once, shared, never written to"""
    if name not in _refs:
        out = fn()
        for a in out if isinstance(out, tuple) else (out,):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[name] = out
    return _refs[name]


# ---- known answers (whoever computed them) -----------------------------------------------------------------------------------------
def ring_of(se, rg, v):
    return rg[se[v, 0]:se[v, 1]].tolist()


def check_small_meshes(impl):
    """octahedron, plane, two triangles, the fan, invalid faces, face order: rings, pins, counts and the smoothing's exact values"""
    v, f = octahedron()
    se, rg, pinned, counts = impl.ring(f, 6)
    for i in range(6):
        assert ring_of(se, rg, i) == [j for j in range(6) if j != i and j != (i ^ 1)]
    assert not pinned.any() and counts == [0, 0]
    one = impl.smooth(v, f, 1, 0.5, 0.0, INF)  # (the mu pass with factor 0 adds 0 * d: the lambda pass alone)
    assert rr.same_bits(one[0], np.array([0.5, 0, 0], F32)) and rr.same_bits(one[4], np.array([0, 0, 0.5], F32))
    pair = impl.smooth(v, f, 1, 0.5, -0.53, INF)
    # lambda: every vertex to half its length exactly; mu: 0.5 + (-0.53) (0 - 0.5) = 0.765 in fp64, rounded to fp32 once
    assert rr.same_bits(pair[0], np.array([F32(0.5 + (-0.53) * (0.0 - 0.5)), 0, 0], F32)) and abs(float(pair[0, 0]) - 0.765) <= 2.0 ** -24
    # the flat plane: pinned rim, symmetric interior rings, any number of passes returns the input's bits
    v, f = plane()
    se, rg, pinned, counts = impl.ring(f, 81)
    rim = ((v[:, 0] == 0) | (v[:, 0] == 8) | (v[:, 1] == 0) | (v[:, 1] == 8))
    assert (pinned.astype(bool) == rim).all() and counts == [32, 0]
    for i in np.flatnonzero(~rim):
        assert np.abs(v[ring_of(se, rg, i)].astype(np.float64).mean(0) - v[i]).max() == 0 and len(ring_of(se, rg, i)) == 6
    for passes in (1, 3, 10):
        assert rr.same_bits(impl.smooth(v, f, passes, 0.5, -0.53, INF), v)
    vj, _ = plane(jitter=0.3)
    out = impl.smooth(vj, f, 10, 0.5, -0.53, INF)
    before, after = float((vj[:, 2].astype(np.float64) ** 2).sum()), float((out[:, 2].astype(np.float64) ** 2).sum())
    print("jittered plane: sum z^2 %.4f -> %.4f after 10 pairs" % (before, after))
    assert after < before and rr.same_bits(out[rim], vj[rim]) and rr.same_bits(out[:, :2], vj[:, :2])
    # two triangles on an edge: four boundary edges, everything pinned
    v, f = two_triangles()
    se, rg, pinned, counts = impl.ring(f, 4)
    assert counts == [4, 0] and pinned.tolist() == [1, 1, 1, 1] and ring_of(se, rg, 1) == [0, 2, 3] and ring_of(se, rg, 0) == [1, 2]
    assert rr.same_bits(impl.smooth(v, f, 3, 0.5, -0.53, INF), v)
    # three triangles on one edge: one non-manifold edge, its ends pinned (and the fan's rim, a boundary); the tetrahedron beside it is free
    v, f = fan()
    se, rg, pinned, counts = impl.ring(f, 9)
    assert counts == [6, 1] and pinned.tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0] and ring_of(se, rg, 0) == [1, 2, 3, 4]
    # a face with a repeated or an out-of-range index changes nothing; nor does the order of the faces; a vertex no face uses is pinned
    base = impl.ring(f, 10)
    assert base[2].tolist()[9] == 1 and ring_of(base[0], base[1], 9) == []
    f_bad = np.concatenate([f[:2], [[5, 5, 6], [0, 10, 1], [-1, 2, 3]], f[2:]]).astype(np.int32)
    perm = np.random.default_rng(1).permutation(len(f_bad))
    for ff in (f_bad, f_bad[perm]):
        got = impl.ring(ff, 10)
        assert all(rr.same_bits(a, b) for a, b in zip(got[:3], base[:3])) and got[3] == base[3]
    v10 = np.concatenate([v, [[9, 9, 9]]]).astype(F32)
    assert rr.same_bits(impl.smooth(v10, f_bad[perm], 2, 0.5, -0.53, 0.2), impl.smooth(v10, f, 2, 0.5, -0.53, 0.2))


def check_face_quality(impl):
    s3 = np.sqrt(3.0)
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, s3 / 2, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0], [3, 0, 0]], F32)
    f = np.array([[0, 1, 3], [0, 1, 4], [0, 1, 5], [0, 0, 1], [0, 1, 7], [0, 4, 6]], np.int32)
    q = impl.quality(v, f)
    assert abs(q[0] - s3 / 2) <= 4 * 2.0 ** -52 and q[1] == 0 and np.isnan(q[2]) and q[3] == 0 and q[4] == 0 and q[5] == 0
    # an equilateral face whose fp32 coordinates are exact: the face (1,0,0), (0,1,0), (0,0,1)
    q = impl.quality(np.eye(3, dtype=F32), np.array([[0, 1, 2]], np.int32))
    assert abs(q[0] - 1.0) <= 4 * 2.0 ** -52
    assert impl.quality(v, np.zeros((0, 3), np.int32)).shape == (0,)


def check_sphere(impl, mesh_fn):
    """the 33^3 sphere: closed, nothing pinned; 10 Taubin pairs raise the 5th percentile of face quality and stay nearer the sphere than
    10 plain Laplacian pairs (mu = lam)"""
    v, f = sphere(mesh_fn)
    se, rg, pinned, counts = impl.ring(f, len(v))
    assert not pinned.any() and counts == [0, 0] and len(rg) == 3 * len(f)  # closed: E = 3F/2 undirected edges, each twice
    taubin, laplace = impl.smooth(v, f, 10, 0.5, -0.53, INF), impl.smooth(v, f, 10, 0.5, 0.5, INF)
    q0, q1 = np.quantile(impl.quality(v, f), 0.05), np.quantile(impl.quality(taubin, f), 0.05)
    e0, et, el = sphere_error(v), sphere_error(taubin), sphere_error(laplace)
    print("sphere33: %d faces; quality p05 %.4f -> %.4f; mean ||v| - R| input %.4f, Taubin %.4f, Laplacian %.4f" % (len(f), q0, q1, e0, et, el))
    assert q1 > q0 and et < el
    return taubin


# ---- the level step on an analytic field -------------------------------------------------------------------------------------------
LEVEL_R, LEVEL_K, LEVEL_SIGMA = 2.0, 3.0, 10.0


def level_points(n=4096, seed=7):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * (LEVEL_R * rng.uniform(0.8, 1.2, (n, 1)))).astype(F32)


def sphere_field(p, call, mode="plain"):
    """(sigma, grad, h) of sigma = level exp(k (R - |p|)) at p, in fp32: h = k (R - |p|), grad / sigma = -k p / |p|.  mode "flip": the
    sign of the gradient is wrong on the odd evaluations (the first, the third, ...); "empty": sigma = 0 everywhere"""
    p = np.asarray(p, F32)
    with np.errstate(all="ignore"):
        r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        h = F32(LEVEL_K) * (F32(LEVEL_R) - r)
        sigma = (F32(LEVEL_SIGMA) * np.exp(h)).astype(F32)
        g = -F32(LEVEL_K) * p / r[:, None]
        if mode == "flip" and call % 2 == 0:
            g = -g
        grad = (sigma[:, None] * g).astype(F32)
        if mode == "empty":
            sigma, grad = np.zeros_like(sigma), np.zeros_like(grad)
            h = np.full_like(h, -np.inf)
    return sigma, grad, h.astype(F32)


def drive(impl, p0, calls, tol, max_step, max_move, mode="plain"):
    """the projection loop on the analytic field: the state after every call (copies)"""
    st = rr.level_state(len(p0))
    st["cand"] = np.ascontiguousarray(p0, F32).copy()
    for key in STATE_KEYS[1:]:  # (what a first call must overwrite)
        st[key] = np.full_like(st[key], 77)
    snaps = []
    for k in range(calls):
        sigma, grad, h = sphere_field(st["cand"], k, mode)
        st = impl.level_step(k == 0, k + 1 < calls, p0, sigma, grad, h, tol, max_step, max_move, st)
        snaps.append({key: st[key].copy() for key in STATE_KEYS})
    return snaps


def _radius_error(p):
    return np.abs(np.linalg.norm(p.astype(np.float64), axis=1) - LEVEL_R)


def check_level_step(impl):
    R, p0 = LEVEL_R, level_points()
    tol = 3e-5  # in h = k (R - |p|): |h| <= tol is ||p| - R| <= 1e-5 = 0.5e-5 R, so CONVERGED implies the bar below
    # loose clamps: h is linear along its gradient, so one Newton step is exact up to fp32 rounding (of order 1e-7 R)
    snaps = drive(impl, p0, 2, tol, 10 * R, 10 * R)
    st = snaps[-1]
    print("level step, loose clamps: max ||p| - R| after the second evaluation %.3g (R = %g)" % (_radius_error(st["best"]).max(), R))
    assert (st["status"] == rr.CONVERGED).all() and (_radius_error(st["best"]) <= 1e-5 * R).all() and (st["evals"] <= 2).all()
    assert (np.abs(st["h_best"]) <= np.abs(snaps[0]["h_best"])).all()
    # short steps: several evaluations, STEP_CLAMPED on every point that started further than a step away, all converged in the end
    snaps = drive(impl, p0, 8, tol, 0.05 * R, 10 * R)
    st = snaps[-1]
    far = _radius_error(p0) > 0.05 * R * 1.01  # (what is left after the clamped step is well above tol)
    assert far.sum() > 2000 and ((st["status"][far] & rr.STEP_CLAMPED) != 0).all() and (st["evals"][far] >= 3).all()
    assert ((st["status"] & rr.CONVERGED) != 0).all() and (st["status"] & (rr.EMPTY | rr.MOVE_CLAMPED) == 0).all()
    assert (st["evals"][_radius_error(p0) > 0.15 * R] >= 5).all() and st["evals"].max() <= 6
    for a, b in zip(snaps[:-1], snaps[1:]):
        assert (np.abs(b["h_best"]) <= np.abs(a["h_best"])).all()
    # a small trust region: the far points end on the ball around their start, the near ones converge
    mm = F32(0.1 * R)
    snaps = drive(impl, p0, 6, tol, 10 * R, mm)
    st = snaps[-1]
    far, near = _radius_error(p0) > float(mm) * 1.01, _radius_error(p0) < float(mm) * 0.99
    moved = np.linalg.norm(st["best"].astype(np.float64) - p0.astype(np.float64), axis=1)
    print("level step, max_move = 0.1 R: %d far points, |p - p0| / max_move in [%.9f, %.9f]" % (far.sum(), (moved[far] / float(mm)).min(),
                                                                                             (moved[far] / float(mm)).max()))
    assert far.sum() > 1000 and ((st["status"][far] & rr.MOVE_CLAMPED) != 0).all() and ((st["status"][far] & rr.CONVERGED) == 0).all()
    assert (moved <= float(mm) * (1 + 2.0 ** -22)).all()
    assert (moved[far] >= float(mm) * (1 - 2.0 ** -15)).all()  # (at most 16 rounds that each pull in by less than 2^-20)
    assert near.sum() > 1000 and (st["status"][near] == rr.CONVERGED).all()
    # a field without density at the start: EMPTY, the position's bits unchanged, no second evaluation counted
    snaps = drive(impl, p0, 3, tol, 10 * R, 10 * R, mode="empty")
    st = snaps[-1]
    assert (st["status"] == rr.EMPTY).all() and rr.same_bits(st["best"], p0) and rr.same_bits(st["cand"], p0) and (st["evals"] == 1).all()
    # an adversarial field (the gradient's sign wrong on the odd evaluations): |h| never grows, the step scale halves
    snaps = drive(impl, p0, 6, 0.0, 10 * R, 10 * R, mode="flip")
    for a, b in zip(snaps[:-1], snaps[1:]):
        assert (np.abs(b["h_best"]) <= np.abs(a["h_best"])).all()
    # the first gradient points the wrong way, so every candidate is worse than the start: none is accepted, the scale halves every time
    assert (snaps[1]["scale"] == 0.5).all() and (snaps[-1]["scale"] == 2.0 ** -5).all()
    assert rr.same_bits(snaps[-1]["best"], p0) and (snaps[-1]["status"] & (rr.CONVERGED | rr.EMPTY) == 0).all() and (snaps[-1]["evals"] == 6).all()


# ---- bit for bit against the restatement -------------------------------------------------------------------------------------------
SMOOTH_CASES = ("octahedron", "plane_jitter", "fan", "sphere")


def smooth_case(name, mesh_fn):
    if name == "octahedron":
        return octahedron() + (0.3,)
    if name == "plane_jitter":
        return plane(jitter=0.3) + (0.05,)
    if name == "fan":
        return fan() + (0.1,)
    return sphere(mesh_fn) + (0.1,)


def check_bits(impl, mesh_fn, tag=""):
    """ring, smooth (with and without max_move), face quality and every state array of six level steps: the restatement's bits"""
    for name in SMOOTH_CASES:
        v, f, mm = smooth_case(name, mesh_fn)
        want = reference(tag + "ring_" + name, lambda: REF.ring(f, len(v)))
        got = impl.ring(f, len(v))
        assert all(rr.same_bits(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3], name
        for move in (INF, mm):
            want = reference(tag + "smooth_%s_%g" % (name, move), lambda: rr.smooth(v, f, 3, 0.5, -0.53, move))
            assert rr.same_bits(impl.smooth(v, f, 3, 0.5, -0.53, move), want), (name, move)
            if np.isfinite(move):  # the clamp holds, up to the grid of the coordinates themselves (include/f2n_abi.h)
                d = np.linalg.norm(want.astype(np.float64) - v, axis=1)
                assert d.max() <= move * (1 + 2.0 ** -22) + 0.87 * np.spacing(F32(np.abs(want).max())), (name, d.max())
                assert name != "octahedron" or d.max() >= 0.99 * move  # (and it acted)
        want = reference(tag + "quality_" + name, lambda: rr.face_quality(v, f))
        assert rr.same_bits(impl.quality(v, f), want), name
    for two in (two_triangles(),):
        assert all(rr.same_bits(a, b) for a, b in zip(impl.ring(two[1], 4)[:3], REF.ring(two[1], 4)[:3]))
    p0 = level_points()
    for mode, args in (("plain", (1e-4, 0.05 * LEVEL_R, 0.1 * LEVEL_R)), ("flip", (0.0, 10.0, 10.0)), ("empty", (1e-4, 1.0, 1.0))):
        want = reference("level_%s" % mode, lambda: tuple(drive(REF, p0, 6, *args, mode=mode)))
        got = drive(impl, p0, 6, *args, mode=mode)
        for k, (a, b) in enumerate(zip(got, want)):
            for key in STATE_KEYS:
                assert rr.same_bits(a[key], b[key]), (mode, k, key)


def check_contract(impl, errors):
    """passes = 0, empty meshes, the arguments that are refused, vertices that are not finite"""
    v, f = octahedron()
    e3f, e3i = np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
    assert rr.same_bits(impl.smooth(v, f, 0, 0.5, -0.53, INF), v) and rr.same_bits(impl.smooth(v, f, 0, 0.5, -0.53, 0.01), v)
    assert impl.smooth(e3f, e3i, 2, 0.5, -0.53, INF).shape == (0, 3) and impl.quality(e3f, e3i).shape == (0,)
    se, rg, pinned, counts = impl.ring(e3i, 0)
    assert se.shape == (0, 2) and rg.shape == (0,) and pinned.shape == (0,) and counts == [0, 0]
    se, rg, pinned, counts = impl.ring(e3i, 6)  # vertices without faces: all pinned, and smoothing leaves them alone
    assert (se == 0).all() and rg.shape == (0,) and pinned.tolist() == [1] * 6 and counts == [0, 0]
    assert rr.same_bits(impl.smooth(v, e3i, 2, 0.5, -0.53, INF), v)
    for bad in ((-1, 0.5, -0.53, INF), (1, float("nan"), -0.53, INF), (1, 0.5, float("inf"), INF), (1, 0.5, -0.53, 0.0), (1, 0.5, -0.53, -1.0),
                (1, 0.5, -0.53, float("nan"))):
        with pytest.raises(errors):
            impl.smooth(v, f, *bad)
    p0 = level_points(8)
    for bad in ((-1.0, 1.0, 1.0), (1e-3, 0.0, 1.0), (1e-3, 1.0, -2.0), (float("nan"), 1.0, 1.0), (1e-3, float("nan"), 1.0)):
        st = rr.level_state(8)
        st["cand"] = p0.copy()
        with pytest.raises(errors):
            impl.level_step(True, True, p0, *sphere_field(p0, 0), *bad, st)
    # a vertex that is not finite stays, and so does every vertex with it in its ring; the others move as the restatement says
    v2 = v.copy()
    v2[4, 1] = np.nan
    out = impl.smooth(v2, f, 2, 0.5, -0.53, INF)
    assert rr.same_bits(out, rr.smooth(v2, f, 2, 0.5, -0.53, INF)) and rr.same_bits(out[[0, 1, 2, 3, 4]], v2[[0, 1, 2, 3, 4]])
    assert not rr.same_bits(out[5], v2[5])
    v2[4, 1] = np.inf
    assert rr.same_bits(impl.smooth(v2, f, 2, 0.5, -0.53, 0.1), rr.smooth(v2, f, 2, 0.5, -0.53, 0.1))


# ---- the restatement alone ---------------------------------------------------------------------------------------------------------
def test_small_meshes_on_the_restatement():
    check_small_meshes(REF)


def test_face_quality_on_the_restatement():
    check_face_quality(REF)


def test_sphere_on_the_restatement(emul):
    check_sphere(REF, reference("mesher", lambda: emul_mesher(emul)))


def test_level_step_on_the_restatement():
    check_level_step(REF)


def test_contract_cases_on_the_restatement():
    check_contract(types.SimpleNamespace(ring=REF.ring, smooth=_checked_ref_smooth, quality=REF.quality, level_step=_checked_ref_level_step),
                   ValueError)


def _checked_ref_smooth(v, f, passes, lam, mu, max_move):
    if passes < 0 or not (np.isfinite(lam) and np.isfinite(mu)) or not max_move > 0:
        raise ValueError("mesh_smooth: bad argument")
    return rr.smooth(v, f, passes, lam, mu, max_move)


def _checked_ref_level_step(first, propose, p0, sigma, grad, h, tol, max_step, max_move, st):
    if not (tol >= 0 and max_step > 0 and max_move > 0):
        raise ValueError("level_step: bad argument")
    return rr.level_step(first, propose, p0, sigma, grad, h, tol, max_step, max_move, st)


# ---- the emulator ------------------------------------------------------------------------------------------------------------------
def test_small_meshes_on_the_emulator(emul):
    check_small_meshes(emul_impl(emul))


def test_face_quality_on_the_emulator(emul):
    check_face_quality(emul_impl(emul))


def test_level_step_on_the_emulator(emul):
    check_level_step(emul_impl(emul))


def test_emulator_matches_the_restatement(emul):
    check_bits(emul_impl(emul), reference("mesher", lambda: emul_mesher(emul)))


def test_sphere_on_the_emulator(emul):
    check_sphere(emul_impl(emul), reference("mesher", lambda: emul_mesher(emul)))


def test_contract_cases_on_the_emulator(emul):
    check_contract(emul_impl(emul), (ValueError, EmulError))


@pytest.mark.parametrize("schedule", [1, 2])
def test_results_do_not_depend_on_the_wave_schedule(emul, schedule):
    emul.wemu_set_schedule(schedule)
    try:
        check_bits(emul_impl(emul), reference("mesher", lambda: emul_mesher(emul)))
    finally:
        emul.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))


def test_error_codes_of_the_entry_points(emul):
    L = emul
    v, f = octahedron()
    se, rg, pinned, _ = rr.ring(f, 6)
    keys, out, q = np.zeros((8, 6), np.int64), np.zeros((6, 3), F32), np.zeros(8, np.float64)
    ek, uses = rr.edges_of(rr.ring_keys(f, 6))
    counts = np.zeros(2, np.int32)
    assert L.f2n_mesh_ring_keys(None, -1, 8, _vp(f), _vp(keys)) == INVALID and L.f2n_mesh_ring_keys(None, 6, 8, None, _vp(keys)) == INVALID
    assert L.f2n_mesh_ring_keys(None, 6, 8, _vp(f), None) == INVALID and L.f2n_mesh_ring_keys(None, 6, 0, None, None) == 0
    assert L.f2n_mesh_ring_keys(None, 6, (2 ** 31 - 1) // 6 + 1, _vp(f), _vp(keys)) == INVALID
    assert L.f2n_mesh_ring_fill(None, 6, len(ek), _vp(ek), _vp(uses), _vp(se.copy()), _vp(rg.copy()), _vp(pinned.copy()), None) == INVALID
    assert L.f2n_mesh_ring_fill(None, 6, len(ek), None, _vp(uses), _vp(se.copy()), _vp(rg.copy()), _vp(pinned.copy()), _vp(counts)) == INVALID
    assert L.f2n_mesh_ring_fill(None, 0, 0, None, None, None, None, None, _vp(counts)) == 0
    for factor in (float("nan"), float("inf")):
        assert L.f2n_mesh_smooth(None, 6, len(rg), _vp(v), _vp(se), _vp(rg), _vp(pinned), _d(factor), _vp(out)) == INVALID
    assert L.f2n_mesh_smooth(None, 6, len(rg), _vp(v), _vp(se), _vp(rg), _vp(pinned), _d(0.5), _vp(v)) == INVALID  # in place
    assert L.f2n_mesh_smooth(None, 6, len(rg), _vp(v), None, _vp(rg), _vp(pinned), _d(0.5), _vp(out)) == INVALID
    assert L.f2n_mesh_smooth(None, 0, 0, None, None, None, None, _d(0.5), None) == 0
    for mm in (0.0, -1.0, float("nan")):
        assert L.f2n_mesh_move_clamp(None, 6, _vp(v), _f(mm), _vp(out)) == INVALID
    assert L.f2n_mesh_move_clamp(None, 6, None, _f(1.0), _vp(out)) == INVALID and L.f2n_mesh_move_clamp(None, 0, None, _f(1.0), None) == 0
    assert L.f2n_mesh_face_quality(None, 6, 8, _vp(v), _vp(f), None) == INVALID and L.f2n_mesh_face_quality(None, 6, -1, _vp(v), _vp(f), _vp(q)) == INVALID
    assert L.f2n_mesh_face_quality(None, 6, 0, None, None, None) == 0
    assert (keys == 0).all() and (out == 0).all() and (q == 0).all()  # nothing was written by any call above
    # a ring that does not fit the vertices is never followed: the vertex is copied through
    bad_se = se.copy()
    bad_se[0] = (0, len(rg) + 5)
    bad_rg = rg.copy()
    bad_rg[se[1, 0]] = 6
    assert L.f2n_mesh_smooth(None, 6, len(rg), _vp(v), _vp(bad_se), _vp(bad_rg), _vp(pinned), _d(0.5), _vp(out)) == 0
    assert rr.same_bits(out[:2], v[:2]) and rr.same_bits(out[2:], rr.smooth_pass(v, se, rg, pinned, 0.5)[2:])


# ---- the options -------------------------------------------------------------------------------------------------------------------
def test_options_parse_and_default():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    o = mesh.options(config.preset("wanjinyou", []))
    assert o["refine"] is None
    o = mesh.options(config.preset("wanjinyou", ["mesh.refine=true"]))
    assert o["refine"] == {"smooth_passes": 2, "lam": 0.5, "mu": -0.53, "project": True, "iters": 8, "max_step_steps": 0.5,
                           "max_move_steps": 1.0, "tol": 1e-3}
    o = mesh.options(config.preset("wanjinyou", ["mesh.refine=true", "refine.smooth_passes=0", "refine.project=false", "refine.iters=3",
                                                 "refine.max_move_steps=2", "refine.tol=0.01", "refine.lam=0.4", "refine.mu=-0.42",
                                                 "refine.max_step_steps=0.25"]))
    assert o["refine"] == {"smooth_passes": 0, "lam": 0.4, "mu": -0.42, "project": False, "iters": 3, "max_step_steps": 0.25,
                           "max_move_steps": 2.0, "tol": 0.01}
    # the TSDF surface is no density level set: project unset means off, set means an error
    assert mesh.options(config.preset("wanjinyou", ["mesh.refine=true", "mesh.source=tsdf"]))["refine"]["project"] is False
    with pytest.raises(ValueError):
        mesh.options(config.preset("wanjinyou", ["mesh.refine=true", "mesh.source=tsdf", "refine.project=true"]))
    for bad in ("refine.smooth_passes=-1", "refine.iters=0", "refine.max_step_steps=0", "refine.max_move_steps=-1", "refine.tol=-1",
                "refine.lam=nan", "refine.mu=inf", "refine.smooth_passes=two"):
        with pytest.raises(ValueError):
            mesh.options(config.preset("wanjinyou", ["mesh.refine=true", bad]))


def test_the_launcher_names_the_refined_file_and_passes_the_option(tmp_path, capsys):
    """mesh.refine=true: extract() writes the unrefined file as ever, asks the runner for the refined mesh with the option's dict and
    writes <name>_r.ply and <name>_r_refine.json; without the option the calls are today's."""
    import json
    import torch
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    v, f = octahedron()
    stats = {"points": 6, "empty": 0, "converged": 6, "h_median_before": 0.5, "h_median_after": 1e-4, "h_p90_before": 0.7, "h_p90_after": 2e-4,
             "moved_median": 0.1, "moved_p90": 0.2, "moved_max": 0.3, "quality_median_before": 0.5, "quality_p05_before": 0.1,
             "quality_median_after": 0.6, "quality_p05_after": 0.2, "flipped_faces": 0, "boundary_edges": 0, "nonmanifold_edges": 0}

    class Runner:
        iter_step = 60
        calls = []

        def extract_mesh(self, lo, hi, res, level):
            self.calls.append(("plain", res))
            return torch.from_numpy(v), torch.from_numpy(f)

        def extract_mesh_attrs(self, lo, hi, res, level, min_component_faces, normals, colors, normal_source, simplify=0, refine=None):
            self.calls.append(("attrs", res, simplify, refine))
            out = {"verts": torch.from_numpy(v * (0.5 if refine is not None else 1.0)), "faces": torch.from_numpy(f), "verts_in": 9, "faces_in": 8}
            if refine is not None:
                out["refine"] = dict(stats)
            return out

    scene = {"center": np.zeros(3, F32), "radius": 1.0}
    r = Runner()
    cfg = config.preset("wanjinyou", ["mesh.resolution=16", "mesh.refine=true", "refine.iters=5"])
    want = dict(mesh.options(cfg)["refine"])
    path = mesh.extract(r, cfg, scene, str(tmp_path))
    meshes = os.path.join(str(tmp_path), "meshes")
    assert path == os.path.join(meshes, "60_16_r.ply") and want["iters"] == 5
    assert r.calls == [("plain", 16), ("attrs", 16, 0, want)]
    import test_mesh_cpu
    pv, _ = test_mesh_cpu.read_ply(os.path.join(meshes, "60_16.ply"))
    rv, rf = test_mesh_cpu.read_ply(path)
    assert rr.same_bits(pv, v) and rr.same_bits(rv, (v * 0.5).astype(F32)) and (rf == f).all()
    assert json.load(open(os.path.join(meshes, "60_16_r_refine.json"))) == stats
    line = capsys.readouterr().out
    assert "Refine:" in line
    r.calls.clear()
    path = mesh.extract(r, config.preset("wanjinyou", ["mesh.resolution=16", "mesh.simplify=2", "mesh.refine=true"]), scene, str(tmp_path))
    assert path == os.path.join(meshes, "60_16_s2_r.ply") and os.path.exists(os.path.join(meshes, "60_16_s2.ply"))
    assert [c[:3] for c in r.calls] == [("attrs", 16, 2), ("attrs", 16, 2)] and r.calls[0][3] is None and r.calls[1][3] is not None
    r.calls.clear()
    capsys.readouterr()
    path = mesh.extract(r, config.preset("wanjinyou", ["mesh.resolution=16"]), scene, str(tmp_path))
    assert path == os.path.join(meshes, "60_16.ply") and r.calls == [("plain", 16)] and "Refine:" not in capsys.readouterr().out


# ---- the host layer ----------------------------------------------------------------------------------------------------------------
def tensor_impl(mod, dev):
    """an `impl` over a module with mesh_ring / mesh_smooth / mesh_face_quality / level_step on torch tensors (the host extension, the
    ctypes binding); dev(tensor) puts a tensor where that module wants it"""
    import torch

    def t(a, dt):
        return dev(torch.from_numpy(np.ascontiguousarray(a, dt)))

    def ring(faces, n_verts):
        se, rg, pinned, counts = mod.mesh_ring(t(faces, np.int32).reshape(-1, 3), int(n_verts))
        return se.cpu().numpy(), rg.cpu().numpy(), pinned.cpu().numpy(), [int(c) for c in counts]

    def smooth(verts, faces, passes, lam=0.5, mu=-0.53, max_move=INF):
        return mod.mesh_smooth(t(verts, F32).reshape(-1, 3), t(faces, np.int32).reshape(-1, 3), passes, lam, mu, max_move).cpu().numpy()

    def quality(verts, faces):
        return mod.mesh_face_quality(t(verts, F32).reshape(-1, 3), t(faces, np.int32).reshape(-1, 3)).cpu().numpy()

    def level_step(first, propose, p0, sigma, grad, h, tol, max_step, max_move, st):
        state = [t(st[k], st[k].dtype) for k in STATE_KEYS]
        mod.level_step(bool(first), bool(propose), t(p0, F32), t(sigma, F32), t(grad, F32), t(h, F32), tol, max_step, max_move, *state)
        for k, x in zip(STATE_KEYS, state):
            st[k] = x.cpu().numpy()
        return st

    return types.SimpleNamespace(ring=ring, smooth=smooth, quality=quality, level_step=level_step)


@pytest.fixture(scope="module")
def emul_host(emul):
    """the C++ host layer compiled against the emulated kernel library (tests/wave_emul/wemu_build.py build_host): on CPU tensors"""
    import importlib.util
    import wemu_build
    path = wemu_build.build_host()
    spec = importlib.util.spec_from_file_location("_f2n_host_emul", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_wrappers_on_the_emulator(emul, emul_host):
    """MeshRing, MeshSmooth, MeshFaceQuality and LevelStep of csrc/host/RendererQuery.cpp over the emulated kernels: the torch sort and run
    lengths in the place of numpy's, the argument checks"""
    impl = tensor_impl(emul_host, lambda x: x)
    check_small_meshes(impl)
    check_face_quality(impl)
    check_bits(impl, reference("mesher", lambda: emul_mesher(emul)))
    check_contract(impl, (ValueError, RuntimeError))
    import torch
    p0 = torch.zeros((4, 3))
    with pytest.raises(RuntimeError):  # a shape that does not match
        emul_host.level_step(True, True, p0, torch.ones(3), torch.zeros((4, 3)), torch.zeros(4), 1e-3, 1.0, 1.0, p0.clone(), p0.clone(), torch.zeros(4),
                             p0.clone(), torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError):  # a dtype that does not match
        emul_host.level_step(True, True, p0, torch.ones(4), torch.zeros((4, 3)), torch.zeros(4), 1e-3, 1.0, 1.0, p0.clone(), p0.clone(), torch.zeros(4),
                             p0.clone(), torch.zeros(4), torch.zeros(4), torch.zeros(4, dtype=torch.int32))
