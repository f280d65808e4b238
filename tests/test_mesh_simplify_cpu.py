"""Mesh simplification without a GPU: the algorithm's known answers on the numpy restatement alone (tests/mesh_simplify_ref.py), then
f2n_mesh_cluster_keys / _accumulate / _place / _faces (csrc/octree.hip) under the wavefront emulator (tests/wave_emul) against that
restatement, bit for bit (both builds use -ffp-contract=off): vertices, faces, vert_map and the raw int64 accumulators; the contract
cases; independence of face order, vertex numbering and wave schedule; the mesh.simplify option.  The bodies that take a
`simplify_fn` run against the device as well (tests/test_gpu_mesh_simplify.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import mesh_ref as mr  # noqa: E402
import mesh_simplify_ref as sr  # noqa: E402

F32 = np.float32
INVALID, UNSUPPORTED = -1, -2  # F2N_ERR_INVALID_ARG, F2N_ERR_UNSUPPORTED
_f, _i, _d = ctypes.c_float, ctypes.c_int, ctypes.c_double


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _lo3(lo):
    return (_f * 3)(*(float(v) for v in lo))


def _dims3(dims):
    return (ctypes.c_int32 * 3)(*(int(v) for v in dims))


def emul_mesh(L, g, level, lo=(0.0, 0.0, 0.0), step=1.0):
    """f2n_mesh_count -> f2n_mesh_emit under the emulator (held to mesh_ref.marching_tets by tests/test_mesh_cpu.py): the input meshes"""
    from test_tsdf_cpu import emul_mesh as em
    o = em(L, g, None, level, lo, step)
    return o["verts"], o["faces"]


class EmulError(RuntimeError):
    def __init__(self, name, rc):
        RuntimeError.__init__(self, "%s failed with status %d" % (name, rc))
        self.rc = rc


def emul_simplify(L, verts, faces, cell, lo=None, lam=1e-3, with_acc=False):
    """MeshSimplify of csrc/host/RendererQuery.cpp call for call, numpy in the place of its torch plumbing (the sorted uniques)."""
    def ck(rc, name):
        if rc != 0:
            raise EmulError(name, rc)
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nv, nf = len(v), len(f)
    lo3, dims = sr.grid_for(v, cell, lo)
    lo_c, dims_c = _lo3(lo3), _dims3(dims)
    key = np.full(nv, -7, np.int64)
    ck(L.f2n_mesh_cluster_keys(None, nv, _vp(v), lo_c, _f(cell), dims_c, _vp(key)), "f2n_mesh_cluster_keys")
    ckeys, cluster_of = sr.clusters(key)
    ckeys, cluster_of = np.ascontiguousarray(ckeys), np.ascontiguousarray(cluster_of)
    nc = len(ckeys)
    none = (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), np.full(nv, -1, np.int32))
    acc = np.zeros((nc, 16), np.int64)
    if nc == 0:
        return none + (acc,) if with_acc else none
    flag = np.full(1, 7, np.int32)
    ck(L.f2n_mesh_cluster_accumulate(None, nv, nf, _vp(v), _vp(f), _vp(cluster_of), nc, lo_c, _f(cell), dims_c, _vp(acc), _vp(flag)),
       "f2n_mesh_cluster_accumulate")
    cverts = np.full((nc, 3), np.nan, F32)
    ck(L.f2n_mesh_cluster_place(None, nc, _vp(acc), _vp(ckeys), lo_c, _f(cell), dims_c, _d(lam), _vp(cverts)), "f2n_mesh_cluster_place")
    if nf == 0:
        return none + (acc,) if with_acc else none
    rows = np.full((nf, 3), -7, np.int32)
    ck(L.f2n_mesh_cluster_faces(None, nv, nf, _vp(f), _vp(cluster_of), _vp(rows)), "f2n_mesh_cluster_faces")
    uf = np.unique(rows, axis=0)
    if len(uf) and uf[0, 0] < 0:
        uf = uf[1:]
    uf = np.ascontiguousarray(uf, np.int32)
    kf0 = len(uf)
    if kf0 == 0:
        return none + (acc,) if with_acc else none
    i32 = lambda *shape: np.full(shape, -7, np.int32)  # noqa: E731
    labels, comp, vkeep, vse, fkeep, fse, totals = np.zeros(nc, np.int32), i32(nc), i32(nc), i32(nc, 2), i32(kf0), i32(kf0, 2), i32(2)
    ck(L.f2n_mesh_filter_count(None, nc, kf0, _vp(uf), _vp(labels), 1, _vp(comp), _vp(vkeep), _vp(vse), _vp(fkeep), _vp(fse), _vp(totals)),
       "f2n_mesh_filter_count")
    kv, kf = (int(x) for x in totals)
    ov, src, of = np.full((kv, 3), np.nan, F32), i32(kv), i32(kf, 3)
    ck(L.f2n_mesh_filter_emit(None, nc, kf0, _vp(cverts), _vp(uf), _vp(vkeep), _vp(vse), _vp(fkeep), _vp(fse), _vp(ov), _vp(src), _vp(of)),
       "f2n_mesh_filter_emit")
    new_of_cluster = np.where(vkeep != 0, vse[:, 0], -1).astype(np.int32)
    vert_map = np.where(cluster_of >= 0, new_of_cluster[np.maximum(cluster_of, 0)], -1).astype(np.int32)
    return (ov, of, vert_map, acc) if with_acc else (ov, of, vert_map)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
PLANE_N = np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
PLANE_C = np.array([11.5, 11.5, 11.5])


def plane_grid(n=24):
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    return (-((x - PLANE_C[0]) * PLANE_N[0] + (y - PLANE_C[1]) * PLANE_N[1] + (z - PLANE_C[2]) * PLANE_N[2])).astype(F32)  # > 0 below


def octahedron():
    c, r = 5.13, 0.85  # neighbouring vertices sqrt(2) r = 1.2 apart
    v = np.array([[c + r, c, c], [c - r, c, c], [c, c + r, c], [c, c - r, c], [c, c, c + r], [c, c, c - r]], F32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


GRID_CASES = {  # name: (grid, level, k, cluster lo or None = the mesh grid's lo)
    "sphere33_k2": (lambda: mr.sphere_grid(33, 0.4 * 32), 0.0, 2, None),
    "sphere33_k3": (lambda: mr.sphere_grid(33, 0.4 * 32), 0.0, 3, None),
    "sphere65_k4": (lambda: mr.sphere_grid(65, 0.4 * 64), 0.0, 4, None),
    "plane24_k3": (plane_grid, 0.0, 3, None),
    "random_k2": (lambda: np.random.default_rng(11).standard_normal((20, 19, 22)).astype(F32), 0.8, 2, None),
    "torus32_k2": (lambda: mr.torus_grid(32, 9.0, 3.5), 0.0, 2, (-0.3, 0.1, 0.2)),
    "torus32_k3": (lambda: mr.torus_grid(32, 9.0, 3.5), 0.0, 3, (-0.3, 0.1, 0.2)),
}
_meshes = {}


def case_mesh(name, mesh_fn):
    """(verts, faces, cell, lo) of a case; mesh_fn(grid, level) -> (verts, faces) of the grid at lo 0, step 1.  The input meshes are made
    once per process and mesher."""
    grid, level, k, lo = GRID_CASES[name]
    key = (name.split("_")[0], id(mesh_fn))
    if key not in _meshes:
        _meshes[key] = mesh_fn(grid(), level)
    v, f = _meshes[key]
    return v, f, float(F32(k) * F32(1.0)), (0.0, 0.0, 0.0) if lo is None else lo


_refs = {}


def reference(name, v, f, cell, lo):
    """the restatement's (verts, faces, vert_map, acc) of a case: computed once, shared, never written to"""
    key = (name, v.tobytes()[:64], len(v), len(f))
    if key not in _refs:
        _refs[key] = sr.simplify(v, f, cell, lo, with_acc=True)
        for a in _refs[key]:
            a.setflags(write=False)
    return _refs[key]


def sphere_rms(v, n):
    c = (n - 1) / 2.0
    return float(np.sqrt(np.mean((np.linalg.norm(v.astype(np.float64) - c, axis=1) - 0.4 * (n - 1)) ** 2)))


def check_closed_manifold(v, f):
    assert set(mr.edge_face_counts(f).values()) == {2}
    assert mr.euler_characteristic(v, f) == 2


def check_known_answers(name, v, f, cell, lo, ov, of, vert_map):
    """The algorithm's known answers on a case's result (whoever computed it)."""
    sr.check_structure(v, f, cell, lo, ov, of, vert_map)
    print("%s: %d -> %d faces (x %.4f), %d -> %d vertices (x %.4f)" % (name, len(f), len(of), len(of) / max(len(f), 1), len(v), len(ov),
                                                                      len(ov) / max(len(v), 1)))
    assert len(of) < len(f)
    if name.startswith("sphere"):
        n = int(name[6:8])
        check_closed_manifold(ov, of)
        mv, _, _ = sr.simplify(v, f, cell, lo, mean_only=True)
        rms, rms_mean = sphere_rms(ov, n), sphere_rms(mv, n)
        print("%s: RMS distance to the sphere %.4f, with mean placement %.4f" % (name, rms, rms_mean))
        assert rms < rms_mean
    if name.startswith("plane"):
        dist = np.abs((ov.astype(np.float64) - PLANE_C) @ PLANE_N) / cell
        dist_in = np.abs((v.astype(np.float64) - PLANE_C) @ PLANE_N) / cell
        print("%s: distance to the plane in cells: max %.3g (input %.3g)" % (name, dist.max(), dist_in.max()))
        assert dist.max() <= 1e-4


# ---- the restatement alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere33_k2", "sphere33_k3", "sphere65_k4", "plane24_k3", "random_k2", "torus32_k2", "torus32_k3"])
def test_known_answers_of_the_restatement(emul, name):
    v, f, cell, lo = case_mesh(name, lambda g, level: emul_mesh(emul, g, level))
    if name == "random_k2":
        assert len(f) == 34820
    ov, of, vert_map, _ = reference(name, v, f, cell, lo)
    check_known_answers(name, v, f, cell, lo, ov, of, vert_map)
    if name == "random_k2":  # duplicates were merged, and walls thinner than a cell are two-sided sheets
        rows = set(map(tuple, of.tolist()))
        twins = sum(1 for a, b, c in rows if (a, c, b) in rows)
        print("random_k2: %d output faces, %d of them with a reversed twin" % (len(of), twins))
        assert twins > 0
        rows = sr.cluster_faces(f, sr.clusters(sr.keys(v, *_grid(v, cell, lo)))[1], len(v))
        assert len(of) <= (rows[:, 0] >= 0).sum()


def _grid(v, cell, lo):
    lo3, dims = sr.grid_for(v, cell, lo)
    return lo3, cell, dims


def check_octahedron(simplify_fn):
    v, f = octahedron()
    ov, of, vert_map = simplify_fn(v, f, 0.5, None, 1e-3)[:3]
    sr.check_structure(v, f, 0.5, None, ov, of, vert_map)
    assert len(ov) == 6 and len(of) == 8 and sorted(vert_map.tolist()) == list(range(6))
    # the vertex lies on all its planes and is its own cluster's mean: it is the exact minimiser
    ulp = np.spacing(np.abs(v).max(1).astype(F32))[:, None]
    assert (np.abs(ov[vert_map].astype(np.float64) - v.astype(np.float64)) <= 4 * ulp).all()
    print("octahedron: max |out - in| = %.3g (ulp %.3g)" % (np.abs(ov[vert_map] - v).max(), ulp.max()))
    # a second copy on vertices of its own, one face reversed: equal rows are merged, the reversed twin stays
    f2 = np.concatenate([f, f + 6, f[:1, ::-1] + 6]).astype(np.int32)
    dv, df, dmap = simplify_fn(np.concatenate([v, v]), f2, 0.5, None, 1e-3)[:3]
    assert len(dv) == 6 and len(df) == 9 and (dmap[:6] == dmap[6:]).all() and (dmap[:6] == vert_map).all()
    rows = set(map(tuple, df.tolist()))
    assert set(map(tuple, of.tolist())) < rows and sum(1 for a, b, c in rows if (a, c, b) in rows) == 2
    return ov, of, vert_map


def test_octahedron_on_the_restatement():
    check_octahedron(sr.simplify)


# ---- the emulator against the restatement ---------------------------------------------------------------------------------------
def check_case_bits(name, v, f, cell, lo, simplify_fn, with_acc):
    """simplify_fn(verts, faces, cell, lo, lam) -> (verts, faces, vert_map[, acc]): the restatement's bits"""
    rv, rf, rmap, racc = reference(name, v, f, cell, lo)
    out = simplify_fn(v, f, cell, lo, 1e-3)
    assert sr.same_bits(out[0], rv), name
    assert sr.same_bits(out[1], rf) and sr.same_bits(out[2], rmap), name
    if with_acc:
        assert sr.same_bits(out[3], racc), name
        assert racc[:, 11].max() > 3 and racc[:, 15].max() > 1
    return out


@pytest.mark.parametrize("name", ["sphere33_k2", "sphere33_k3", "sphere65_k4", "plane24_k3", "random_k2", "torus32_k2", "torus32_k3"])
def test_emulator_matches_the_restatement(emul, name):
    v, f, cell, lo = case_mesh(name, lambda g, level: emul_mesh(emul, g, level))
    check_case_bits(name, v, f, cell, lo, lambda *a: emul_simplify(emul, *a, with_acc=True), True)


@pytest.mark.parametrize("schedule", [1, 2])
def test_results_do_not_depend_on_the_wave_schedule(emul, schedule):
    emul.wemu_set_schedule(schedule)
    try:
        for name in ("random_k2", "torus32_k3"):
            v, f, cell, lo = case_mesh(name, lambda g, level: emul_mesh(emul, g, level))
            check_case_bits(name, v, f, cell, lo, lambda *a: emul_simplify(emul, *a, with_acc=True), True)
    finally:
        emul.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))


def test_octahedron_on_the_emulator(emul):
    out = check_octahedron(lambda *a: emul_simplify(emul, *a))
    ref = sr.simplify(*octahedron(), 0.5)
    assert all(sr.same_bits(a, b) for a, b in zip(out, ref))


def check_contract(simplify_fn, error_type, mesh_fn):
    """Empty meshes, invalid cells, vertices that are not finite, indices out of range, unused vertices, order independence."""
    e3f, e3i = np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
    ov, of, vm = simplify_fn(e3f, e3i, 1.0, None, 1e-3)[:3]
    assert ov.shape == (0, 3) and of.shape == (0, 3) and vm.shape == (0,)
    v, f = octahedron()
    ov, of, vm = simplify_fn(v, e3i, 0.5, None, 1e-3)[:3]  # vertices without faces: nothing is used
    assert ov.shape == (0, 3) and of.shape == (0, 3) and (vm == -1).all() and vm.shape == (6,)
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        for vv, ff in ((v, f), (e3f, e3i)):
            with pytest.raises(error_type) as e:
                simplify_fn(vv, ff, cell, None, 1e-3)
            assert "status -1" in str(e.value) or "-1" in str(e.value), (cell, str(e.value))
    # a NaN / infinite vertex, a face with an index >= V or < 0, vertices no face uses (one in a used cluster, one alone)
    v, f, cell, lo = case_mesh("torus32_k2", mesh_fn)
    rng = np.random.default_rng(5)
    v2 = np.concatenate([v, [[np.nan, 1.0, 2.0], [3.0, np.inf, 1.0], v[7], [40.0, 40.0, 40.0]]]).astype(F32)
    nan_v, inf_v, near_v, far_v = len(v), len(v) + 1, len(v) + 2, len(v) + 3
    f2 = np.concatenate([f, [[0, 1, len(v2)], [5, -1, 6], [nan_v, 10, 11], [12, inf_v, 13]]]).astype(np.int32)
    hit = rng.choice(len(f), 40, replace=False)
    f2[hit[:20], 1] = nan_v  # faces of the mesh that lose a corner to the NaN vertex: dropped, a hole
    rv, rf, rmap = sr.simplify(v2, f2, cell, lo)
    sr.check_structure(v2, f2, cell, lo, rv, rf, rmap)
    assert rmap[nan_v] == -1 and rmap[inf_v] == -1 and rmap[far_v] == -1 and rmap[near_v] == rmap[7]
    ov, of, vm = simplify_fn(v2, f2, cell, lo, 1e-3)[:3]
    assert sr.same_bits(ov, rv) and sr.same_bits(of, rf) and sr.same_bits(vm, rmap)
    # lo derived from the vertices: the finite coordinates of a vertex that is not finite count for the grid's extent, nothing else
    v, f = octahedron()
    v4 = np.concatenate([v, [[np.nan, 1.0, 2.0]]]).astype(F32)
    rv, rf, rmap = sr.simplify(v4, f, 0.5, None)
    assert rmap[6] == -1 and len(rf) == 8 and sr.grid_for(v4, 0.5)[0].tolist() == [v[:, 0].min(), 1.0, 2.0]
    ov, of, vm = simplify_fn(v4, f, 0.5, None, 1e-3)[:3]
    assert sr.same_bits(ov, rv) and sr.same_bits(of, rf) and sr.same_bits(vm, rmap)
    # order independence: the faces permuted, the vertices renumbered (faces re-indexed, corners not rotated): the same vertex bits and
    # the same face array
    v, f, cell, lo = case_mesh("plane24_k3", mesh_fn)
    rv, rf, rmap, _ = reference("plane24_k3", v, f, cell, lo)
    assert len(f) > 2000  # many waves, several blocks
    perm = rng.permutation(len(v))  # new index of old vertex i
    v3 = np.empty_like(v)
    v3[perm] = v
    f3 = perm[f[rng.permutation(len(f))]].astype(np.int32)
    ov, of, vm = simplify_fn(v3, f3, cell, lo, 1e-3)[:3]
    assert sr.same_bits(ov, rv) and sr.same_bits(of, rf) and sr.same_bits(vm[perm], rmap)


def test_contract_cases_on_the_emulator(emul):
    check_contract(lambda *a: emul_simplify(emul, *a), EmulError, lambda g, level: emul_mesh(emul, g, level))


def test_error_codes_of_the_entry_points(emul):
    v, f = octahedron()
    lo, dims = _lo3((4.0, 4.0, 4.0)), _dims3((4, 4, 4))
    key, rows = np.zeros(6, np.int64), np.zeros((8, 3), np.int32)
    acc, cof, ck, out, flag = np.zeros((6, 16), np.int64), np.arange(6, dtype=np.int32), np.arange(6, dtype=np.int64), np.zeros((6, 3), F32), np.zeros(1, np.int32)
    L = emul
    for cell in (0.0, -2.0, float("nan"), float("inf")):
        assert L.f2n_mesh_cluster_keys(None, 6, _vp(v), lo, _f(cell), dims, _vp(key)) == INVALID
        assert L.f2n_mesh_cluster_accumulate(None, 6, 8, _vp(v), _vp(f), _vp(cof), 6, lo, _f(cell), dims, _vp(acc), _vp(flag)) == INVALID
        assert L.f2n_mesh_cluster_place(None, 6, _vp(acc), _vp(ck), lo, _f(cell), dims, _d(1e-3), _vp(out)) == INVALID
    for bad_dims in ((0, 4, 4), (4, -1, 4), (4, 4, (1 << 20) + 1)):
        assert L.f2n_mesh_cluster_keys(None, 6, _vp(v), lo, _f(0.5), _dims3(bad_dims), _vp(key)) == INVALID
    assert L.f2n_mesh_cluster_keys(None, 6, _vp(v), _lo3((0.0, float("nan"), 0.0)), _f(0.5), dims, _vp(key)) == INVALID
    assert L.f2n_mesh_cluster_keys(None, 6, _vp(v), None, _f(0.5), dims, _vp(key)) == INVALID
    assert L.f2n_mesh_cluster_keys(None, 6, _vp(v), lo, _f(0.5), None, _vp(key)) == INVALID
    assert L.f2n_mesh_cluster_keys(None, -1, _vp(v), lo, _f(0.5), dims, _vp(key)) == INVALID
    assert L.f2n_mesh_cluster_keys(None, 6, None, lo, _f(0.5), dims, _vp(key)) == INVALID
    assert L.f2n_mesh_cluster_keys(None, 0, None, lo, _f(0.5), dims, None) == 0
    for lam in (-1.0, float("nan"), float("inf")):
        assert L.f2n_mesh_cluster_place(None, 6, _vp(acc), _vp(ck), lo, _f(0.5), dims, _d(lam), _vp(out)) == INVALID
    assert L.f2n_mesh_cluster_place(None, 0, None, None, lo, _f(0.5), dims, _d(0.0), None) == 0
    assert L.f2n_mesh_cluster_accumulate(None, 6, 8, _vp(v), None, _vp(cof), 6, lo, _f(0.5), dims, _vp(acc), _vp(flag)) == INVALID
    assert L.f2n_mesh_cluster_accumulate(None, 6, 8, _vp(v), _vp(f), _vp(cof), 6, lo, _f(0.5), dims, None, _vp(flag)) == INVALID
    assert L.f2n_mesh_cluster_accumulate(None, 0, 0, None, None, None, 0, lo, _f(0.5), dims, None, None) == 0
    assert L.f2n_mesh_cluster_faces(None, 6, -1, _vp(f), _vp(cof), _vp(rows)) == INVALID
    assert L.f2n_mesh_cluster_faces(None, 6, 8, _vp(f), _vp(cof), None) == INVALID
    assert L.f2n_mesh_cluster_faces(None, 6, 0, None, None, None) == 0
    assert (key == 0).all() and (acc == 0).all() and (out == 0).all() and (rows == 0).all()  # nothing was written by any call above
    assert L.f2n_mesh_cluster_keys(None, 6, _vp(v), lo, _f(0.5), dims, _vp(key)) == 0 and len(set(key.tolist())) == 6 and key.min() >= 0


def strip(n_faces, seed=3):
    """a strip of n_faces triangles (i, i+1, i+2) over random points inside one cell of size 1 at the origin: no degenerate face"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.05, 0.95, (n_faces + 2, 3)).astype(F32)
    i = np.arange(n_faces, dtype=np.int32)
    return v, np.stack([i, i + 1, i + 2], 1).astype(np.int32)


def test_the_record_guard(emul):
    """More than 2^18 corner records in one cluster: F2N_ERR_UNSUPPORTED; exactly at the bound the sums are the restatement's."""
    n_ok = (1 << 18) // 3  # 87 381 faces: 262 143 records
    v, f = strip(n_ok + 20)
    lo, dims = _lo3((0.0, 0.0, 0.0)), _dims3((1, 1, 1))
    cof, flag = np.zeros(len(v), np.int32), np.zeros(1, np.int32)

    def run(nf):
        acc = np.zeros((1, 16), np.int64)
        rc = emul.f2n_mesh_cluster_accumulate(None, nf + 2, nf, _vp(v), _vp(f), _vp(cof), 1, lo, _f(1.0), dims, _vp(acc), _vp(flag))
        return rc, acc

    rc, acc = run(n_ok)
    assert rc == 0 and acc[0, 11] == 3 * n_ok <= 1 << 18 and acc[0, 15] == n_ok + 2
    assert sr.same_bits(acc, sr.accumulate(v[:n_ok + 2], f[:n_ok], cof[:n_ok + 2], 1, (0.0, 0.0, 0.0), 1.0, (1, 1, 1)))
    rc, acc = run(n_ok + 20)
    assert rc == UNSUPPORTED and acc[0, 11] == 3 * (n_ok + 20) > 1 << 18
    with pytest.raises(sr.Unsupported):
        sr.accumulate(v, f, cof, 1, (0.0, 0.0, 0.0), 1.0, (1, 1, 1))
    with pytest.raises(EmulError) as e:
        emul_simplify(emul, v, f, 1.0, (0.0, 0.0, 0.0))
    assert e.value.rc == UNSUPPORTED


def test_options_parse_and_default():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    assert mesh.options(config.preset("wanjinyou", []))["simplify"] == 0
    assert mesh.options(config.preset("wanjinyou", ["mesh.simplify=3"]))["simplify"] == 3
    assert mesh.options(config.preset("wanjinyou", ["mesh.simplify=1"]))["simplify"] == 1
    for bad in ("-1", "two", "2.5", "", "true"):
        with pytest.raises(ValueError):
            mesh.options(config.preset("wanjinyou", ["mesh.simplify=%s" % bad]))


def test_the_launcher_names_the_simplified_file_and_passes_the_option(tmp_path, capsys):
    """mesh.simplify=k >= 2: extract() asks the runner for simplify=k and writes <iter>_<res>_s<k>.ply; 0 and 1 leave call and name alone."""
    import torch
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    v, f = octahedron()

    class Runner:
        iter_step = 60
        calls = []

        def extract_mesh(self, lo, hi, res, level):
            self.calls.append(("plain", res))
            return torch.from_numpy(v), torch.from_numpy(f)

        def extract_mesh_attrs(self, lo, hi, res, level, min_component_faces, normals, colors, normal_source, simplify=0):
            self.calls.append(("attrs", res, min_component_faces, normals, colors, normal_source, simplify))
            return {"verts": torch.from_numpy(v), "faces": torch.from_numpy(f[:6]), "verts_in": 9, "faces_in": 8}

    scene = {"center": np.zeros(3, F32), "radius": 1.0}
    r = Runner()
    path = mesh.extract(r, config.preset("wanjinyou", ["mesh.resolution=16", "mesh.simplify=2"]), scene, str(tmp_path))
    assert path == os.path.join(str(tmp_path), "meshes", "60_16_s2.ply") and r.calls == [("attrs", 16, 0, False, False, "grid", 2)]
    line = capsys.readouterr().out
    assert "6 faces" in line and "from 8 faces" in line
    for k in (0, 1):
        r.calls.clear()
        path = mesh.extract(r, config.preset("wanjinyou", ["mesh.resolution=16", "mesh.simplify=%d" % k]), scene, str(tmp_path))
        assert path == os.path.join(str(tmp_path), "meshes", "60_16.ply") and r.calls == [("plain", 16)]
    r.calls.clear()
    mesh.extract(r, config.preset("wanjinyou", ["mesh.resolution=16", "mesh.simplify=3", "mesh.min_component_faces=5"]), scene, str(tmp_path))
    assert r.calls == [("attrs", 16, 5, False, False, "grid", 3)] and os.path.exists(os.path.join(str(tmp_path), "meshes", "60_16_s3.ply"))
