"""Mesh ray casting without a GPU: the known answers of the numpy restatement (tests/mesh_raycast_ref.py), then f2n_mesh_raycast_count /
_fill / f2n_mesh_raycast (csrc/octree.hip) under the wavefront emulator (tests/wave_emul) against that restatement, bit for bit on t, face,
bary and the cell lists (both builds use -ffp-contract=off); the independence of the acceleration grid, ray order, face order and wave
schedule; the contract cases; compare_depth; the loop TSDF -> mesh -> ray cast; the check.* options.  The bodies that take a `Caster`
run against the device as well (tests/test_gpu_mesh_raycast.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import mesh_raycast_ref as rr  # noqa: E402
import mesh_ref as mr  # noqa: E402
import tsdf_ref as tr  # noqa: E402

F32 = np.float32
INVALID, UNSUPPORTED = -1, -2  # F2N_ERR_INVALID_ARG, F2N_ERR_UNSUPPORTED
_f, _i = ctypes.c_float, ctypes.c_int


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def _lo3(lo):
    return (_f * 3)(*(float(v) for v in lo))


def _dims3(dims):
    return (ctypes.c_int32 * 3)(*(int(v) for v in dims))


class EmulError(RuntimeError):
    def __init__(self, name, rc):
        RuntimeError.__init__(self, "%s failed with status %d" % (name, rc))
        self.rc = rc


def emul_build(L, verts, faces, cell=None, lo=None):
    """MeshRaycastBuild of csrc/host/RendererQuery.cpp call for call, numpy in the place of its torch plumbing (prefix sum, sort,
    searchsorted): (lo, cell, dims, cell_start, cell_faces)."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nv, nf = len(v), len(f)
    cell = rr.default_cell(v, f) if cell is None else float(F32(cell))
    if not (cell > 0 and cell < float("inf")):
        raise ValueError("cell must be positive and finite")
    lo3, dims = rr.grid_for(v, cell, lo)
    fin = v[np.isfinite(v).all(1)]
    if lo is not None and len(fin) and (lo3 > fin.min(0)).any():
        raise ValueError("the grid must cover the mesh")
    nc = int(dims[0]) * int(dims[1]) * int(dims[2])
    if nc > rr.MAX_CELLS:
        raise ValueError("more than 2^27 cells")
    counts, flag = np.zeros(nf, np.int32), np.zeros(1, np.int32)
    rc = L.f2n_mesh_raycast_count(None, nv, nf, _vp(v), _vp(f), _lo3(lo3), _f(cell), _dims3(dims), _vp(counts), _vp(flag))
    if rc != 0:
        raise EmulError("f2n_mesh_raycast_count", rc)
    ends = np.cumsum(counts, dtype=np.int64)
    total = int(ends[-1]) if nf else 0
    keys = np.full(total, -7, np.int64)
    if total:
        rc = L.f2n_mesh_raycast_fill(None, nv, nf, _vp(v), _vp(f), _lo3(lo3), _f(cell), _dims3(dims), _vp(np.ascontiguousarray(ends - counts)),
                                     _vp(keys))
        if rc != 0:
            raise EmulError("f2n_mesh_raycast_fill", rc)
    keys = np.sort(keys)
    m = max(nf, 1)
    cell_start = np.searchsorted(keys, np.arange(nc + 1, dtype=np.int64) * m).astype(np.int32)
    return [float(x) for x in lo3], cell, [int(x) for x in dims], cell_start, (keys % m).astype(np.int32)


def emul_cast(L, verts, faces, accel, rays_o, rays_d, bounds=None):
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    o, d = np.ascontiguousarray(rays_o, F32).reshape(-1, 3), np.ascontiguousarray(rays_d, F32).reshape(-1, 3)
    b = None if bounds is None else np.ascontiguousarray(bounds, F32).reshape(-1, 2)
    R = len(o)
    t, face, bary = np.zeros(R, F32), np.full(R, -1, np.int32), np.zeros((R, 3), F32)
    lo = cell = dims = cs = cf = None
    if accel is not None:
        lo, cell, dims, cs, cf = accel
        if not rr.in_domain(lo, cell, dims, o):
            raise ValueError("a ray origin lies outside the traversal's domain")
        cs, cf = np.ascontiguousarray(cs, np.int32), np.ascontiguousarray(cf, np.int32)
    rc = L.f2n_mesh_raycast(None, len(v), len(f), _vp(v), _vp(f), None if lo is None else _lo3(lo), _f(cell or 0.0),
                            None if dims is None else _dims3(dims), None if cs is None else cs.ctypes.data_as(ctypes.c_void_p),
                            None if cf is None else _vp(cf), R, _vp(o), _vp(d), None if b is None else _vp(b), _vp(t), _vp(face), _vp(bary))
    if rc != 0:
        raise EmulError("f2n_mesh_raycast", rc)
    return t, face, bary


class Caster:
    """build(v, f, cell=None, lo=None) -> accel; cast(v, f, accel or None, o, d, bounds=None) -> (t, face, bary) as numpy arrays;
    error: what a status code of the library raises"""
    def __init__(self, build, cast, error):
        self.build, self.cast, self.error = build, cast, error


def emul_caster(L):
    return Caster(lambda *a, **k: emul_build(L, *a, **k), lambda *a, **k: emul_cast(L, *a, **k), EmulError)


# ---- meshes and rays ---------------------------------------------------------------------------------------------------------------
_meshes = {}
FOX_LO, FOX_STEP = (-1.0, -1.0, -1.0), float(F32(2.0 / 255.0))


def grid_of(name):
    if name.startswith("sphere"):
        n = int(name[6:])
        return mr.sphere_grid(n, 0.4 * (n - 1)), 0.0
    if name == "torus32":
        return mr.torus_grid(32, 9.0, 3.5), 0.0
    if name == "noise":  # the non-manifold grid of test_mesh_simplify_cpu's random_k2
        return np.random.default_rng(11).standard_normal((20, 19, 22)).astype(F32), 0.8
    raise KeyError(name)


def get_mesh(name, mesh_fn, lo=(0.0, 0.0, 0.0), step=1.0):
    """mesh_fn(grid, level, lo, step) -> (verts, faces); made once per process, mesher and frame"""
    key = (name, id(mesh_fn), tuple(lo), step)
    if key not in _meshes:
        g, level = grid_of(name)
        v, f = mesh_fn(g, level, lo, step)
        v.setflags(write=False)
        f.setflags(write=False)
        _meshes[key] = (v, f)
    return _meshes[key]


def emul_mesher(L):
    from test_tsdf_cpu import emul_mesh as em

    def fn(g, level, lo=(0.0, 0.0, 0.0), step=1.0):
        o = em(L, g, None, level, lo, step)
        return o["verts"], o["faces"]
    return _mesher_once(L, fn)


_mesher_cache = {}


def _mesher_once(key, fn):  # (one function object per library: get_mesh caches by it)
    return _mesher_cache.setdefault(id(key), fn)


def edges_of(f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return np.unique(np.sort(e, 1), axis=0)


INTERIOR = np.array([0.3, 0.2, 0.1])  # offset of the interior point from the sphere's centre: no special direction


def watertight_rays(v, f, n):
    """from an interior point at every vertex and every edge midpoint"""
    e = edges_of(f)
    targets = np.concatenate([v.astype(np.float64), 0.5 * (v[e[:, 0]].astype(np.float64) + v[e[:, 1]])])
    o = np.broadcast_to((n - 1) / 2.0 + INTERIOR, targets.shape).astype(F32)
    return o, (targets - o).astype(F32)


def lattice_rays(n, shape=None):
    """axis-parallel rays through every grid point along all three axes, and rays along (1,1,0) and (1,1,1) through cell corners; each
    cast in both directions from outside the grid.  Returns (o, d, n_axis_rays): the axis-parallel ones come first."""
    nx, ny, nz = shape or (n, n, n)
    o, d = [], []
    ext = (nx, ny, nz)
    for ax in range(3):
        a, b = [k for k in range(3) if k != ax]
        ia, ib = np.meshgrid(np.arange(ext[a]), np.arange(ext[b]), indexing="ij")
        for sign in (1.0, -1.0):
            p = np.zeros((ia.size, 3))
            p[:, a], p[:, b] = ia.reshape(-1), ib.reshape(-1)
            p[:, ax] = -2.0 if sign > 0 else ext[ax] + 1.0
            dd = np.zeros((ia.size, 3))
            dd[:, ax] = sign
            o.append(p)
            d.append(dd)
    n_axis = sum(len(x) for x in o)
    for dirn, plane in (((1.0, 1.0, 0.0), 1), ((1.0, 1.0, 1.0), 2)):
        a, b = [k for k in range(3) if k != plane]
        ia, ib = np.meshgrid(np.arange(ext[a]), np.arange(ext[b]), indexing="ij")
        p = np.zeros((ia.size, 3))
        p[:, a], p[:, b] = ia.reshape(-1), ib.reshape(-1)
        dv = np.array(dirn)
        o += [p - 2.0 * dv, p + (max(ext) + 2.0) * dv]
        d += [np.broadcast_to(dv, p.shape), np.broadcast_to(-dv, p.shape)]
    return np.concatenate(o).astype(F32), np.concatenate(d).astype(F32), n_axis


def outside_rays(n, count, seed=2):
    """unit rays from a shell of radius 2 n at points of a ball of radius 0.3 (n - 1) around the sphere's centre (radius 0.4 (n - 1)):
    every one hits; (o, d, analytic t)"""
    rng = np.random.default_rng(seed)
    c, r = (n - 1) / 2.0, 0.4 * (n - 1)
    u = rng.standard_normal((count, 3))
    o = c + 2.0 * n * u / np.linalg.norm(u, axis=1, keepdims=True)
    w = rng.standard_normal((count, 3))
    tgt = c + 0.3 * (n - 1) * rng.uniform(0, 1, (count, 1)) ** (1 / 3) * w / np.linalg.norm(w, axis=1, keepdims=True)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o32, d32 = o.astype(F32), d.astype(F32)
    oc = o32.astype(np.float64) - c
    dd = d32.astype(np.float64)
    a, b, cc = (dd * dd).sum(1), (dd * oc).sum(1), (oc * oc).sum(1) - r * r
    return o32, d32, (-b - np.sqrt(b * b - a * cc)) / a


def camera_rays(n, side, seed=0):
    """a side x side pinhole image of the n^3 sphere from outside its grid, row by row"""
    c = (n - 1) / 2.0
    eye = np.array([c + 1.9 * n, c + 0.7 * n, c - 1.1 * n])
    fwd = (c - eye) / np.linalg.norm(c - eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    a, b = np.meshgrid(np.linspace(-0.25, 0.25, side), np.linspace(-0.25, 0.25, side), indexing="ij")
    d = fwd[None] + a.reshape(-1, 1) * up[None] + b.reshape(-1, 1) * right[None]
    return np.broadcast_to(eye, d.shape).astype(F32), d.astype(F32)


_refs = {}


def reference(key, v, f, o, d, bounds=None):
    """the restatement's (t, face, bary) of a ray set: computed once per process, shared, never written to"""
    import hashlib
    h = hashlib.sha1()
    for a in (v, f, o, d) + (() if bounds is None else (bounds,)):
        h.update(np.ascontiguousarray(a).tobytes())
    key = h.hexdigest()  # (by content: a ray set that two bodies share is computed once)
    if key not in _refs:
        _refs[key] = rr.raycast(v, f, o, d, bounds)
        for a in _refs[key]:
            a.setflags(write=False)
    return _refs[key]


def same(out, ref):
    return all(rr.same_bits(a, b) for a, b in zip(out, ref))


# ---- bodies (rc: a Caster; mesh_fn: a mesher) ----------------------------------------------------------------------------------------
def check_watertight(rc, mesh_fn, every=1, brute_rays=0):
    """The 17^3 sphere from an interior point at every vertex and edge midpoint: no ray misses; the caster gives the restatement's bits
    (on every `every`-th ray), and so does its brute-force mode on the first brute_rays of them."""
    v, f = get_mesh("sphere17", mesh_fn)
    assert len(v) == 2234 and len(f) == 4464
    o, d = watertight_rays(v, f, 17)
    assert len(o) == 8930
    accel = rc.build(v, f)
    out = rc.cast(v, f, accel, o, d)
    print("watertightness: %d rays, %d missed" % (len(o), int((out[1] < 0).sum())))
    assert (out[1] >= 0).all()
    ref = reference(("sphere17", "watertight", every), v, f, o[::every], d[::every])
    assert (ref[1] >= 0).all()
    assert same([a[::every] for a in out], ref)
    if brute_rays:
        assert same(rc.cast(v, f, None, o[:brute_rays * every:every], d[:brute_rays * every:every]), [a[:brute_rays] for a in ref])
    return out


def axis_ray_hits_sphere(o, d, n):
    c, r = (n - 1) / 2.0, 0.4 * (n - 1)
    oc = o.astype(np.float64) - c
    dd = d.astype(np.float64)
    dist2 = (oc * oc).sum(1) - (oc * dd).sum(1) ** 2 / (dd * dd).sum(1)
    return dist2, r * r


def check_lattice(rc, mesh_fn, name, brute_rays=0):
    """Rays in the grid's own planes and through mesh vertices, in both directions: the restatement's bits with the default cell and with
    cells of one grid step (the rays then lie in the accel grid's cell planes)."""
    v, f = get_mesh(name, mesh_fn)
    n = int(name[-2:])
    o, d, n_axis = lattice_rays(n)
    if not name.startswith("sphere"):  # (more faces: every third ray keeps the restatement's time down)
        o, d, n_axis = o[::3], d[::3], 0
    ref = reference((name, "lattice"), v, f, o, d)
    if name.startswith("sphere"):  # axis-parallel rays through grid points hit or miss as the analytic sphere says
        dist2, r2 = axis_ray_hits_sphere(o[:n_axis], d[:n_axis], n)
        assert ((ref[1][:n_axis] >= 0) == (dist2 < r2)).all() and np.abs(dist2 - r2).min() > 1e-6
    assert (ref[1] >= 0).sum() > len(o) // 8
    for cell in (None, 1.0):
        assert same(rc.cast(v, f, rc.build(v, f, cell, (0.0, 0.0, 0.0)), o, d), ref), (name, cell)
    if brute_rays:
        pick = np.linspace(0, len(o) - 1, brute_rays).astype(int)
        assert same(rc.cast(v, f, None, o[pick], d[pick]), [a[pick] for a in ref])
    return ref


def check_known_answer(rc, mesh_fn, n=17, count=400):
    """Rays from outside at the sphere: |t - analytic| <= 0.2 grid steps (measured: 0.072 at 17^3 with these 400 rays; the issue's
    brute force over more rays gave 0.096 at 17^3 and 0.058 at 33^3)."""
    v, f = get_mesh("sphere%d" % n, mesh_fn)
    o, d, t_true = outside_rays(n, count)
    ref = reference(("sphere%d" % n, "outside", count), v, f, o, d)
    out = rc.cast(v, f, rc.build(v, f), o, d)
    assert same(out, ref) and (out[1] >= 0).all()
    err = np.abs(out[0].astype(np.float64) - t_true)
    print("sphere%d: max |t - analytic| = %.4f grid steps over %d rays" % (n, err.max(), count))
    assert err.max() <= 0.2
    return err.max()


def check_grid_independence(rc, mesh_fn, name="sphere17", side=40, lo=(0.0, 0.0, 0.0), step=1.0):
    """Four cell sizes -- one grid step, 2.5 steps, one cell for the whole mesh, the default -- and the brute-force mode: identical bits."""
    v, f = get_mesh(name, mesh_fn, lo, step)
    n = int(name[-2:])
    o, d = camera_rays(n, side)
    o, d = (o * F32(step) + np.asarray(lo, F32)).astype(F32), d
    brute = rc.cast(v, f, None, o, d)
    assert (brute[1] >= 0).sum() > len(o) // 4 and (brute[1] < 0).sum() > len(o) // 8
    dims_seen = set()
    for cell in (1.0 * step, float(F32(2.5) * F32(step)), 1e3 * step, None):
        accel = rc.build(v, f, cell)
        dims_seen.add(tuple(accel[2]))
        assert same(rc.cast(v, f, accel, o, d), brute), cell
    assert (1, 1, 1) in dims_seen and len(dims_seen) == 4
    return brute


def check_cell_cap(rc, mesh_fn):
    v, f = get_mesh("sphere17", mesh_fn)
    with pytest.raises(ValueError):
        rc.build(v, f, 12.8 / 600.0)  # 601^3 > 2^27 cells
    with pytest.raises(ValueError):
        rc.build(v, f, 1.0, (3.0, 0.0, 0.0))  # lo above the mesh: the grid would not cover it
    for bad in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError):
            rc.build(v, f, bad)


def check_origins(rc, mesh_fn):
    """Origins inside the grid, outside it, at the far end of the documented domain (2^15 cells from the frame's origin), beyond it (an
    error), rays that miss the grid box entirely and rays that graze a face of the box."""
    v, f = get_mesh("sphere17", mesh_fn)
    accel = rc.build(v, f, 1.0)
    lo, cell, dims = np.array(accel[0]), accel[1], np.array(accel[2])
    hi = lo + dims * cell
    c = 8.0
    rng = np.random.default_rng(7)
    tgt = c + rng.uniform(-3, 3, (64, 3))
    inside = c + rng.uniform(-3, 3, (64, 3))
    outside = c + 40.0 * np.where(rng.uniform(size=(64, 3)) < 0.5, -1.0, 1.0)
    u = rng.standard_normal((64, 3))
    far = 32768.0 * cell * u / np.abs(u).max(1, keepdims=True)  # the largest coordinate is exactly 2^15 cells
    o = np.concatenate([inside, outside, far]).astype(F32)
    d = (np.concatenate([tgt, tgt, tgt]) - o).astype(F32)
    # missing the box: parallel to x beside it; grazing: in the planes of the box's faces and just outside / inside them
    gy = np.array([lo[1], hi[1], np.nextafter(F32(lo[1]), F32(-1e9)), np.nextafter(F32(hi[1]), F32(1e9)), lo[1] - 5.0, hi[1] + 5.0, 8.0])
    graze_o = np.stack([np.full(len(gy), -3.0), gy, np.full(len(gy), 8.25)], 1)
    o = np.concatenate([o, graze_o]).astype(F32)
    d = np.concatenate([d, np.broadcast_to(np.array([1.0, 0.0, 0.0], F32), graze_o.shape)]).astype(F32)
    assert np.abs(o).max() == 32768.0 * cell
    ref = reference(("sphere17", "origins"), v, f, o, d)
    assert (ref[1][:128] >= 0).all() and (ref[1][128:192] >= 0).sum() > 32 and ref[1][-1] >= 0 and (ref[1][-3:-1] < 0).all()
    for a in (accel, rc.build(v, f)):
        assert same(rc.cast(v, f, a, o, d), ref)
    beyond = o.copy()
    beyond[130] = beyond[130] * F32(1.01)
    with pytest.raises(ValueError):
        rc.cast(v, f, accel, beyond, d)
    assert same(rc.cast(v, f, None, beyond[128:136], d[128:136])[1:2], [rr.raycast(v, f, beyond[128:136], d[128:136])[1]])  # brute: no domain


def check_windows(rc, mesh_fn):
    """t_min just beyond the first hit returns the far side (facing false), t_max short of it a miss, bounds None is (0, inf)."""
    v, f = get_mesh("sphere17", mesh_fn)
    o, d, _ = outside_rays(17, 96, seed=5)
    accel = rc.build(v, f)
    first = rc.cast(v, f, accel, o, d)
    assert (first[1] >= 0).all()
    inf = np.full(len(o), np.inf, F32)
    assert same(rc.cast(v, f, accel, o, d, np.stack([np.zeros(len(o), F32), inf], 1)), first)
    beyond = np.nextafter(first[0], inf)
    b = np.concatenate([np.stack([beyond, inf], 1), np.stack([np.zeros(len(o), F32), first[0]], 1), np.stack([first[0], beyond], 1),
                        np.stack([np.full(len(o), -np.inf, F32), inf], 1)]).astype(F32)
    o4, d4 = np.tile(o, (4, 1)), np.tile(d, (4, 1))
    ref = reference(("sphere17", "windows"), v, f, o4, d4, b)
    out = rc.cast(v, f, accel, o4, d4, b)
    assert same(out, ref)
    n = len(o)
    far = [a[:n] for a in out]
    assert (far[1] >= 0).all() and (far[0] > first[0] + 5).all()
    r = rr.render(v, f, o, d, *far)
    r0 = rr.render(v, f, o, d, *first)
    assert r0["facing"].all() and not r["facing"].any()
    assert (out[1][n:3 * n] < 0).all() and (out[0][n:3 * n] == 0).all() and (out[2][n:3 * n] == 0).all()  # (t_min, t_max) is open
    assert same([a[3 * n:] for a in out], first)  # nothing of the mesh lies behind these origins


def check_scaling_and_frame(rc, mesh_fn):
    """d scaled by 0.25 and by 7 (t counts in units of d), and the fox grid's frame: lo = -1, step = 2 / 255."""
    v, f = get_mesh("sphere17", mesh_fn)
    o, d, _ = outside_rays(17, 64, seed=6)
    accel = rc.build(v, f)
    base = rc.cast(v, f, accel, o, d)
    for s in (0.25, 7.0):
        ds = (d * F32(s)).astype(F32)
        out = rc.cast(v, f, accel, o, ds)
        assert same(out, reference(("sphere17", "scaled", s), v, f, o, ds))
        assert (out[1] == base[1]).all() and np.allclose(out[0] * s, base[0], rtol=1e-5)
    vf, ff = get_mesh("sphere17", mesh_fn, FOX_LO, FOX_STEP)
    of = (o * F32(FOX_STEP) + np.asarray(FOX_LO, F32)).astype(F32)
    ref = reference(("sphere17", "fox frame"), vf, ff, of, d)
    assert (ref[1] >= 0).all()
    for cell in (None, FOX_STEP):
        assert same(rc.cast(vf, ff, rc.build(vf, ff, cell, FOX_LO if cell else None), of, d), ref)


def check_order_independence(rc, mesh_fn):
    """Permuting the rays permutes the outputs; under a face permutation t is bit-equal and face maps through it wherever t is not tied."""
    v, f = get_mesh("sphere17", mesh_fn)
    o, d, _ = lattice_rays(17)
    o, d = o[::3], d[::3]
    accel = rc.build(v, f)
    base = rc.cast(v, f, accel, o, d)
    rng = np.random.default_rng(9)
    p = rng.permutation(len(o))
    assert same(rc.cast(v, f, accel, o[p], d[p]), [a[p] for a in base])
    fp = rng.permutation(len(f))  # new face j is old face fp[j]
    f2 = np.ascontiguousarray(f[fp])
    out = rc.cast(v, f2, rc.build(v, f2), o, d)
    assert rr.same_bits(out[0], base[0]) and ((out[1] >= 0) == (base[1] >= 0)).all()
    hit = base[1] >= 0
    mapped = np.where(hit, fp[np.maximum(out[1], 0)], -1)
    moved = hit & (mapped != base[1])  # only where another face gives the same t: rays through a vertex or an edge
    print("face order: %d of %d hits change their face under the permutation (ties of equal t)" % (moved.sum(), hit.sum()))
    assert hit.sum() > 300
    for r in np.flatnonzero(moved)[:50]:
        t2 = rr.raycast(v, f[[base[1][r], mapped[r]]], o[r:r + 1], d[r:r + 1])
        one = [rr.raycast(v, f[[k]], o[r:r + 1], d[r:r + 1])[0][0] for k in (base[1][r], mapped[r])]
        assert one[0] == one[1] == base[0][r] and t2[1][0] == 0


def octahedron():
    c, r = 5.13, 0.85
    v = np.array([[c + r, c, c], [c - r, c, c], [c, c + r, c], [c, c - r, c], [c, c, c + r], [c, c, c - r]], F32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def check_contract(rc):
    """R = 0 and F = 0; degenerate faces and faces with a vertex that is not finite are never hit; NaN / inf / zero directions miss; a face
    index out of range is F2N_ERR_INVALID_ARG."""
    v, f = octahedron()
    e3f, e3i = np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
    o = np.array([[5.0, 5.1, 9.0]] * 8, F32)
    d = np.array([[0, 0, -1], [0, 0, 0], [np.nan, 0, -1], [0, np.inf, -1], [0, -np.inf, 0], [0.01, 0.02, -1], [0, 0, 1], [1e-30, 0, -1e-30]], F32)
    for accel in (None, rc.build(v, f), rc.build(v, f, 0.25)):
        t, face, bary = rc.cast(v, f, accel, e3f, e3f)
        assert t.shape == (0,) and face.shape == (0,) and bary.shape == (0, 3)
        out = rc.cast(v, f, accel, o, d)
        assert same(out, rr.raycast(v, f, o, d))
        assert out[1].tolist()[:5] == [out[1][0], -1, -1, -1, -1] and out[1][0] >= 0 and out[1][5] >= 0 and out[1][6] == -1
    for vv, accel in ((v, None), (v, rc.build(v, e3i)), (e3f, rc.build(e3f, e3i))):
        t, face, bary = rc.cast(vv, e3i, accel, o, d)
        assert (face == -1).all() and (t == 0).all() and (bary == 0).all()
    # degenerate faces (a repeated index, three points on a line) and a face with a NaN / inf vertex in front of the octahedron
    v2 = np.concatenate([v, [[5.0, 5.1, 8.0], [4.0, 4.1, 8.0], [6.0, 6.1, 8.0], [np.nan, 5.0, 8.0], [np.inf, 5.0, 8.0], [3.0, 3.0, 8.0], [7.0, 3.0, 8.0],
                             [5.0, 9.0, 8.0]]]).astype(F32)
    f2 = np.concatenate([[[6, 6, 7], [6, 7, 8], [9, 11, 12], [10, 11, 12], [7, 8, 8]], f]).astype(np.int32)
    ref = rr.raycast(v2, f2, o, d)
    assert ref[1][0] >= 5
    for accel in (None, rc.build(v2, f2), rc.build(v2, f2, 0.5)):
        assert same(rc.cast(v2, f2, accel, o, d), ref)
    f3 = np.concatenate([f2, [[11, 12, 13]]]).astype(np.int32)  # and a proper face there: it is the first hit
    assert rc.cast(v2, f3, rc.build(v2, f3), o[:1], d[:1])[1][0] == len(f3) - 1
    for bad in ([0, 1, len(v)], [0, -1, 2]):
        fb = np.concatenate([f, [bad]]).astype(np.int32)
        with pytest.raises(rc.error) as e:
            rc.cast(v, fb, None, o, d)
        assert "-1" in str(e.value)
        with pytest.raises(rc.error) as e:
            rc.build(v, fb)
        assert "-1" in str(e.value)
        with pytest.raises(rc.error) as e:
            rc.cast(v, fb, rc.build(v, f), o, d)
        assert "-1" in str(e.value)


def check_non_manifold(rc, mesh_fn, count=1024):
    """The noise grid of the simplifier's random_k2 at level 0.8 (34 820 faces, non-manifold) with 1 024 random rays."""
    v, f = get_mesh("noise", mesh_fn)
    assert len(f) == 34820
    rng = np.random.default_rng(13)
    o = rng.uniform(-3, 24, (count, 3)).astype(F32)
    d = (rng.uniform(0, 20, (count, 3)) - o).astype(F32)
    ref = reference(("noise", "random", count), v, f, o, d)
    assert (ref[1] >= 0).sum() > count // 2
    assert same(rc.cast(v, f, rc.build(v, f), o, d), ref)
    return ref


# ---- the restatement alone ------------------------------------------------------------------------------------------------------
def numpy_mesher(g, level, lo=(0.0, 0.0, 0.0), step=1.0):
    return mr.marching_tets(g, level, lo, step)[:2]


def numpy_caster():
    def build(v, f, cell=None, lo=None):
        v, f = np.asarray(v, F32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)
        if len(f) and (f.min() < 0 or f.max() >= len(v)):
            raise ValueError("status -1")
        cell = rr.default_cell(v, f) if cell is None else float(F32(cell))
        if not (cell > 0 and cell < float("inf")):
            raise ValueError("cell")
        lo3, dims = rr.grid_for(v, cell, lo)
        fin = v[np.isfinite(v).all(1)]
        if (lo is not None and len(fin) and (lo3 > fin.min(0)).any()) or dims[0] * dims[1] * dims[2] > rr.MAX_CELLS:
            raise ValueError("grid")
        return [float(x) for x in lo3], cell, dims, None, None

    def cast(v, f, accel, o, d, bounds=None):
        if accel is not None and not rr.in_domain(accel[0], accel[1], accel[2], o):
            raise ValueError("domain")
        try:
            return reference(None, np.asarray(v, F32), np.asarray(f, np.int32), np.asarray(o, F32), np.asarray(d, F32), bounds)
        except ValueError:
            raise ValueError("status -1")
    return Caster(build, cast, ValueError)


def test_known_answers_of_the_restatement(emul):
    """The restatement on its own: watertight from inside (8 930 rays, none missed), the analytic sphere from outside (0.072 step at most),
    the lattice rays hit or miss as the analytic sphere says, the contract cases."""
    rc, mesher = numpy_caster(), emul_mesher(emul)
    check_watertight(rc, mesher)
    assert check_known_answer(rc, mesher) <= 0.2
    check_lattice(rc, mesher, "sphere17")
    check_contract(rc)
    check_windows(rc, mesher)


def test_the_emulated_mesher_is_the_numpy_one(emul):
    v, f = get_mesh("sphere17", emul_mesher(emul))
    rv, rf = numpy_mesher(*grid_of("sphere17"))
    assert rr.same_bits(v, rv) and rr.same_bits(f, rf)


# ---- the emulator against the restatement ---------------------------------------------------------------------------------------
def test_cell_lists_match_the_restatement(emul):
    mesher = emul_mesher(emul)
    for name, cell, lo in (("sphere17", None, None), ("sphere17", 1.0, (0.0, 0.0, 0.0)), ("sphere17", 2.5, (-0.3, 0.1, 0.2)), ("sphere17", 1e3, None),
                           ("torus32", None, None), ("noise", None, None)):
        v, f = get_mesh(name, mesher)
        a = emul_build(emul, v, f, cell, lo)
        cs, cf = rr.bin_faces(v, f, a[0], a[1], a[2])
        assert rr.same_bits(a[3], cs) and rr.same_bits(a[4], cf), (name, cell)
        n_occ = int((np.diff(cs) > 0).sum())
        print("%s cell %s: dims %s, %d entries for %d faces, %.1f faces per occupied cell" % (name, cell, a[2], len(cf), len(f), len(cf) / max(n_occ, 1)))
    v, f = octahedron()
    v2 = np.concatenate([v, [[np.nan, 5.0, 5.0]]]).astype(F32)
    f2 = np.concatenate([f, [[0, 1, 6]]]).astype(np.int32)
    a = emul_build(emul, v2, f2, 0.25)
    cs, cf = rr.bin_faces(v2, f2, a[0], a[1], a[2])
    assert rr.same_bits(a[3], cs) and rr.same_bits(a[4], cf) and 8 not in cf.tolist()


def test_watertight_from_inside_on_the_emulator(emul):
    check_watertight(emul_caster(emul), emul_mesher(emul), brute_rays=192)


@pytest.mark.parametrize("name", ["sphere17", "torus32"])
def test_lattice_rays_on_the_emulator(emul, name):
    check_lattice(emul_caster(emul), emul_mesher(emul), name, brute_rays=128)


def test_known_answer_on_the_emulator(emul):
    """max |t - analytic| = 0.072 grid steps at 17^3 (400 rays); the bar is 0.2"""
    check_known_answer(emul_caster(emul), emul_mesher(emul))


def test_the_acceleration_grid_does_not_change_a_bit(emul):
    rc, mesher = emul_caster(emul), emul_mesher(emul)
    brute = check_grid_independence(rc, mesher, "sphere09", side=16)
    v, f = get_mesh("sphere09", mesher)
    assert same(brute, rr.raycast(v, f, *camera_rays(9, 16)))
    check_cell_cap(rc, mesher)


def test_origins_on_the_emulator(emul):
    check_origins(emul_caster(emul), emul_mesher(emul))


def test_windows_on_the_emulator(emul):
    check_windows(emul_caster(emul), emul_mesher(emul))


def test_scaling_and_frame_on_the_emulator(emul):
    check_scaling_and_frame(emul_caster(emul), emul_mesher(emul))


def test_ray_and_face_order_on_the_emulator(emul):
    check_order_independence(emul_caster(emul), emul_mesher(emul))


@pytest.mark.parametrize("schedule", [1, 2])
def test_results_do_not_depend_on_the_wave_schedule(emul, schedule):
    emul.wemu_set_schedule(schedule)
    try:
        rc, mesher = emul_caster(emul), emul_mesher(emul)
        check_known_answer(rc, mesher)
        v, f = get_mesh("sphere09", mesher)
        o, d = camera_rays(9, 16)
        assert same(rc.cast(v, f, None, o, d), reference(("sphere09", "camera16"), v, f, o, d))
        a = emul_build(emul, v, f)
        cs, cf = rr.bin_faces(v, f, a[0], a[1], a[2])
        assert rr.same_bits(a[3], cs) and rr.same_bits(a[4], cf)
    finally:
        emul.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))


def test_contract_cases_on_the_emulator(emul):
    check_contract(emul_caster(emul))


def test_error_codes_of_the_entry_points(emul):
    L = emul
    v, f = octahedron()
    lo, dims = _lo3((4.0, 4.0, 4.0)), _dims3((8, 8, 8))
    counts, flag, offs, keys = np.zeros(8, np.int32), np.zeros(1, np.int32), np.zeros(8, np.int64), np.zeros(64, np.int64)
    o, d = np.array([[5.0, 5.1, 9.0]], F32), np.array([[0.0, 0.0, -1.0]], F32)
    t, face, bary = np.zeros(1, F32), np.zeros(1, np.int32), np.zeros((1, 3), F32)
    cs, cf = np.zeros(513, np.int32), np.zeros(1, np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    count = lambda **k: L.f2n_mesh_raycast_count(None, k.get("nv", 6), k.get("nf", 8), k.get("v", P(v)), k.get("f", P(f)), k.get("lo", lo),  # noqa: E731
                                                 _f(k.get("cell", 0.5)), k.get("dims", dims), k.get("counts", P(counts)), k.get("flag", P(flag)))
    cast = lambda **k: L.f2n_mesh_raycast(None, k.get("nv", 6), k.get("nf", 8), k.get("v", P(v)), k.get("f", P(f)), k.get("lo", lo),  # noqa: E731
                                          _f(k.get("cell", 0.5)), k.get("dims", dims), k.get("cs", P(cs)), P(cf), k.get("R", 1), k.get("o", P(o)),
                                          k.get("d", P(d)), None, k.get("t", P(t)), k.get("face", P(face)), k.get("bary", P(bary)))
    for cell in (0.0, -2.0, float("nan"), float("inf")):
        assert count(cell=cell) == INVALID and cast(cell=cell) == INVALID
    for bad in ((0, 8, 8), (8, -1, 8), (1024, 1024, 129)):  # the last: 2^27 + 2^20 cells
        assert count(dims=_dims3(bad)) == INVALID and cast(dims=_dims3(bad)) == INVALID
        assert L.f2n_mesh_raycast_fill(None, 6, 8, P(v), P(f), lo, _f(0.5), _dims3(bad), P(offs), P(keys)) == INVALID
    assert count(dims=_dims3((1024, 1024, 128))) == 0 and (counts > 0).all()
    counts[:] = 0
    assert count(lo=None) == INVALID and count(dims=None) == INVALID and count(lo=_lo3((0.0, float("nan"), 0.0))) == INVALID
    assert count(v=None) == INVALID and count(f=None) == INVALID and count(counts=None) == INVALID and count(flag=None) == INVALID
    assert count(nv=-1) == INVALID and count(nf=-1) == INVALID and count(nf=0, f=None, counts=None, flag=None) == 0
    assert cast(v=None) == INVALID and cast(f=None) == INVALID and cast(o=None) == INVALID and cast(d=None) == INVALID
    assert cast(t=None) == INVALID and cast(face=None) == INVALID and cast(bary=None) == INVALID and cast(R=-1) == INVALID
    assert cast(R=0, o=None, d=None, t=None, face=None, bary=None) == 0
    assert (t == 0).all() and (face == 0).all() and (counts == 0).all()  # nothing was written by any call above
    # the box part of the traversal's domain is host data: a grid further than 2^15 cells from the frame's origin is refused
    assert cast(lo=_lo3((4.0, 4.0, 20000.0))) == UNSUPPORTED and cast(cs=None, lo=_lo3((4.0, 4.0, 20000.0))) == 0
    assert face[0] >= 0 and abs(t[0] - 3.0) < 0.2  # (that last call was the brute-force mode: it ran)


def test_a_non_manifold_mesh_on_the_emulator(emul):
    check_non_manifold(emul_caster(emul), emul_mesher(emul))


# ---- compare_depth, render, options ------------------------------------------------------------------------------------------------
def compare_cases():
    rng = np.random.default_rng(21)
    n = 257
    tf, tm = rng.uniform(1, 3, n).astype(F32), rng.uniform(1, 3, n).astype(F32)
    hf, hm = rng.uniform(size=n) < 0.7, rng.uniform(size=n) < 0.6
    z, one = np.zeros(n, bool), np.ones(n, bool)
    yield tf, hf, tm, hm, 0.01
    yield tf, z, tm, hm, 0.01      # no field surface
    yield tf, hf, tm, z, 0.01      # no mesh surface
    yield tf, hf, tm, ~hf, 0.01    # never both
    yield tf, hf, tm, hf, 0.01     # never only one
    yield tf, one, tf, one, 0.5    # identical
    yield tf[:0], z[:0], tm[:0], z[:0], 1.0  # no ray
    yield tf[:1], one[:1], tm[:1], one[:1], 0.25


def check_compare_depth(compare_fn):
    """compare_fn(t_field, has_field, t_mesh, has_mesh, step) -> dict against the restatement and against numpy on a sorted copy"""
    keys = {"n_rays", "n_field", "n_mesh", "n_both", "completeness", "extra", "mean", "median", "p90", "max", "within_1", "within_2"}
    for tf, hf, tm, hm, step in compare_cases():
        out, ref = compare_fn(tf, hf, tm, hm, step), rr.compare_depth(tf, hf, tm, hm, step)
        assert set(out) == keys
        for k in keys:
            assert np.isfinite(out[k]) and abs(out[k] - ref[k]) <= 1e-6 * max(1.0, abs(ref[k])), (k, out[k], ref[k])
        both = hf & hm
        e = np.sort(np.abs(tm[both] - tf[both]) / F32(step))
        if len(e):
            assert out["median"] == float(e[min(len(e) - 1, len(e) // 2)]) and out["max"] == float(e[-1])
            assert out["p90"] == float(e[min(len(e) - 1, int(np.floor(0.9 * len(e))))])
            assert out["within_1"] == float((e <= 1).sum()) / len(e) and abs(out["mean"] - e.astype(np.float64).mean()) < 1e-6 * max(1, e.max())
        else:
            assert out["median"] == out["p90"] == out["max"] == out["mean"] == out["within_1"] == out["within_2"] == 0.0
        assert out["n_both"] == int(both.sum()) and out["completeness"] == (both.sum() / hf.sum() if hf.sum() else 0.0)
        assert out["extra"] == ((hm & ~hf).sum() / len(tf) if len(tf) else 0.0)


def test_compare_depth():
    import torch
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    check_compare_depth(lambda tf, hf, tm, hm, step: mesh.compare_depth(T(tf), T(hf), T(tm), T(hm), step))
    out = mesh.compare_depth(T(np.array([1.0, 2.0, 3.0, 4.0], F32)), T(np.array([True, True, True, False])),
                             T(np.array([1.5, 2.0, 9.0, 4.0], F32)), T(np.array([True, True, False, True])), 0.25)
    assert out == {"n_rays": 4, "n_field": 3, "n_mesh": 3, "n_both": 2, "completeness": 2 / 3, "extra": 0.25, "mean": 1.0, "median": 2.0, "p90": 2.0,
                   "max": 2.0, "within_1": 0.5, "within_2": 1.0}


def test_options_parse_and_default():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    assert mesh.check_options(config.preset("wanjinyou", [])) == {"check": False, "res_level": 4, "tau": 0.5, "min_opacity": 0.5, "max_views": 0}
    o = mesh.check_options(config.preset("wanjinyou", ["mesh.check=true", "check.res_level=16", "check.tau=0.25", "check.min_opacity=0.1",
                                                        "check.max_views=3"]))
    assert o == {"check": True, "res_level": 16, "tau": 0.25, "min_opacity": 0.1, "max_views": 3}
    for bad in ("check.res_level=0", "check.max_views=-1", "check.tau=0", "check.tau=1.5", "check.min_opacity=-0.5", "check.res_level=x"):
        with pytest.raises(ValueError):
            mesh.check_options(config.preset("wanjinyou", [bad]))
    assert "check" not in config.GROUP_DEFAULTS


def test_the_launcher_without_the_option_writes_what_it_wrote_and_with_it_needs_the_cameras(tmp_path, capsys):
    import torch
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    v, f = octahedron()

    class Runner:
        iter_step = 60

        def extract_mesh(self, lo, hi, res, level):
            return torch.from_numpy(v), torch.from_numpy(f)

    scene = {"center": np.zeros(3, F32), "radius": 1.0}
    path = mesh.extract(Runner(), config.preset("wanjinyou", ["mesh.resolution=16"]), scene, str(tmp_path))
    assert sorted(os.listdir(os.path.dirname(path))) == ["60_16.ply"]
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 1 and lines[0].startswith("Mesh: 6 vertices, 8 faces at level")
    before = open(path, "rb").read()
    with pytest.raises(ValueError) as e:
        mesh.extract(Runner(), config.preset("wanjinyou", ["mesh.resolution=16", "mesh.check=true"]), scene, str(tmp_path))
    assert "data set" in str(e.value) and open(path, "rb").read() == before


# ---- the loop: depth maps -> TSDF -> mesh -> ray cast ------------------------------------------------------------------------------------
def loop_rays(c, every):
    """the rays of tsdf_ref.sphere_depth_maps' pixels (float64 there, float32 here) with a surface, every `every`-th: (o, d unit, depth)"""
    o, d, depth = [], [], []
    h, w = c["h"], c["w"]
    a, b = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    for vw in range(len(c["poses"])):
        P, K, k = (np.asarray(c[n][vw], np.float64) for n in ("poses", "intri", "dist"))
        xd, yd = (b + 0.5 - K[0, 2]) / K[0, 0], (a + 0.5 - K[1, 2]) / K[1, 1]
        u, vv = xd.copy(), yd.copy()
        for _ in range(50):
            r2 = u * u + vv * vv
            radial = k[0] * r2 + k[1] * r2 * r2
            u, vv = (xd - (u * radial + 2 * k[2] * u * vv + k[3] * (r2 + 2 * u * u)),
                     yd - (vv * radial + 2 * k[3] * u * vv + k[2] * (r2 + 2 * vv * vv)))
        dd = np.stack([u, -vv, -np.ones_like(u)], -1) @ P[:, :3].T
        dd /= np.linalg.norm(dd, axis=-1, keepdims=True)
        keep = c["conf"][vw] > 0
        o.append(np.broadcast_to(P[:, 3], dd.shape)[keep])
        d.append(dd[keep])
        depth.append(c["depth"][vw][keep])
    o, d, depth = np.concatenate(o)[::every], np.concatenate(d)[::every], np.concatenate(depth)[::every]
    return o.astype(F32), d.astype(F32), depth.astype(np.float64)


def check_loop_closure(rc, fused_mesh, c):
    """Depth maps of a sphere -> tsdf_integrate -> the masked mesher -> ray cast from the same cameras: where the mesh has a surface,
    |t_mesh - depth| stays within the bar.  Measured with the restatements on the CPU at 32^3 over every 5th ray with a surface: 0.39 grid steps at most
    (median 0.035); the bar is twice that, 0.78 steps, below the one step the TSDF test allows its vertices."""
    v, f = fused_mesh
    o, d, depth = loop_rays(c, 5)
    assert len(o) > 1500
    ref = reference(("loop", len(f), len(o)), v, f, o, d)
    out = rc.cast(v, f, rc.build(v, f), o, d)
    assert same(out, ref)
    hit = out[1] >= 0
    err = np.abs(out[0][hit].astype(np.float64) - depth[hit]) / float(c["step"])
    print("loop closure: %d of %d rays hit, |t_mesh - depth| max %.3f, median %.3f grid steps" % (hit.sum(), len(o), err.max(), np.median(err)))
    assert hit.sum() > 0.8 * len(o)
    assert err.max() <= LOOP_BAR
    return err.max()


LOOP_BAR = 0.78


def test_loop_closure_on_the_emulator(emul, fox_state):
    from test_tsdf_cpu import emul_finalize, emul_integrate, emul_mesh, sphere_case
    c, _ = sphere_case(fox_state, 32)
    S, W = np.zeros((32, 32, 32), F32), np.zeros((32, 32, 32), F32)
    assert emul_integrate(emul, c, S, W) == 0
    g, valid = emul_finalize(emul, S, W, 1.0)
    m = emul_mesh(emul, g, valid, 0.0, c["lo"], c["step"])
    check_loop_closure(emul_caster(emul), (m["verts"], m["faces"]), c)
