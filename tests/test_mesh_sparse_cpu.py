"""Sparse meshing on bricks without a GPU: f2n_brick_mark, f2n_brick_mesh_count / _emit (csrc/octree.hip) and their host wrappers
(csrc/host/RendererQuery.cpp BrickMark, MeshFromBricks) under the wavefront emulator (tests/wave_emul), against the numpy restatement
of tests/mesh_sparse_ref.py and against the dense kernels' own output (f2n_mesh_count -> f2n_mesh_emit), bit for bit.  The checks are
functions of an `impl` (brick_mark, mesh_from_bricks, mesh_from_grid on numpy arrays): tests/test_gpu_mesh_sparse.py runs them on the
device through host.* and capi.*.  The check_huge_* bodies run the listed-brick kernels on windows of virtual grids whose corner indices,
keys and brick ids need more than 32 bits (tests/mesh_sparse_ref.py, HUGE_GRIDS)."""
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
import mesh_sparse_ref as sr  # noqa: E402

F32 = np.float32
_f, _i = ctypes.c_float, ctypes.c_int

# (lo, hi, res, B, active bricks, bricks) on the octree of tests/golden/fox_state.npz
FOX_CASES = [
    ((-1.0, -0.8, -0.9), (1.0, 0.7, 1.05), 40, 4, 460, 800),
    ((-3.0, -3.0, -3.0), (3.0, 3.0, 3.0), 48, 4, 995, 1728),
    ((-3.0, -3.0, -3.0), (3.0, 3.0, 3.0), 48, 8, 163, 216),
    ((-20.0, -20.0, -20.0), (20.0, 20.0, 20.0), 48, 4, 921, 1728),
]


def fox_tree():
    return np.array(np.load(os.path.join(ROOT, "tests", "golden", "fox_state.npz"))["tree_nodes"], np.uint8).reshape(-1)


def cut_tree(tree):
    """the fox tree with 40 child slots of interior nodes set to -1 (as tests/test_gpu_mesh.py::test_locate_agrees_with_a_numpy_descent)"""
    rng = np.random.default_rng(2)
    t = tree.copy().reshape(-1, 64)
    words = t.view(np.int32)
    interior = np.nonzero((words[:, 5:13] >= 0).any(1))[0]
    for u in rng.choice(interior[interior > 0], 40, replace=False):
        words[u, 5 + rng.integers(0, 8)] = -1
    return t.reshape(-1)


_REF_FLAGS = {}


def ref_flags(case, cut):
    """the restatement's flags of a fox case, computed once"""
    key = (case, cut)
    if key not in _REF_FLAGS:
        lo, hi, res, B = FOX_CASES[case][:4]
        step, n = sr.grid_spec(lo, hi, res)
        tree = cut_tree(fox_tree()) if cut else fox_tree()
        _REF_FLAGS[key] = (tree, step, n, sr.brick_mark(mr.parse_nodes(tree), lo, step, n, B))
    return _REF_FLAGS[key]


def check_brick_mark(impl, case, cut):
    lo, hi, res, B, active, total = FOX_CASES[case]
    tree, step, n, want = ref_flags(case, cut)
    flags = impl.brick_mark(tree, lo, step, n, B)
    assert flags.dtype == np.uint8 and flags.shape == want.shape and (flags == want).all()
    assert flags.size == total and 0 < int(flags.sum()) < total and set(np.unique(flags)) == {0, 1}
    if not cut:
        assert int(flags.sum()) == active
    return flags


def check_non_empty_points_lie_in_flagged_bricks(flags, case):
    """every grid point that mesh_ref.locate finds non-empty lies only in rows of flagged bricks"""
    lo, hi, res, B = FOX_CASES[case][:4]
    tree, step, n, _ = ref_flags(case, False)
    nodes = mr.parse_nodes(tree)
    ax = mr.grid_points(lo, step, n)
    flat = flags.reshape(-1)
    non_empty = 0
    for iz in range(n[2]):
        for iy in range(n[1]):
            for ix in range(n[0]):
                if mr.locate(nodes, [ax[0][ix], ax[1][iy], ax[2][iz]])[0] >= 0:
                    non_empty += 1
                    assert all(flat[b] for b in sr.bricks_reading((ix, iy, iz), n, B)), (ix, iy, iz)
    assert 0 < non_empty < n[0] * n[1] * n[2]


def mesh_cases():
    rng = np.random.default_rng(5)
    return [
        ("sphere", mr.sphere_grid(18, 6.2), 0.0, (0.0, 0.0, 0.0), 1.0),
        ("torus", mr.torus_grid(20, 5, 2.2), 0.0, (-1.0, 0.5, 2.0), 0.25),
        ("random", rng.uniform(-1, 1, (11, 7, 9)).astype(F32), 0.1, (0.5, -2.0, 1.0), 0.125),  # nx = 9: n - 1 a multiple of both B
    ]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_mesh_from_bricks(impl, B):
    for name, grid, level, lo, step in mesh_cases():
        nz, ny, nx = grid.shape
        n = (nx, ny, nz)
        nb = sr.n_bricks(n, B)
        assert any((n[k] - 1) % B for k in range(3))  # (clipped bricks are covered)
        dv, df = impl.mesh_from_grid(grid, level, lo, step)
        assert len(dv) > 0 and len(df) > 0
        every = np.arange(nb[0] * nb[1] * nb[2], dtype=np.int32)
        both = sr.bricks_with_both_sides(grid, level, B)
        assert 0 < len(both) <= len(every) and (name == "random" or len(both) < len(every))
        rng = np.random.default_rng(B)
        mixed = rng.permutation(both).astype(np.int32)
        # (one brick per batch: batches that own vertices but no face, and faces whose vertices all lie in other batches)
        for ids, batch in ((every, 0), (both, 0), (mixed, -(-len(mixed) // 3)), (both, 1)):
            values = sr.brick_values(grid, ids, B)  # (NaN where a corner does not exist: never read)
            v, f = impl.mesh_from_bricks(values, ids, n, lo, step, level, B, batch)
            assert f.dtype == np.int32 and same_bits(f, df), (name, B, len(ids), batch)
            assert v.dtype == F32 and same_bits(v, dv), (name, B, len(ids), batch)
        # the keys behind the order are the header's: as many as the dense mesh has vertices and faces
        vk, fk = sr.mesh_keys(grid, level)
        assert len(vk) == len(dv) and len(fk) == len(df) and len(np.unique(vk)) == len(vk) and (np.diff(fk) > 0).all()


def check_errors(impl):
    _, grid, level, lo, step = mesh_cases()[0]
    n = grid.shape[::-1]
    ids = sr.bricks_with_both_sides(grid, level, 4)
    values = sr.brick_values(grid, ids, 4)
    with pytest.raises(ValueError):  # a brick size that does not exist
        impl.mesh_from_bricks(sr.brick_values(grid, ids[:2], 5, 0.0), ids[:2], n, lo, step, level, 5, 0)
    with pytest.raises(ValueError):
        impl.brick_mark(fox_tree(), lo, step, n, 5)
    total = int(np.prod(sr.n_bricks(n, 4)))
    for bad in (total, -1):  # a brick id outside the grid
        with pytest.raises(ValueError):
            impl.mesh_from_bricks(values, np.concatenate([ids[:-1], [bad]]).astype(np.int32), n, lo, step, level, 4, 0)
    with pytest.raises(ValueError):  # a brick id listed twice
        impl.mesh_from_bricks(values, np.concatenate([ids[:-1], ids[:1]]).astype(np.int32), n, lo, step, level, 4, 0)
    keep = np.arange(len(ids)) != len(ids) // 2
    with pytest.raises(ValueError):  # a list that lacks the owner of a face's vertex (a brick in the middle of the surface)
        impl.mesh_from_bricks(values[keep], ids[keep], n, lo, step, level, 4, 0)
    with pytest.raises(ValueError):  # 2^31 bricks or more
        impl.brick_mark(fox_tree(), lo, step, (1 << 19, 1 << 19, 1 << 19), 4)


# ---- virtual grids whose indices need more than 32 bits (tests/mesh_sparse_ref.py, HUGE_GRIDS) -----------------------------------
_HUGE = {}


def huge_case(name, which):
    """(window, its dense sub-grid of an analytic sphere, the rows of its bricks, the restatement's mesh of the sub-grid): built once"""
    if (name, which) not in _HUGE:
        w = sr.huge_window(name, which)
        g = sr.window_sphere(w)
        rv, rf = mr.marching_tets(g, 0.0, w["lo_w"], w["step"])
        values = sr.brick_values(g, w["local_ids"], w["B"])  # (NaN where a corner does not exist: never read)
        for a in (g, values, rv, rf):
            a.setflags(write=False)
        _HUGE[(name, which)] = (w, g, values, rv, rf)
    return _HUGE[(name, which)]


def check_huge_magnitudes(name):
    """what the grids were chosen for, in Python integers"""
    far, inner = (sr.huge_magnitudes(sr.huge_window(name, which)) for which in ("far", "inner"))
    n, B = sr.HUGE_GRIDS[name]["n"], sr.HUGE_GRIDS[name]["B"]
    assert far["corner"] == n[0] * n[1] * n[2] - 1 and far["brick_id"] == far["bricks"] - 1  # the far window ends at the last corner
    for m in (far, inner):
        assert m["corner"] > 2 ** 36 and m["vertex_key"] > 2 ** 39 and m["face_key"] > 2 ** 39
    if name == "wide16":
        assert far["bricks"] == 2 ** 25 and far["brick_id"] > 2 ** 24 and inner["brick_id"] > 2 ** 24
    if name == "full":  # the most bricks the entry points accept along x and z, and a clipped last brick along x
        assert far["bricks"] == 131072 * 8191 * 2 == 2 ** 31 - 262144 and far["brick_id"] == 2 ** 31 - 262145 and inner["brick_id"] > 2 ** 30
        assert (n[0] - 1) % B == 3 and sr.huge_window(name, "far")["m"][0] == 4 * B
    (bad_n, bad_B) = sr.HUGE_REFUSED
    assert int(np.prod([int(v) for v in sr.n_bricks(bad_n, bad_B)], dtype=object)) == 2 ** 31


def check_huge_mesh_from_bricks(impl, name):
    """mesh_from_bricks over a window of a huge virtual grid = mesh_from_grid on the window's dense sub-grid with the translated lo, bit
    for bit (the translation is exact; vertex and face order is lexicographic in (z, y, x) on both sides) -- with the list ascending
    and shuffled, in one batch and in three; and the dense mesh is the restatement's."""
    check_huge_magnitudes(name)
    for which in ("far", "inner"):
        w, g, values, rv, rf = huge_case(name, which)
        n, B, lo, step = w["n"], w["B"], w["lo"], w["step"]
        dv, df = impl.mesh_from_grid(np.array(g), 0.0, w["lo_w"], step)  # (a copy: the cached grid is read-only)
        assert len(df) > 0 and df.dtype == np.int32 and same_bits(df, rf)
        assert dv.shape == rv.shape and np.abs(dv - rv).max() <= 1e-6 * step * max(1.0, np.abs(rv).max())
        ids = w["ids"]
        mixed = np.random.default_rng(B).permutation(len(ids))
        third = -(-len(ids) // 3)
        for order, batch in ((np.arange(len(ids)), 0), (mixed, 0), (np.arange(len(ids)), third), (mixed, third)):
            v, f = impl.mesh_from_bricks(values[order], ids[order], n, lo, step, 0.0, B, batch)
            assert f.dtype == np.int32 and same_bits(f, df), (name, which, batch)
            assert v.dtype == F32 and same_bits(v, dv), (name, which, batch)


# the first corner of a window of each grid inside the fox scene, where live and dead leaves of 4 to 16 steps meet (found on the CPU
# with mesh_ref.locate; the checks below assert that both kinds of point are there)
LOCATE_LO_W = {"wide16": (-0.4375, -0.6875, 0.3125), "wide8": (0.375, 0.375, -0.3125), "full": (0.6875, -0.3125, -0.125)}


def fox_transes():
    return np.array(np.load(os.path.join(ROOT, "tests", "golden", "fox_state.npz"))["pers_trans"], np.uint8).reshape(-1)


def check_huge_locate(loc, name):
    """loc.bricks(ids, lo, step, n, B, tree, transes) / loc.points(pts, tree, transes) -> (warped [m,3], anchors [m,3]): the rows of
    f2n_oct_locate_warp_bricks are f2n_oct_locate_warp's on the explicit corner coordinates; a corner beyond n - 1 is an empty point"""
    tree, transes = fox_tree(), fox_transes()
    nodes = mr.parse_nodes(tree)
    for which in ("far", "inner"):
        w = sr.huge_window(name, which, lo_w=LOCATE_LO_W[name])
        n, B, step = w["n"], w["B"], w["step"]
        order = np.random.default_rng(7).permutation(len(w["ids"]))
        warped, anchors = loc.bricks(w["ids"][order], w["lo"], step, n, B, tree, transes)
        idx, ex = (np.stack(a) for a in zip(*(sr.brick_corner_indices(int(b), w["m"], B) for b in w["local_ids"][order])))
        pts = (np.array(w["lo_w"])[None, None] + step * idx).astype(F32).reshape(-1, 3)  # (exact)
        ex = ex.reshape(-1)
        assert (~ex).any() == (name == "full" and which == "far")  # (the clipped last brick along x)
        rw, ra = loc.points(pts, tree, transes)
        assert warped.shape == rw.shape and anchors.shape == ra.shape and anchors.dtype == np.int32 and warped.dtype == F32
        assert same_bits(anchors[ex], ra[ex]) and same_bits(warped[ex], rw[ex])
        assert (anchors[~ex] == np.array([-1, -1, 0])).all() and (warped[~ex] == 0).all()
        empty = ra[ex, 0] < 0
        assert 0 < empty.sum() < ex.sum(), (name, which, int(empty.sum()))
        for j in np.random.default_rng(8).choice(np.flatnonzero(ex), 40, replace=False):  # (the oracle's own footing)
            assert tuple(anchors[j, :2]) == mr.locate(nodes, pts[j])


def check_huge_errors(impl):
    """exactly 2^31 bricks: refused before anything is allocated or launched"""
    n, B = sr.HUGE_REFUSED
    w, g, values, rv, rf = huge_case("full", "inner")
    with pytest.raises(ValueError):
        impl.brick_mark(fox_tree(), w["lo"], w["step"], n, B)
    with pytest.raises(ValueError):
        impl.mesh_from_bricks(np.array(values), w["ids"], n, w["lo"], w["step"], 0.0, B, 0)


# ---- the emulator ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


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


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _lo3(lo):
    return (_f * 3)(*(float(v) for v in lo))


def emul_brick_mark(L, tree, lo, step, n, B, flags=None):
    nb = sr.n_bricks(n, B) if B > 0 else (1, 1, 1)
    flags = np.full((nb[2], nb[1], nb[0]), 7, np.uint8) if flags is None else flags
    return L.f2n_brick_mark(None, _vp(np.ascontiguousarray(tree)), _lo3(lo), _f(step), _i(n[0]), _i(n[1]), _i(n[2]), _i(B), _vp(flags)), flags


def host_impl(host, wrap, unwrap):
    """impl over a host module (the emulated one here, the product's on the device); wrap / unwrap: numpy <-> its tensors"""
    def brick_mark(tree, lo, step, n, B):
        return unwrap(host.brick_mark(wrap(tree), [float(v) for v in lo], float(step), [int(v) for v in n], B))

    def mesh_from_bricks(values, ids, n, lo, step, level, B, batch):
        v, f = host.mesh_from_bricks(wrap(values), wrap(np.asarray(ids, np.int32)), [int(v) for v in n], [float(v) for v in lo], float(step),
                                     float(level), B, batch)
        return unwrap(v), unwrap(f)

    def mesh_from_grid(grid, level, lo, step):
        v, f = host.mesh_from_grid(wrap(grid), float(level), [float(v) for v in lo], float(step))
        return unwrap(v), unwrap(f)

    return types.SimpleNamespace(brick_mark=brick_mark, mesh_from_bricks=mesh_from_bricks, mesh_from_grid=mesh_from_grid)


@pytest.fixture(scope="module")
def impl(emul_host):
    import torch
    return host_impl(emul_host, lambda a: torch.from_numpy(np.ascontiguousarray(a)), lambda t: t.numpy())


@pytest.mark.parametrize("case", range(len(FOX_CASES)))
def test_brick_mark_equals_the_restatement(impl, emul, case):
    flags = check_brick_mark(impl, case, cut=False)
    lo, hi, res, B = FOX_CASES[case][:4]
    tree, step, n, want = ref_flags(case, False)
    rc, direct = emul_brick_mark(emul, tree, lo, step, n, B)  # the C entry point itself
    assert rc == 0 and (direct == flags).all()


def test_brick_mark_on_a_tree_with_missing_child_slots(impl):
    whole = check_brick_mark(impl, 0, cut=False)
    cut = check_brick_mark(impl, 0, cut=True)
    assert (cut <= whole).all() and (cut < whole).any()  # (cutting children can only clear flags, and here it does)


def test_non_empty_grid_points_lie_in_flagged_bricks_only(impl):
    check_non_empty_points_lie_in_flagged_bricks(check_brick_mark(impl, 0, cut=False), 0)


@pytest.mark.parametrize("B", [4, 8])
def test_mesh_from_bricks_equals_the_dense_kernels(impl, B):
    check_mesh_from_bricks(impl, B)


def test_dense_kernels_equal_the_restatement_on_the_random_grid(impl):
    """(the oracle's own footing: the shared device functions still produce mesh_ref's mesh)"""
    _, grid, level, lo, step = mesh_cases()[2]
    v, f = impl.mesh_from_grid(grid, level, lo, step)
    rv, rf = mr.marching_tets(grid, level, lo, step)
    assert same_bits(v, rv) and same_bits(f, rf)


def test_errors(impl, emul):
    check_errors(impl)
    tree = fox_tree()
    assert emul_brick_mark(emul, tree, (0, 0, 0), 1.0, (9, 9, 9), 5, np.zeros(8, np.uint8))[0] == -1        # F2N_ERR_INVALID_ARG
    assert emul_brick_mark(emul, tree, (0, 0, 0), 1.0, (9, 1, 9), 4, np.zeros(8, np.uint8))[0] == -1
    assert emul_brick_mark(emul, tree, (0, 0, 0), 1.0, (1 << 19,) * 3, 4, np.zeros(8, np.uint8))[0] == -2   # F2N_ERR_UNSUPPORTED


def emul_locate(L):
    """f2n_oct_locate_warp_bricks / f2n_oct_locate_warp themselves, on host arrays"""
    def out(m):
        return np.full((m, 3), 7, F32), np.full((m, 3), 7, np.int32)

    def bricks(ids, lo, step, n, B, tree, transes):
        ids = np.ascontiguousarray(ids, np.int32)
        w, a = out(len(ids) * (B + 1) ** 3)
        assert L.f2n_oct_locate_warp_bricks(None, _lo3(lo), _f(step), _i(n[0]), _i(n[1]), _i(n[2]), _i(B), _i(len(ids)), _vp(ids), _vp(tree),
                                            _vp(transes), _vp(w), _vp(a)) == 0
        return w, a

    def points(pts, tree, transes):
        pts = np.ascontiguousarray(pts, F32)
        w, a = out(len(pts))
        assert L.f2n_oct_locate_warp(None, _i(len(pts)), _vp(pts), _vp(tree), _vp(transes), _vp(w), _vp(a)) == 0
        return w, a

    return types.SimpleNamespace(bricks=bricks, points=points)


@pytest.mark.parametrize("name", sorted(sr.HUGE_GRIDS))
def test_mesh_from_bricks_on_a_huge_virtual_grid(impl, name):
    check_huge_mesh_from_bricks(impl, name)


@pytest.mark.parametrize("name", sorted(sr.HUGE_GRIDS))
def test_locate_warp_bricks_on_a_huge_virtual_grid(emul, name):
    check_huge_locate(emul_locate(emul), name)


def test_two_to_the_31_bricks_are_refused(impl, emul):
    check_huge_errors(impl)
    n, B = sr.HUGE_REFUSED
    rc, flags = emul_brick_mark(emul, fox_tree(), (0, 0, 0), 1.0, n, B, np.full(8, 7, np.uint8))
    assert rc == -2 and (flags == 7).all()  # F2N_ERR_UNSUPPORTED, nothing written
