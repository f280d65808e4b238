"""Sparse meshing on bricks on the MI355X (csrc/octree.hip, host/RendererQuery.cpp): the bodies of tests/test_mesh_sparse_cpu.py against the
device through host.* and capi.*; the 129^3 sphere; runner.extract_mesh_sparse against runner.extract_mesh on the fox scene, bit for bit,
in one batch and in several; a grid above the dense path's cap against the dense mesher on point queries; extract_mesh_attrs(...,
sparse=); no effect on training; the launcher's mesh.sparse.  Indices past 32 bits: windows of virtual grids with corner indices above
2^36 and brick ids up to the last one below 2^31, f2n_brick_mark over 2^31 - 262144 bricks, extract_mesh_sparse at res 8192."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_ref as mr  # noqa: E402
import mesh_sparse_ref as sr  # noqa: E402
import test_mesh_sparse_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return cpu.same_bits(_np(a) if torch.is_tensor(a) else a, _np(b) if torch.is_tensor(b) else b)


@pytest.fixture(scope="module")
def impls(rt):
    from f2_nerf_amd import capi
    return cpu.host_impl(rt.host(), _dev, _np), cpu.host_impl(capi, _dev, _np)


def test_kernel_cases_on_the_device(impls):
    for impl in impls:
        flags = [cpu.check_brick_mark(impl, case, cut=False) for case in range(len(cpu.FOX_CASES))]
        cut = cpu.check_brick_mark(impl, 0, cut=True)
        assert (cut <= flags[0]).all() and (cut < flags[0]).any()
        for B in (4, 8):
            cpu.check_mesh_from_bricks(impl, B)
        cpu.check_errors(impl)


def _capi_locate():
    """cpu.check_huge_locate's `loc` over the ctypes binding (the host layer calls f2n_oct_locate_warp_bricks inside extract_mesh_sparse only)"""
    import types
    from f2_nerf_amd import capi

    def bricks(ids, lo, step, n, B, tree, transes):
        w, a = capi.locate_warp_bricks(_dev(np.asarray(ids, np.int32)), lo, step, n, B, _dev(tree), _dev(transes))
        return _np(w), _np(a)

    def points(pts, tree, transes):
        w = torch.full((len(pts), 3), 7.0, device="cuda")
        a = torch.full((len(pts), 3), 7, dtype=torch.int32, device="cuda")
        capi.oct_locate_warp(len(pts), _dev(np.asarray(pts, F32)), _dev(tree), _dev(transes), w, a)
        return _np(w), _np(a)

    return types.SimpleNamespace(bricks=bricks, points=points)


@pytest.mark.parametrize("name", sorted(sr.HUGE_GRIDS))
def test_listed_brick_kernels_on_a_huge_virtual_grid(impls, name):
    """corner indices past 2^36, vertex keys past 2^39, brick ids up to the last one below 2^31: windows of at most 64 bricks against the
    dense kernels on the window's sub-grid (tests/test_mesh_sparse_cpu.py)"""
    for impl in impls:
        cpu.check_huge_mesh_from_bricks(impl, name)
    cpu.check_huge_locate(_capi_locate(), name)


def test_two_to_the_31_bricks_are_refused(impls):
    import ctypes
    from f2_nerf_amd import capi
    for impl in impls:
        cpu.check_huge_errors(impl)
    (nx, ny, nz), B = sr.HUGE_REFUSED
    flags, tree = torch.full((8,), 7, dtype=torch.uint8, device="cuda"), _dev(cpu.fox_tree())
    rc = capi.lib().f2n_brick_mark(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.c_void_p(tree.data_ptr()),
                                   (ctypes.c_float * 3)(0.0, 0.0, 0.0), ctypes.c_float(1.0), ctypes.c_int(nx), ctypes.c_int(ny), ctypes.c_int(nz),
                                   ctypes.c_int(B), ctypes.c_void_p(flags.data_ptr()))
    torch.cuda.synchronize()
    assert rc == -2 and bool((flags == 7).all())  # F2N_ERR_UNSUPPORTED, nothing written


def test_brick_mark_on_the_full_grid(rt):
    """f2n_brick_mark over 131072 x 8191 x 2 = 2^31 - 262144 bricks (2 GiB of flags, 3.4 10^7 workgroups): step 1 and an integer lo put
    the fox tree's live leaves into a box of fewer than 4096 bricks next to the grid's far corner; inside that box the flags are the
    restatement's, brick by brick, and no brick outside it is flagged.  Compared on the device: only the box reaches the host."""
    from f2_nerf_amd import capi
    n, B, step = sr.HUGE_GRIDS["full"]["n"], sr.HUGE_GRIDS["full"]["B"], 1.0
    lo = (72.0 - step * (n[0] - 1), 72.0 - step * (n[1] - 1), -4.0)  # (integers below 2^24: every coordinate is exact)
    nb = sr.n_bricks(n, B)
    assert nb == (131072, 8191, 2) and nb[0] * nb[1] * nb[2] == 2 ** 31 - 262144
    tree = cpu.fox_tree()
    nodes = mr.parse_nodes(tree)
    live = (nodes["childs"] < 0).all(1) & (nodes["trans"] >= 0)
    half = nodes["side"][live].astype(np.float64)[:, None] / 2
    bl, bh = (nodes["center"][live] - half).min(0), (nodes["center"][live] + half).max(0)
    # the bricks that meet the closed bounding box of the live leaves, and one more on every side
    b0 = tuple(max(0, int(np.floor((bl[k] - lo[k]) / step / B)) - 1) for k in range(3))
    b1 = tuple(min(nb[k] - 1, int(np.floor((bh[k] - lo[k]) / step / B)) + 1) for k in range(3))
    assert np.prod([b1[k] - b0[k] + 1 for k in range(3)]) <= 4096 and sr.brick_id(b1, nb) > 2 ** 31 - 2 ** 20
    want = sr.brick_mark(nodes, lo, step, n, B, b0, b1)
    assert set(np.unique(want)) == {0, 1}
    torch.cuda.reset_peak_memory_stats()
    d_tree = _dev(tree)
    for mark in (rt.host().brick_mark, capi.brick_mark):
        flags = mark(d_tree, list(lo), step, list(n), B)
        assert flags.dtype == torch.uint8 and tuple(flags.shape) == nb[::-1]
        box = _np(flags[b0[2]:b1[2] + 1, b0[1]:b1[1] + 1, b0[0]:b1[0] + 1])
        assert (box == want).all()
        # nothing outside the box: the sum of all flags is the box's (every flag is 0 or 1; counted in slices of 2^27: a reduction over
        # the whole tensor works on a widened copy of the 2 GiB)
        flat = flags.view(-1)
        parts = [flat[a:a + (1 << 27)] for a in range(0, flat.numel(), 1 << 27)]
        assert max(int(p.max()) for p in parts) == 1 and sum(int(torch.count_nonzero(p)) for p in parts) == int(want.sum())
        del flat, parts
        del flags
    print("brick_mark on %d bricks: %d of the %d in the box flagged; peak device memory %.1f GB"
          % (nb[0] * nb[1] * nb[2], int(want.sum()), want.size, torch.cuda.max_memory_allocated() / 1e9))
    torch.cuda.empty_cache()


def test_sphere_129_on_bricks(rt):
    """the 129^3 sphere of tests/test_gpu_mesh_attrs.py (296 k faces), B = 8 and 16: host.mesh_from_grid's bits, a closed surface"""
    h = rt.host()
    grid = mr.sphere_grid(129, 0.4 * 128)
    dv, df = h.mesh_from_grid(_dev(grid), 0.0, [0.0, 0.0, 0.0], 1.0)
    assert len(df) > 290000
    for B in (8, 16):
        ids = sr.bricks_with_both_sides(grid, 0.0, B)
        assert 0 < len(ids) < (128 // B) ** 3
        v, f = h.mesh_from_bricks(_dev(sr.brick_values(grid, ids, B)), _dev(ids), [129, 129, 129], [0.0, 0.0, 0.0], 1.0, 0.0, B)
        assert _same(v, dv) and _same(f, df)
    fn = _np(f).astype(np.int64)
    edges = np.sort(np.concatenate([fn[:, [0, 1]], fn[:, [1, 2]], fn[:, [2, 0]]]), 1)
    n_edges = len(np.unique(edges[:, 0] * len(_np(v)) + edges[:, 1]))
    assert len(np.unique(fn)) - n_edges + len(fn) == 2  # Euler characteristic of a sphere


# ---- the fox runner ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fox_runner(rt, fox_state):
    runner, cfg, arrays = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    return runner


BOX = ([-1.0, -0.8, -0.9], [1.0, 0.7, 1.05])  # the box of tests/test_gpu_mesh_refine.py


@pytest.fixture(scope="module")
def fox_level(fox_runner):
    gn = fox_runner.density_grid(BOX[0], BOX[1], 64).cpu().numpy()
    return float(np.quantile(gn[gn > 0], 0.5))  # a level the scene crosses


STAT_KEYS = ["active_bricks", "batches", "bricks", "grid", "meshed_bricks", "points_evaluated", "points_nonempty"]


def _expected_points(flags, n, B):
    """the corners that exist in the rows of the flagged bricks"""
    return int(sum(sr.brick_corner_indices(int(b), n, B)[1].sum() for b in np.nonzero(flags.reshape(-1))[0]))


@pytest.mark.parametrize("res,B", [(40, 4), (97, 8), (97, 16)])
def test_extract_mesh_sparse_equals_extract_mesh_on_the_fox(rt, fox_runner, fox_state, fox_level, res, B):
    runner, h = fox_runner, rt.host()
    lo, hi = BOX
    dv, df = runner.extract_mesh(lo, hi, res, fox_level)
    assert len(df) > 1000
    m = runner.extract_mesh_sparse(lo, hi, res, fox_level, B)
    assert sorted(m) == ["faces", "stats", "verts"] and sorted(m["stats"]) == STAT_KEYS
    assert m["faces"].dtype == torch.int32 and _same(m["faces"], df) and _same(m["verts"], dv)
    st = m["stats"]
    step, nx, ny, nz = h.grid_spec(lo, hi, res)
    flags = _np(h.brick_mark(_dev(np.asarray(fox_state["tree_nodes"], np.uint8).reshape(-1)), lo, step, [nx, ny, nz], B))
    P = (B + 1) ** 3
    print("fox res %d B %d: %r; %d vertices, %d faces" % (res, B, st, len(dv), len(df)))
    assert st["grid"] == (nx, ny, nz) and st["bricks"] == flags.size and st["active_bricks"] == int(flags.sum())
    assert 0 < st["active_bricks"] < st["bricks"] and 0 < st["meshed_bricks"] <= st["active_bricks"] and st["batches"] == 1
    assert st["points_evaluated"] == _expected_points(flags, (nx, ny, nz), B) <= st["active_bricks"] * P
    assert 0 < st["points_nonempty"] <= st["points_evaluated"]
    again = runner.extract_mesh_sparse(lo, hi, res, fox_level, B)  # two calls: the same bits
    assert _same(again["verts"], m["verts"]) and _same(again["faces"], m["faces"]) and again["stats"] == st
    slab = runner.density_slab_points
    try:  # at least four batches
        runner.density_slab_points = max(P, st["active_bricks"] * P // 4)
        parts = runner.extract_mesh_sparse(lo, hi, res, fox_level, B)
    finally:
        runner.density_slab_points = slab
    assert parts["stats"]["batches"] >= 4 and {k: v for k, v in parts["stats"].items() if k != "batches"} == {k: v for k, v in st.items() if k != "batches"}
    assert _same(parts["verts"], dv) and _same(parts["faces"], df)
    assert runner.density_slab_points == slab


# res 8192 with a power-of-two step: 8193 x 8193 x 65 = 4 363 096 385 grid points, more than 2^32.  tests/mesh_sparse_ref.brick_mark flags
# 5379 of its 512 x 512 x 4 bricks of 16^3 cells on the fox tree (computed on the CPU over the bricks around the live leaves).
RES_8192_BOX = ([-512.0, -512.0, -4.0], [512.0, 512.0, 4.0])


def test_extract_mesh_sparse_at_res_8192(rt, fox_runner, fox_state, fox_level):
    """runner.extract_mesh_sparse on a grid of more than 2^32 points against runner.extract_mesh on the bounding window of the flagged
    bricks (the same step, lo translated by whole steps: exact), bit for bit; the stats carry the grid and the brick count unharmed"""
    from f2_nerf_amd import capi
    runner, h = fox_runner, rt.host()
    (lo, hi), res, B = RES_8192_BOX, 8192, 16
    step, nx, ny, nz = h.grid_spec(lo, hi, res, 8192)
    n = (nx, ny, nz)
    assert step == 0.125 and n == (8193, 8193, 65) and nx * ny * nz > 2 ** 32
    nb = sr.n_bricks(n, B)
    flags = _np(capi.brick_mark(_dev(np.asarray(fox_state["tree_nodes"], np.uint8).reshape(-1)), lo, step, n, B))
    assert 1 <= int(flags.sum()) <= 20000, int(flags.sum())
    at = np.argwhere(flags)  # (bz, by, bx)
    w0, w1 = at.min(0)[::-1], at.max(0)[::-1]
    i0 = [int(w0[k]) * B for k in range(3)]
    i1 = [min((int(w1[k]) + 1) * B, n[k] - 1) for k in range(3)]
    lo_w, hi_w = [lo[k] + step * i0[k] for k in range(3)], [lo[k] + step * i1[k] for k in range(3)]
    res_w = max(i1[k] - i0[k] for k in range(3))
    assert res_w <= 1024 and h.grid_spec(lo_w, hi_w, res_w)[0] == step and tuple(h.grid_spec(lo_w, hi_w, res_w)[1:]) == tuple(i1[k] - i0[k] + 1 for k in range(3))
    torch.cuda.reset_peak_memory_stats()
    m = runner.extract_mesh_sparse(lo, hi, res, fox_level, B)
    st = m["stats"]
    dv, df = runner.extract_mesh(lo_w, hi_w, res_w, fox_level)
    print("res 8192, B %d: %r; %d vertices, %d faces; window %r..%r; peak device memory %.1f GB"
          % (B, st, len(dv), len(df), i0, i1, torch.cuda.max_memory_allocated() / 1e9))
    assert len(df) > 1000 and m["faces"].dtype == torch.int32 and m["verts"].dtype == torch.float32
    # (tens of millions of vertices and faces: compared where they are)
    assert torch.equal(m["faces"], df) and torch.equal(m["verts"].view(torch.int32), dv.view(torch.int32))
    assert st["grid"] == n and st["bricks"] == nb[0] * nb[1] * nb[2] == 512 * 512 * 4 and st["active_bricks"] == int(flags.sum())
    assert 0 < st["meshed_bricks"] <= st["active_bricks"]
    assert st["points_evaluated"] == _expected_points(flags, n, B) and 0 < st["points_nonempty"] <= st["points_evaluated"]


def test_extract_mesh_sparse_refuses(fox_runner, fox_level):
    lo, hi = BOX
    for bad in (dict(level=-1.0), dict(level=float("nan")), dict(brick=5), dict(brick=0)):
        kw = dict(level=fox_level, brick=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            fox_runner.extract_mesh_sparse(lo, hi, 40, **kw)
    with pytest.raises((ValueError, RuntimeError)):
        fox_runner.extract_mesh_sparse(lo, hi, 8193, fox_level, 8)
    assert len(fox_runner.extract_mesh_sparse(lo, hi, 40, 0.0, 8)["faces"]) > 0  # level 0 is allowed: the boundary of the non-empty space


# The thin box holds live leaves of the fox tree: tests/mesh_sparse_ref.brick_mark flags 1300 of its 2304 bricks of 8^3 cells (computed
# on the CPU from tests/golden/fox_state.npz), so it was not shifted.
THIN_BOX = ([-1.0, -0.01, -0.01], [1.0, 0.01, 0.01])


def test_above_the_dense_cap(rt, fox_runner, fox_state):
    """res 2048 (2049 x 21 x 21 points): density_grid refuses it; the dense grid built from query_density at the grid's points and meshed by
    host.mesh_from_grid is extract_mesh_sparse's mesh, bit for bit"""
    runner, h = fox_runner, rt.host()
    lo, hi = THIN_BOX
    with pytest.raises((ValueError, RuntimeError)):
        runner.density_grid(lo, hi, 2048)
    with pytest.raises((ValueError, RuntimeError)):
        h.grid_spec(lo, hi, 2048)
    step, nx, ny, nz = h.grid_spec(lo, hi, 2048, 8192)
    assert (nx, ny, nz) == (2049, 21, 21) == sr.grid_spec(lo, hi, 2048)[1]
    ax = mr.grid_points(lo, step, (nx, ny, nz))
    pts = np.stack(np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")[::-1], -1).reshape(-1, 3)  # [nz, ny, nx] rows, (x, y, z) each
    grid = runner.query_density(_dev(pts)).view(nz, ny, nx)
    g = _np(grid)
    level = float(np.quantile(g[g > 0], 0.5))
    dv, df = h.mesh_from_grid(grid, level, lo, step)
    assert len(df) > 1000
    m = runner.extract_mesh_sparse(lo, hi, 2048, level, 8)
    st = m["stats"]
    print("thin box res 2048: %r; %d vertices, %d faces at level %.4g" % (st, len(dv), len(df), level))
    assert st["grid"] == (2049, 21, 21) and st["bricks"] == 2304 and st["active_bricks"] == 1300
    assert st["points_nonempty"] >= int((g > 0).sum()) > 0  # (every non-empty point is evaluated; rows share their border corners)
    assert _same(m["verts"], dv) and _same(m["faces"], df)


def _view_dirs(normals):
    flat = (normals == 0).all(1)
    return np.where(flat[:, None], np.array([0.0, 0.0, -1.0], np.float32), -normals).astype(np.float32)


def test_extract_mesh_attrs_sparse_on_the_fox(fox_runner, fox_level):
    runner = fox_runner
    lo, hi = BOX
    res, level = 64, fox_level
    dense = runner.extract_mesh_attrs(lo, hi, res, level, normal_source="field")
    m = runner.extract_mesh_attrs(lo, hi, res, level, normal_source="field", sparse=8)
    assert sorted(m) == sorted(list(dense) + ["sparse"]) and sorted(m["sparse"]) == STAT_KEYS
    assert len(m["faces"]) > 1000 and _same(m["verts"], dense["verts"]) and _same(m["faces"], dense["faces"])
    assert 0 < m["sparse"]["active_bricks"] < m["sparse"]["bricks"]
    fn = _np(runner.field_normals(m["verts"]))
    assert _same(m["normals"], fn) and (fn != 0).any()
    assert _same(m["colors"], runner.query_radiance(m["verts"], _dev(_view_dirs(fn)))[1])
    # where the field's normal does not vanish the dense call agrees; where it does the dense call falls back to the grid
    live = (fn != 0).any(1)
    assert cpu.same_bits(_np(dense["normals"])[live], fn[live])
    # the later stages see the same mesh: their outputs are the dense call's, bit for bit
    for kw in (dict(simplify=2), dict(refine={}), dict(min_component_faces=50, simplify=2, refine={})):
        a = runner.extract_mesh_attrs(lo, hi, res, level, normals=False, colors=False, **kw)
        b = runner.extract_mesh_attrs(lo, hi, res, level, normals=False, colors=False, sparse=8, **kw)
        assert sorted(b) == sorted(list(a) + ["sparse"]) and len(b["faces"]) > 0
        assert all(_same(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a), kw
    full = runner.extract_mesh_attrs(lo, hi, res, level, normal_source="field", simplify=2, refine={}, sparse=16)
    assert _same(full["normals"], runner.field_normals(full["verts"])) and full["colors"].shape == full["verts"].shape
    # no dense grid exists: its normals cannot be asked for
    for kw in (dict(), dict(normals=False), dict(colors=False), dict(normal_source="grid")):
        with pytest.raises(ValueError):
            runner.extract_mesh_attrs(lo, hi, res, level, sparse=8, **kw)
    assert len(runner.extract_mesh_attrs(lo, hi, res, level, normals=False, colors=False, sparse=8)["faces"]) == len(dense["faces"])
    with pytest.raises(ValueError):
        runner.extract_mesh_attrs(lo, hi, res, level, normal_source="field", sparse=5)
    with pytest.raises(ValueError):
        runner.extract_mesh_attrs(lo, hi, res, -1.0, normal_source="field", sparse=8)
    again = runner.extract_mesh_attrs(lo, hi, res, level, normal_source="field")  # the dense call is what it was
    assert sorted(again) == ["colors", "faces", "normals", "verts"] and all(_same(again[k], dense[k]) for k in dense)


def test_sparse_extraction_has_no_effect_on_training(rt, fox_state):
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 4096, rng)) for _ in range(6)]
    box = ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0])

    def run(extract):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=15"], seed=3, table_init=0.3)
        runner.n_edge_pts = 512
        losses = []
        for k, b in enumerate(batches):
            if extract and k == 3:
                g = runner.density_grid(box[0], box[1], 48).cpu().numpy()
                level = float(np.quantile(g[g > 0], 0.5))  # a level the scene crosses
                m = runner.extract_mesh_sparse(box[0], box[1], 48, level, 8)
                assert len(m["faces"]) > 0 and m["stats"]["active_bricks"] > 0
                a = runner.extract_mesh_attrs(box[0], box[1], 48, level, min_component_faces=20, normal_source="field", simplify=2, refine={}, sparse=4)
                assert len(a["faces"]) > 0 and a["colors"].shape == a["verts"].shape
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [t.detach().cpu().numpy().copy() for t in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))


def test_launcher_mesh_sparse(tmp_path, monkeypatch, capsys):
    """The synthetic rig of tests/test_gpu_mesh_refine.py's launcher test: mesh.sparse=8 writes the same bytes under the same name and
    prints the brick counts; with mesh.source=tsdf, or with grid normals, it raises before anything is extracted."""
    from PIL import Image
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh, rigs, run
    rng = np.random.default_rng(2)
    meta, hw = rigs.forward_facing(rng, n_side=(5, 4), hw=(48, 64), focal=56.0)
    meta[:, 12:14] *= 4.0; meta[:, 14] *= 4.0; meta[:, 16:18] *= 4.0
    data = tmp_path / "data" / "synth" / "rig"
    (data / "images_4").mkdir(parents=True)
    np.save(data / "cams_meta.npy", meta)
    for i in range(len(meta)):
        Image.fromarray(rng.integers(0, 255, (48, 64, 3), dtype=np.uint8)).save(data / "images_4" / ("%03d.png" % i))
    common = ["--config-name=llff", "dataset_name=synth", "case_name=rig", "exp_name=t", "+work_dir=%s" % tmp_path,
              "field.log2_table_size=14", "train.end_iter=60", "train.save_freq=30", "train.learning_rate_warm_up_end_iter=10",
              "pts_sampler.sub_div_milestones=[20]", "pts_sampler.compact_freq=25", "train.pts_batch_size=32768"]
    assert run.main(common + ["mode=train"]) == 0
    orig = mesh.extract
    extracted = []

    def spy(runner, cfg, scene, exp_dir, dataset=None):  # a density level the scene crosses
        o = mesh.options(cfg)
        if o["source"] == "density":
            g = runner.density_grid(o["bbox_min"], o["bbox_max"], o["resolution"]).cpu().numpy()
            cfg["mesh"]["level"] = float(np.quantile(g[g > 0], 0.5)) if (g > 0).any() else 1.0
        extracted.append(o["sparse"])
        return orig(runner, cfg, scene, exp_dir, dataset=dataset)

    monkeypatch.setattr(mesh, "extract", spy)
    meshes = tmp_path / "exp" / "rig" / "t" / "meshes"
    ex = common + ["mode=extract_mesh", "is_continue=true", "mesh.resolution=24"]
    capsys.readouterr()
    for extra, name in (([], "60_24"), (["mesh.normals=true", "mesh.colors=true", "mesh.simplify=2"], "60_24_s2")):
        assert run.main(ex + ["mesh.normal_source=field"] + extra) == 0
        dense_line = [ln for ln in capsys.readouterr().out.split("\n") if ln.startswith("Mesh:")]
        ply = open(meshes / (name + ".ply"), "rb").read()
        v0, f0 = mesh.read_ply(str(meshes / (name + ".ply")))
        assert len(f0) > 0
        os.remove(meshes / (name + ".ply"))
        for flag, B in ((("8", 8), ("true", 8)) if not extra else (("4", 4),)):
            assert run.main(ex + ["mesh.sparse=%s" % flag, "mesh.normal_source=field"] + extra) == 0
            line = [ln for ln in capsys.readouterr().out.split("\n") if ln.startswith("Mesh:")]
            assert len(line) == 1 and "bricks of %d^3 cells active" % B in line[0] and len(dense_line) == 1 and "bricks" not in dense_line[0]
            if not extra:
                assert open(meshes / (name + ".ply"), "rb").read() == ply  # the same name, the same bytes
            else:  # (a vertex whose field normal vanishes keeps its grid normal in the dense export only: compare the geometry)
                v1, f1 = mesh.read_ply(str(meshes / (name + ".ply")))
                assert cpu.same_bits(v1, v0) and cpu.same_bits(f1, f0) and len(open(meshes / (name + ".ply"), "rb").read()) == len(ply)
            os.remove(meshes / (name + ".ply"))
    assert extracted[-1] == 4 and extracted[0] == 0
    n_files = len(os.listdir(meshes))
    tsdf = ["mesh.source=tsdf", "tsdf.res_level=2", "tsdf.tau=0.0001", "tsdf.min_opacity=0.0001", "tsdf.min_weight=0.0001"]
    for bad in (["mesh.sparse=8"] + tsdf, ["mesh.sparse=8", "mesh.normals=true"], ["mesh.sparse=8", "mesh.colors=true", "mesh.normal_source=grid"],
                ["mesh.sparse=8", "mesh.texture=true"], ["mesh.sparse=5"]):
        with pytest.raises(ValueError):
            run.main(ex + bad)
    assert len(os.listdir(meshes)) == n_files  # nothing was written
