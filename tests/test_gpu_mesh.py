"""World-space density queries and mesh extraction on the MI355X (csrc/octree.hip, host/RendererQuery.cpp): point location against the
oracle's ray march and a numpy descent, densities against the oracle's field, grids against point queries, the marching-tetrahedra
kernels against their numpy restatement (tests/mesh_ref.py), no effect on training, and the launcher's mode=extract_mesh."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


def _dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).cuda()


def _locate(capi, tree, trans, pts):
    n = len(pts)
    w = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    a = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    capi.oct_locate_warp(n, torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda(), tree, trans, w, a)
    return w.cpu().numpy(), a.cpu().numpy()


def test_locate_agrees_with_the_ray_march():
    from f2_nerf_amd import capi
    from oracle import capi as oc
    d = dict(np.load(os.path.join(ROOT, "tools", "data", "converged_sampler.npz")))
    rng = np.random.default_rng(1)
    sel = rng.choice(len(d["rays_o"]), 1024, replace=False)
    ro = d["rays_o"][sel]
    rd = oc.normalize_dirs(d["rays_d"][sel])
    noise = ((rng.random(1024 + len(ro) + 10, dtype=np.float32) - np.float32(.5)) + np.float32(1.)) * np.float32(d["fineness"])
    hits = oc.oct_intersect(d["search_order"], ro, rd, 0.01, 1e8, d["tree_nodes"])
    s = oc.ray_march(ro, rd, noise.astype(np.float32), 1. / 256., True, *hits, d["tree_nodes"], d["pers_trans"])
    se = s["pts_idx_bounds"]
    ray = np.repeat(np.arange(len(ro)), se[:, 1] - se[:, 0])
    world = (ro[ray] + rd[ray] * s["t"][:, None]).astype(np.float32)
    assert len(world) > 10000
    w, a = _locate(capi, _dev_u8(d["tree_nodes"]), _dev_u8(d["pers_trans"]), world)
    same = (a[:, 0] == s["anchors"][:, 0]) & (a[:, 1] == s["anchors"][:, 1])
    nodes = mr.parse_nodes(d["tree_nodes"])
    leaf = s["anchors"][:, 1]
    dist = np.min(np.abs(np.abs(world - nodes["center"][leaf]) - nodes["side"][leaf][:, None] * .5), 1)
    near_face = dist <= 1e-5 * nodes["side"][leaf]
    assert (same | near_face).all(), np.count_nonzero(~same & ~near_face)
    assert np.count_nonzero(~same) < 1e-4 * len(world), np.count_nonzero(~same)
    assert (w[same].view(np.uint32) == s["pts"][same].view(np.uint32)).all()
    ref_w, _ = oc.warp(d["pers_trans"], a[same, 0], world[same])
    assert (w[same].view(np.uint32) == ref_w.view(np.uint32)).all()


def test_locate_agrees_with_a_numpy_descent(fox_state):
    from f2_nerf_amd import capi
    from oracle import capi as oc
    st = fox_state
    rng = np.random.default_rng(2)
    # the fox tree has every child slot of its interior nodes filled: cut a few (slot -> -1) so that points fall into missing slots
    tree = np.array(st["tree_nodes"], np.uint8).reshape(-1, 64)
    words = tree.view(np.int32)
    interior = np.nonzero((words[:, 5:13] >= 0).any(1))[0]
    for u in rng.choice(interior[interior > 0], 40, replace=False):
        words[u, 5 + rng.integers(0, 8)] = -1
    tree = tree.reshape(-1)
    nodes = mr.parse_nodes(tree)
    pts = rng.uniform(-1.2, 1.2, (4000, 3)).astype(np.float32)
    pts = np.concatenate([pts, rng.uniform(-600, 600, (200, 3)).astype(np.float32),  # outside the 512-wide root cube too
                          nodes["center"].astype(np.float32)])  # node centres: exact ties of the octant test
    w, a = _locate(capi, _dev_u8(tree), _dev_u8(st["pers_trans"]), pts)
    ref = np.array([mr.locate(nodes, p) for p in pts])
    assert (a[:, :2] == ref).all() and (a[:, 2] == 0).all()
    empty = ref[:, 0] < 0
    assert (w[empty] == 0).all()
    # the set holds every kind of empty point: outside the root, a missing child slot, a leaf with trans_idx < 0
    h = nodes["side"][0] * .5
    outside = (np.abs(pts - nodes["center"][0]) > h).any(1)
    assert outside.any()
    kinds = set()
    for p in pts[empty & ~outside][:2000]:
        u = 0
        while True:
            ch = nodes["childs"][u]
            if (ch < 0).all():
                kinds.add("dead_leaf")
                break
            c = nodes["center"][u]
            sl = 4 * int(p[0] >= c[0]) + 2 * int(p[1] >= c[1]) + int(p[2] >= c[2])
            if ch[sl] < 0:
                kinds.add("missing_child")
                break
            u = ch[sl]
    assert kinds == {"dead_leaf", "missing_child"}, kinds
    ref_w, _ = oc.warp(st["pers_trans"], a[~empty, 0], pts[~empty])
    assert (w[~empty].view(np.uint32) == ref_w.view(np.uint32)).all()


@pytest.fixture(scope="module")
def fox_runner(rt, fox_state):
    runner, cfg, arrays = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    return runner, arrays


def test_density_agrees_with_the_oracle(fox_runner, fox_state):
    from oracle import capi as oc, pipeline as op
    runner, arrays = fox_runner
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1.1, 1.1, (20000, 3)).astype(np.float32)
    dens = runner.query_density(torch.from_numpy(pts).cuda()).cpu().numpy()
    w, a = runner.locate_points(torch.from_numpy(pts).cuda())
    a = a.cpu().numpy()
    empty = a[:, 0] < 0
    assert 0 < empty.sum() < len(pts)
    assert (dens[empty] == 0).all()
    ref_w, _ = oc.warp(fox_state["pers_trans"], a[~empty, 0], pts[~empty])
    grid = op.HashGrid(arrays[4], arrays[5], arrays[6], int(arrays[7][0]), 14)
    f0 = op.field_fwd(grid, arrays[8], ref_w, a[~empty, 0])[:, 0]
    ref = np.exp(f0.astype(np.float64) - 3.0)
    err = np.abs(dens[~empty] - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() <= 1e-3, err.max()


def _grid_world(rt, lo, hi, res):
    step, nx, ny, nz = rt.host().grid_spec(lo, hi, res)
    ax = mr.grid_points(lo, np.float32(step), (nx, ny, nz))
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3), (nz, ny, nx)


@pytest.mark.parametrize("res,slab", [(97, None), (40, 5000)])
def test_density_grid_equals_point_queries(rt, fox_runner, res, slab):
    runner, _ = fox_runner
    lo, hi = [-1.0, -0.8, -0.9], [1.0, 0.7, 1.05]
    if slab is not None:
        runner.density_slab_points = slab  # several z-slabs
    try:
        g = runner.density_grid(lo, hi, res).cpu().numpy()
    finally:
        runner.density_slab_points = 1 << 22
    world, shape = _grid_world(rt, lo, hi, res)
    assert g.shape == shape and max(shape) == res + 1
    d = runner.query_density(torch.from_numpy(world).cuda()).cpu().numpy().reshape(shape)
    assert (g.view(np.uint32) == d.view(np.uint32)).all()
    assert (g == 0).any() and (g > 0).any()


def _gpu_mesh(rt, g, level=0.0, lo=(0.0, 0.0, 0.0), step=1.0):
    v, f = rt.host().mesh_from_grid(torch.from_numpy(np.ascontiguousarray(g, np.float32)).cuda(), level, list(lo), step)
    return v.cpu().numpy(), f.cpu().numpy()


def _euler_np(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    return len(np.unique(f)) - len(ue) + len(f), cnt


def test_mesh_matches_the_restatement(rt):
    from f2_nerf_amd import capi
    cases = [(mr.sphere_grid(18, 6.2), 0.0, (0.0, 0.0, 0.0), 1.0), (mr.torus_grid(20, 5.0, 2.2), 0.0, (-1.0, 0.5, 2.0), 0.25),
             (mr.sphere_grid(12, 7.0) * 3.0 + 1.0, 2.5, (0.0, 0.0, 0.0), 0.5)]
    rng = np.random.default_rng(4)
    cases.append((rng.standard_normal((9, 7, 11)).astype(np.float32), 0.1, (0.3, -0.2, 0.1), 0.125))  # arbitrary (non-cubic) grid
    for g, level, lo, step in cases:
        v, f = _gpu_mesh(rt, g, level, lo, step)
        rv, rf = mr.marching_tets(g, level, lo, step)
        assert f.shape == rf.shape and (f == rf).all()
        assert v.shape == rv.shape and np.abs(v - rv).max() <= 1e-6 * step * max(1.0, np.abs(rv).max())
        cv, cf = capi.mesh_from_grid(torch.from_numpy(np.ascontiguousarray(g)).cuda(), level, lo, step)
        assert (cf.cpu().numpy() == f).all() and (cv.cpu().numpy().view(np.uint32) == v.view(np.uint32)).all()


@pytest.mark.parametrize("n", [64, 129])
def test_mesh_sphere_closed_and_volume(rt, n):
    r = 0.4 * (n - 1)
    g = mr.sphere_grid(n, r)
    v, f = _gpu_mesh(rt, g)
    chi, cnt = _euler_np(f)
    assert chi == 2 and (cnt == 2).all()
    vol = mr.signed_volume(v, f)
    assert vol > 0 and abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1.0) < 0.01, vol
    v2, f2 = _gpu_mesh(rt, g)
    assert (f2 == f).all() and (v2.view(np.uint32) == v.view(np.uint32)).all()  # the same bits on two calls


def test_mesh_torus_empty_and_open(rt):
    v, f = _gpu_mesh(rt, mr.torus_grid(64, 18.0, 7.0))
    chi, cnt = _euler_np(f)
    assert chi == 0 and (cnt == 2).all()
    v, f = _gpu_mesh(rt, np.full((17, 9, 33), -1.0, np.float32))
    assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = _gpu_mesh(rt, mr.sphere_grid(40, 30.0))  # cut by the grid's faces
    _, cnt = _euler_np(f)
    assert len(f) > 0 and (cnt == 1).any() and cnt.max() == 2


def test_dense_mesher_at_its_cap(rt):
    """1025^3 = 1 076 890 625 grid points (mesh.resolution=1024 on a cubic box; about 31 GB of device memory): 2^30 lies in the plane
    z = 1022 of this grid, so the corners of the planes z >= 1022 are the ones whose offset 2 i into the [N,2] vertex scan needs more than
    31 bits.  The surface is a sphere of radius 9.3 cells near the far corner whose top lies between the planes z = 1022 and 1023: the
    edges its cap crosses are owned by corners of the plane z = 1022, past 2^30 (asserted below in Python integers), and every crossing
    edge keeps two cells away from the grid's faces along x and y and one along z.  step = 2^-6 and lo = -2^9 make every coordinate
    exact, so the 33^3 sub-grid at the far corner with lo translated by 992 steps has the same points bit for bit: the big grid's
    mesh must be the sub-grid's -- the restatement's (faces identical, vertices at test_mesh_matches_the_restatement's bar) and the
    dense kernels' own (bit for bit; vertex and face order is lexicographic in (z, y, x) on both sides) -- unmasked and masked."""
    h = rt.host()
    N, Wn, step = 1025, 33, 2.0 ** -6
    i0 = N - Wn
    lo, lo_w = [-512.0] * 3, [-512.0 + step * i0] * 3
    centre, radius = (1007.3, 1006.6, 1013.2), 9.3  # in cells
    big, sub = mr.grid_points(lo, step, (N,) * 3), mr.grid_points(lo_w, step, (Wn,) * 3)
    for k in range(3):  # lo + step (i0 + l) and lo_w + step l are the same floats, and exact
        assert big[k][i0:].tobytes() == sub[k].tobytes()
        assert (big[k].astype(np.float64) == lo[k] + step * np.arange(N)).all()
    torch.cuda.reset_peak_memory_stats()
    grid = torch.empty((N, N, N), dtype=torch.float32, device="cuda")
    ax = torch.arange(N, dtype=torch.float64, device="cuda")
    dxy = ((ax - centre[1]) ** 2)[:, None] + ((ax - centre[0]) ** 2)[None, :]
    for z0 in range(0, N, 64):  # the signed distance in world units, positive inside; float64 in slabs of 64 planes
        dz = ((ax[z0:z0 + 64] - centre[2]) ** 2)[:, None, None]
        grid[z0:z0 + 64] = (step * (radius - torch.sqrt(dz + dxy[None]))).to(torch.float32)
    del dxy, dz
    assert int((grid[:i0] > 0).sum()) == 0 and int((grid[:, :i0] > 0).sum()) == 0 and int((grid[:, :, :i0] > 0).sum()) == 0  # all in the window
    g_sub = grid[i0:, i0:, i0:].contiguous().cpu().numpy()
    ins = g_sub > 0
    at = np.argwhere(ins) + i0  # (z, y, x) of the inside corners: every crossing edge has one of them and a neighbour
    assert at.min() >= i0 + 2 and at[:, 1:].max() <= N - 4 and at[:, 0].max() == N - 3 == 1022
    past = 0  # crossing edges whose owner corner (the lower endpoint) has an index above 2^30
    for o in mr.EDGE_OFFSETS:
        d = (o & 1, (o >> 1) & 1, (o >> 2) & 1)
        a, b = ins[:Wn - d[2], :Wn - d[1], :Wn - d[0]], ins[d[2]:, d[1]:, d[0]:]
        for z, y, x in np.argwhere(a != b) + i0:
            past += ((int(z) * N + int(y)) * N + int(x)) > 2 ** 30
    assert past > 100 and N ** 3 - 1 > 2 ** 30 and (N - 1) ** 3 == 2 ** 30
    try:
        v, f = h.mesh_from_grid(grid, 0.0, lo, step)
        rv, rf = mr.marching_tets(g_sub, 0.0, lo_w, step)
        v, f = v.cpu().numpy(), f.cpu().numpy()
        assert len(rf) > 1000 and f.shape == rf.shape and (f == rf).all()
        assert v.shape == rv.shape and np.abs(v - rv).max() <= 1e-6 * step * max(1.0, np.abs(rv).max())
        d_sub = torch.from_numpy(g_sub).cuda()
        sv, sf = h.mesh_from_grid(d_sub, 0.0, lo_w, step)
        assert f.dtype == np.int32 and f.tobytes() == sf.cpu().numpy().tobytes() and v.tobytes() == sv.cpu().numpy().tobytes()
        # the masked mesher: valid on the far-corner window only (here every face lies in it: the unmasked mesh again)
        valid = torch.zeros((N, N, N), dtype=torch.uint8, device="cuda")
        valid[i0:, i0:, i0:] = 1
        mv, mf = h.mesh_from_grid_masked(grid, valid, lo, step, 0.0)
        smv, smf = h.mesh_from_grid_masked(d_sub, torch.ones((Wn,) * 3, dtype=torch.uint8, device="cuda"), lo_w, step, 0.0)
        mv, mf = mv.cpu().numpy(), mf.cpu().numpy()
        assert mf.tobytes() == smf.cpu().numpy().tobytes() and mv.tobytes() == smv.cpu().numpy().tobytes()
        assert mf.tobytes() == f.tobytes() and mv.tobytes() == v.tobytes()
        print("dense mesher at 1025^3: %d vertices, %d faces, %d crossing edges owned past 2^30; peak device memory %.1f GB"
              % (len(v), len(f), past, torch.cuda.max_memory_allocated() / 1e9))
    finally:
        grid = valid = d_sub = ax = None
        torch.cuda.empty_cache()


def test_extraction_has_no_effect_on_training(rt, fox_state):
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 4096, rng)) for _ in range(6)]

    def run(extract):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=15"], seed=3, table_init=0.3)
        runner.n_edge_pts = 512
        losses = []
        for k, b in enumerate(batches):
            if extract and k == 3:
                runner.extract_mesh([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 48, 1.0)
                runner.query_density(torch.rand((1000, 3), device="cuda") * 2 - 1)
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [t.detach().cpu().numpy().copy() for t in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))


def test_launcher_extract_mesh(tmp_path, monkeypatch):
    from PIL import Image
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh, rigs, run
    import test_mesh_cpu
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
    seen = {}
    orig = mesh.extract

    def spy(runner, cfg, scene, exp_dir):
        o = mesh.options(cfg)
        g = runner.density_grid(o["bbox_min"], o["bbox_max"], o["resolution"]).cpu().numpy()
        assert o["resolution"] == 40
        cfg["mesh"]["level"] = float(np.quantile(g[g > 0], 0.5)) if (g > 0).any() else 1.0  # a level the scene crosses
        path = orig(runner, cfg, scene, exp_dir)
        v, f = runner.extract_mesh(o["bbox_min"], o["bbox_max"], o["resolution"], cfg["mesh"]["level"])
        seen.update(path=path, v=mesh.to_world(v.cpu().numpy(), scene["center"], scene["radius"]), f=f.cpu().numpy(),
                    iter=runner.iter_step)
        return path

    monkeypatch.setattr(mesh, "extract", spy)
    assert run.main(common + ["mode=extract_mesh", "is_continue=true", "mesh.resolution=40"]) == 0
    assert seen["path"] == str(tmp_path / "exp" / "rig" / "t" / "meshes" / "60_40.ply") and seen["iter"] == 60
    v, f = test_mesh_cpu.read_ply(seen["path"])
    assert len(f) > 0 and (v.view(np.uint32) == seen["v"].view(np.uint32)).all() and (f == seen["f"]).all()
