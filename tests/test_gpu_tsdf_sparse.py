"""Sparse TSDF fusion on bricks on the MI355X (csrc/dataset.hip, csrc/octree.hip, host/RendererQuery.cpp): the bodies of
tests/test_tsdf_sparse_cpu.py against the device through host.* and capi.*; the C entry points' error codes; mesh.fuse_tsdf_sparse against
mesh.fuse_tsdf + host.mesh_from_grid_masked on the fox scene, bit for bit, in one batch and in several; no effect on training; the
launcher's tsdf.sparse.  Indices past 32 bits: windows of virtual grids with corner indices above 2^36 and brick ids up to the last one
below 2^31; f2n_tsdf_brick_mark over more bricks than it launches workgroups."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_sparse_ref as sr  # noqa: E402
import tsdf_ref as tr  # noqa: E402
import tsdf_sparse_ref as ts  # noqa: E402
import test_tsdf_sparse_cpu as cpu  # noqa: E402
from test_gpu_tsdf import _fox_options  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
_f, _i = ctypes.c_float, ctypes.c_int


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module", params=["host", "capi"])
def impl(rt, request):
    from f2_nerf_amd import capi
    return cpu.module_impl(rt.host() if request.param == "host" else capi, _dev, _np)


@pytest.mark.parametrize("name,B", [("synth_conf", 4), ("synth", 4), ("synth_conf", 8), ("synth", 8), ("sphere", 4), ("sphere", 8), ("sphere", 16)])
def test_flags_equal_the_restatement(impl, fox_state, name, B):
    cpu.check_mark(impl, fox_state, name, B)


def test_flags_of_one_view_and_of_none(impl, fox_state):
    cpu.check_mark_few_views(impl, fox_state)


@pytest.mark.parametrize("name,B", [("synth_conf", 4), ("synth", 8), ("sphere", 16)])
def test_brick_integration_equals_the_dense_kernel(impl, fox_state, name, B):
    cpu.check_integrate_bricks(impl, fox_state, name, B)


@pytest.mark.parametrize("B", [4, 8])
def test_masked_brick_mesher_equals_the_dense_masked_mesher(impl, B):
    cpu.check_masked_brick_mesher(impl, B)


@pytest.mark.parametrize("name,B", [("synth_conf", 4), ("synth_conf", 8), ("sphere", 4), ("sphere", 8)])
def test_flagged_bricks_give_the_dense_mesh(impl, fox_state, name, B):
    cpu.check_flagged_bricks_give_the_dense_mesh(impl, fox_state, name, B)


def test_value_errors(impl, fox_state):
    cpu.check_value_errors(impl, fox_state)


@pytest.mark.parametrize("name", sorted(sr.HUGE_GRIDS))
def test_listed_brick_kernels_on_a_huge_virtual_grid(impl, fox_state, name):
    """corner indices past 2^36, brick ids up to the last one below 2^31: the masked brick mesher and the brick integration over windows
    of at most 64 bricks against the dense kernels on the window's sub-grid (tests/test_tsdf_sparse_cpu.py)"""
    cpu.check_huge_masked_mesher(impl, name)
    cpu.check_huge_integrate_bricks(impl, fox_state, name)


def test_two_to_the_31_bricks_are_refused(impl, fox_state):
    from f2_nerf_amd import capi
    cpu.check_huge_value_errors(impl, fox_state)
    (nx, ny, nz), B = sr.HUGE_REFUSED
    w, c, big = cpu.huge_tsdf_case(fox_state, "full", "inner")
    d = dict(poses=_dev(c["poses"]), intri=_dev(c["intri"]), dist=_dev(c["dist"]), depth=_dev(c["depth"]), conf=_dev(c["conf"]),
             flags=torch.full((8,), 7, dtype=torch.uint8, device="cuda"), ids=_dev(w["ids"][:2]),
             S=torch.full((2, 125), 7.0, device="cuda"), W=torch.full((2, 125), 7.0, device="cuda"))
    assert _raw(capi.lib(), big, d, nx=nx, ny=ny, nz=nz, B=B) == (cpu.UNSUPPORTED, cpu.UNSUPPORTED)
    torch.cuda.synchronize()
    assert (d["flags"] == 7).all() and (d["S"] == 7).all() and (d["W"] == 7).all()  # nothing was written
    assert _raw(capi.lib(), big, d, "integrate", B=B) == 0 and (d["W"] != 7).any()  # the full grid, 2^31 - 262144 bricks, is accepted


def test_brick_mark_where_a_workgroup_takes_several_bricks(impl, fox_state):
    """n = (524288, 97, 9), B = 4: 131072 x 24 x 2 = 6 291 456 bricks, six for every workgroup of f2n_tsdf_brick_mark's 2^20.  Two views of
    tsdf_ref.synthetic_case see the last 8 bricks along x only: the case is built on the window's own grid (32 x 97 x 9 points, a
    power-of-two step, lo a multiple of it) and every depth that could put a hit at or below the window's second plane is removed
    (a hit needs |p - o| <= D + trunc, and |p - o| >= o_x - p_x).  Inside the window the flags are the restatement's; outside all zero."""
    n, B, wbx = (524288, 97, 9), 4, 8
    nb = sr.n_bricks(n, B)
    assert nb == (131072, 24, 2) and nb[0] * nb[1] * nb[2] == 6 * 2 ** 20
    i0 = (nb[0] - wbx) * B
    c = tr.synthetic_case(fox_state, dims=(n[0] - i0, n[1], n[2]), n_views=2, pow2=True)
    step, trunc = float(c["step"]), float(c["trunc"])
    lo = (float(c["lo"][0]) - step * i0, float(c["lo"][1]), float(c["lo"][2]))
    x_big = F32(lo[0]) + F32(step) * np.arange(i0, n[0]).astype(F32)
    x_sub = c["lo"][0] + c["step"] * np.arange(n[0] - i0, dtype=F32)
    assert F32(lo[0]) == lo[0] and x_big.tobytes() == x_sub.tobytes() and (x_big.astype(np.float64) == lo[0] + step * np.arange(i0, n[0])).all()
    depth = c["depth"].copy()
    for v in range(len(depth)):
        limit = (float(c["poses"][v, 0, 3]) - (float(c["lo"][0]) + step)) - trunc - 1e-3
        depth[v][np.isfinite(depth[v]) & (depth[v] > limit)] = 0.0
    c = dict(c, depth=depth)
    want = ts.brick_mark(c, B)
    assert want.shape == (nb[2], nb[1], wbx) and set(np.unique(want)) == {0, 1}
    flags = impl.mark(dict(c, nx=n[0], lo=np.array(lo, F32)), B)
    assert flags.dtype == np.uint8 and flags.shape == nb[::-1]
    assert (flags[:, :, -wbx:] == want).all() and int(flags[:, :, :-wbx].sum()) == 0
    print("tsdf_brick_mark on %d bricks: %d of the window's %d flagged" % (flags.size, int(want.sum()), want.size))


# ---- the C entry points themselves -------------------------------------------------------------------------------------------------
def _lo3(lo):
    return (_f * 3)(*(float(v) for v in lo))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw(L, c, d, which="both", **repl):
    """f2n_tsdf_brick_mark and / or f2n_tsdf_integrate_bricks over device tensors d with replaced arguments: the status code(s)"""
    a = dict(lo=_lo3(c["lo"]), step=c["step"], nx=c["nx"], ny=c["ny"], nz=c["nz"], B=4, V=len(c["depth"]), h=c["h"], w=c["w"], trunc=c["trunc"],
             n_bricks=int(d["ids"].numel()), **d)
    a.update(repl)
    views = [_i(a["V"]), _ptr(a["poses"]), _ptr(a["intri"]), _ptr(a["dist"]), _ptr(a["depth"]), _ptr(a["conf"]), _i(a["h"]), _i(a["w"]), _f(a["trunc"])]
    grid = [a["lo"], _f(a["step"]), _i(a["nx"]), _i(a["ny"]), _i(a["nz"]), _i(a["B"])]
    mark = lambda: L.f2n_tsdf_brick_mark(_stream(), *grid, *views, _ptr(a["flags"]))  # noqa: E731
    integ = lambda: L.f2n_tsdf_integrate_bricks(_stream(), *grid, _i(a["n_bricks"]), _ptr(a["ids"]), *views, _ptr(a["S"]), _ptr(a["W"]))  # noqa: E731
    return (mark(), integ()) if which == "both" else mark() if which == "mark" else integ()


def test_error_codes_and_foreign_rows(fox_state):
    from f2_nerf_amd import capi
    L = capi.lib()
    c = tr.synthetic_case(fox_state, dims=(9, 7, 5))
    nb = sr.n_bricks((9, 7, 5), 4)
    d = dict(poses=_dev(c["poses"]), intri=_dev(c["intri"]), dist=_dev(c["dist"]), depth=_dev(c["depth"]), conf=_dev(c["conf"]),
             flags=torch.full(nb[::-1], 7, dtype=torch.uint8, device="cuda"), ids=torch.arange(2, dtype=torch.int32, device="cuda"),
             S=torch.full((2, 125), 7.0, device="cuda"), W=torch.full((2, 125), 7.0, device="cuda"))
    bad = [dict(B=B) for B in (0, 5, 32, -4)] + [dict(trunc=t) for t in (0.0, -0.5, float("nan"), float("inf"))]
    bad += [{k: -1} for k in ("nx", "ny", "nz", "V", "h", "w")] + [dict(h=0), dict(w=0), dict(h=(1 << 24) + 1), dict(nx=1), dict(nz=(1 << 19) + 1)]
    bad += [{k: None} for k in ("lo", "poses", "intri", "dist", "depth")]
    for r in bad:
        assert _raw(L, c, d, **r) == (cpu.INVALID, cpu.INVALID), r
    assert _raw(L, c, d, V=0) == (0, 0) and _raw(L, c, d, V=0, poses=None, depth=None) == (0, 0)
    assert _raw(L, c, d, "mark", flags=None) == cpu.INVALID and _raw(L, c, d, "mark", nx=1 << 19, ny=1 << 19, nz=1 << 19) == cpu.UNSUPPORTED
    for r in (dict(S=None), dict(W=None), dict(ids=None), dict(n_bricks=-1)):
        assert _raw(L, c, d, "integrate", **r) == cpu.INVALID, r
    assert _raw(L, c, d, "integrate", n_bricks=0) == 0
    assert (d["flags"] == 7).all() and (d["S"] == 7).all() and (d["W"] == 7).all()  # nothing was written by any of the calls above
    assert _raw(L, c, d) == (0, 0) and set(np.unique(_np(d["flags"]))) <= {0, 1} and (d["W"] != 7).any()
    assert _raw(L, c, d, conf=None) == (0, 0)

    def raw(cc, S, W, ids, B):  # a brick id outside the grid keeps its whole row
        dd = dict(poses=_dev(cc["poses"]), intri=_dev(cc["intri"]), dist=_dev(cc["dist"]), depth=_dev(cc["depth"]), conf=_dev(cc["conf"]),
                  flags=None, ids=_dev(ids), S=_dev(S), W=_dev(W))
        rc = _raw(L, cc, dd, "integrate", B=B)
        S[...] = _np(dd["S"])
        W[...] = _np(dd["W"])
        return rc

    cpu.check_integrate_bricks_leaves_foreign_rows(raw, fox_state)
    # the masked brick mesher: valid == NULL, a brick size that does not exist
    vals, ok = torch.zeros((2, 125), device="cuda"), torch.ones((2, 125), dtype=torch.uint8, device="cuda")
    vc, fc = torch.full((2,), 7, dtype=torch.int32, device="cuda"), torch.full((2,), 7, dtype=torch.int32, device="cuda")
    count = lambda B=4, n=2, o=ok: L.f2n_brick_mesh_count_masked(  # noqa: E731
        _stream(), _i(9), _i(7), _i(5), _i(B), _i(n), _ptr(d["ids"]), _ptr(vals), _ptr(o), _f(0.0), _ptr(vc), _ptr(fc))
    assert count(B=5) == cpu.INVALID and count(n=-1) == cpu.INVALID and count(o=None) == cpu.INVALID and count(n=0) == 0 and (vc == 7).all()
    assert count() == 0 and (vc == 0).all() and (fc == 0).all()


# ---- the fox runner ----------------------------------------------------------------------------------------------------------------
STAT_KEYS = ["active_bricks", "batches", "bricks", "grid", "meshed_bricks", "points_evaluated", "points_known"]


@pytest.fixture(scope="module")
def fox(rt, fox_state):
    """the runner and data set of tests/test_gpu_tsdf.py::test_fuse_tsdf_on_the_fox; dense(views) = its options with max_views = views
    (4: the test's own; 0: every training camera) and the dense result, computed once"""
    from f2_nerf_amd import mesh
    runner, cfg, arrays = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    ds = rt.make_dataset(fox_state)
    done = {}

    def dense(views):
        if views not in done:
            o = _fox_options(fox_state, max_views=views)
            t = mesh.fuse_tsdf(runner, ds, fox_state, o)
            dv, df = rt.host().mesh_from_grid_masked(t["g"], t["valid"], t["lo"], t["step"], 0.0)
            done[views] = (o, t, _np(dv), _np(df))
        return done[views]

    return runner, ds, dense


# views = 4: the options of test_fuse_tsdf_on_the_fox as they are -- 245 grid points known and NO face on the untrained field, so what
# is compared there is the empty mesh and the statistics; views = 0 (all 43 cameras, everything else the same) gives a surface
@pytest.mark.parametrize("views,B", [(4, 4), (4, 8), (0, 4), (0, 8)])
def test_fuse_tsdf_sparse_on_the_fox(rt, fox, fox_state, views, B):
    from f2_nerf_amd import mesh
    runner, ds, dense = fox
    o, t, dv, df = dense(views)
    assert _fox_options(fox_state)["max_views"] == 4 and o["resolution"] == 31
    m = mesh.fuse_tsdf_sparse(runner, ds, fox_state, o, B)
    assert sorted(m) == ["faces", "lo", "n_views", "stats", "step", "trunc", "verts"] and sorted(m["stats"]) == STAT_KEYS
    st = m["stats"]
    print("fox res %d, %d views, B %d: %r; dense mesh %d vertices, %d faces, %d of %d grid points known" % (
        o["resolution"], t["n_views"], B, st, len(dv), len(df), int(t["valid"].sum()), t["valid"].numel()))
    assert views == 4 or len(df) > 1000  # (the dense path's own mesh: the comparison below is not between two empty meshes)
    assert m["faces"].dtype == torch.int32 and m["verts"].dtype == torch.float32
    assert tr.same_bits(_np(m["verts"]), dv) and tr.same_bits(_np(m["faces"]), df)
    assert (m["lo"], m["step"], m["n_views"], m["trunc"]) == (t["lo"], t["step"], t["n_views"], t["trunc"])
    n = tuple(int(v) for v in t["S"].shape[::-1])
    assert st["grid"] == n and st["bricks"] == int(np.prod(sr.n_bricks(n, B))) and 0 < st["active_bricks"] <= st["bricks"]
    assert (len(df) == 0 or st["meshed_bricks"] > 0) and st["meshed_bricks"] <= st["active_bricks"]
    assert st["batches"] == 1 and 0 < st["points_known"] <= st["points_evaluated"] <= st["active_bricks"] * (B + 1) ** 3
    slab = runner.density_slab_points
    try:  # at least three batches: the same bits
        runner.density_slab_points = max(1, st["active_bricks"] // 3) * (B + 1) ** 3
        m3 = mesh.fuse_tsdf_sparse(runner, ds, fox_state, o, B)
    finally:
        runner.density_slab_points = slab
    assert m3["stats"]["batches"] >= 3 and {k: v for k, v in m3["stats"].items() if k != "batches"} == {k: v for k, v in st.items() if k != "batches"}
    assert tr.same_bits(_np(m3["verts"]), dv) and tr.same_bits(_np(m3["faces"]), df)


def test_fuse_tsdf_sparse_has_no_effect_on_training(rt, fox_state):
    from f2_nerf_amd import mesh
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 4096, rng)) for _ in range(5)]
    ds = rt.make_dataset(st)

    def run(query):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=15"], seed=3, table_init=0.3)
        runner.n_edge_pts = 512
        losses = []
        for k, b in enumerate(batches):
            if query and k == 3:
                m = mesh.fuse_tsdf_sparse(runner, ds, st, _fox_options(st, max_views=2, views_per_batch=2), 8)
                assert m["stats"]["active_bricks"] > 0
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [x.detach().cpu().numpy().copy() for x in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))


def test_launcher_tsdf_sparse(tmp_path, capsys):
    """mode=extract_mesh mesh.source=tsdf tsdf.sparse=8 on the synthetic rig of tests/test_gpu_tsdf.py::test_launcher_extract_mesh_from_the_tsdf:
    the dense run's vertices and faces in the same file, the brick counts in the Mesh: line; what the option refuses writes nothing"""
    from PIL import Image
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import rigs, run
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
    opts = ["mode=extract_mesh", "is_continue=true", "mesh.source=tsdf", "mesh.resolution=24", "tsdf.res_level=2", "tsdf.tau=0.0001",
            "tsdf.min_opacity=0.0001", "tsdf.min_weight=0.0001", "tsdf.views_per_batch=7"]
    path = str(tmp_path / "exp" / "rig" / "t" / "meshes" / "60_24_tsdf.ply")
    capsys.readouterr()
    assert run.main(common + opts) == 0 and os.path.exists(path)
    dense_line = [ln for ln in capsys.readouterr().out.split("\n") if ln.startswith("Mesh:")]
    dense_bytes = open(path, "rb").read()
    dv, df = test_mesh_cpu.read_ply(path)
    assert len(dense_line) == 1 and "grid points known" in dense_line[0] and "bricks" not in dense_line[0] and len(df) > 0
    os.remove(path)
    for extra in (["tsdf.sparse=8", "mesh.normals=true"], ["tsdf.sparse=5"], ["tsdf.sparse=8", "mesh.sparse=8"]):
        with pytest.raises(ValueError):
            run.main(common + opts + extra)
        assert not os.path.exists(path)
    assert run.main(common + opts + ["tsdf.sparse=8"]) == 0 and os.path.exists(path)
    line = [ln for ln in capsys.readouterr().out.split("\n") if ln.startswith("Mesh:")]
    v, f = test_mesh_cpu.read_ply(path)
    print(dense_line[0] + "\n" + line[0])
    assert tr.same_bits(v, dv) and tr.same_bits(f, df) and open(path, "rb").read() == dense_bytes
    assert len(line) == 1 and "bricks of 8^3 cells active" in line[0] and "grid points known" not in line[0]
    head = "Mesh: %d vertices, %d faces from the TSDF of" % (len(dv), len(df))
    assert line[0].startswith(head) and dense_line[0].startswith(head) and line[0].endswith(path) and dense_line[0].endswith(path)
    # field normals and colours go through: the vertex element carries them
    os.remove(path)
    assert run.main(common + opts + ["tsdf.sparse=true", "mesh.normals=true", "mesh.colors=true", "mesh.normal_source=field"]) == 0
    with open(path, "rb") as fh:
        head = fh.read().split(b"end_header\n", 1)[0].decode("ascii")
    assert "property float nx" in head and "property uchar red" in head and "element vertex %d\n" % len(dv) in head
