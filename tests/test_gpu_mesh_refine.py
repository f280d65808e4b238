"""Mesh refinement on the MI355X (csrc/octree.hip, host/RendererQuery.cpp): the bodies of tests/test_mesh_refine_cpu.py against the device
through host.* (twice in a row) and capi.*, bit for bit with the numpy restatement (tests/mesh_refine_ref.py); the device's own 129^3
sphere; runner.project_to_level and extract_mesh_attrs(..., refine=) on the fox scene; no effect on training; the launcher's mesh.refine."""
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_ref as mr  # noqa: E402
import mesh_refine_ref as rr  # noqa: E402
import test_mesh_refine_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = float("inf")


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _same_bits(a, b):
    return rr.same_bits(np.asarray(a), np.asarray(b))


@pytest.fixture(scope="module")
def device_mesher(rt):
    def fn(g, level):
        v, f = rt.host().mesh_from_grid(_dev(g, np.float32), level, [0.0, 0.0, 0.0], 1.0)
        return v.cpu().numpy(), f.cpu().numpy()
    return fn  # (one object: test_mesh_refine_cpu.sphere makes the mesh once)


@pytest.fixture(scope="module")
def impls(rt):
    from f2_nerf_amd import capi
    return cpu.tensor_impl(rt.host(), lambda x: x.cuda()), cpu.tensor_impl(capi, lambda x: x.cuda())


def test_known_answers_on_the_device(impls, device_mesher):
    for impl in impls:
        cpu.check_small_meshes(impl)
        cpu.check_face_quality(impl)
        cpu.check_level_step(impl)
    cpu.check_sphere(impls[0], device_mesher)


def test_device_matches_the_restatement(impls, device_mesher):
    host, capi = impls
    cpu.check_bits(host, device_mesher, tag="device_")
    cpu.check_bits(host, device_mesher, tag="device_")  # twice in a row
    cpu.check_bits(capi, device_mesher, tag="device_")


def test_contract_cases_on_the_device(impls):
    for impl in impls:
        cpu.check_contract(impl, (ValueError, RuntimeError))


def test_the_devices_own_sphere(rt, device_mesher):
    """The 129^3 sphere mesh of tests/test_gpu_mesh_attrs.py (296 k faces): ring, 5 Taubin pairs and face quality are the restatement's
    bits; the wall time of each stage is printed (no bar)."""
    h = rt.host()
    v, f = device_mesher(mr.sphere_grid(129, 0.4 * 128), 0.0)
    assert len(f) > 290000
    dv, df = _dev(v, F32), _dev(f, np.int32)

    def timed(fn):
        """(result, the median wall time in ms of five calls between device synchronisations, after one call that is not timed)"""
        fn()
        ms = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return out, float(np.median(ms))

    ring, t_ring = timed(lambda: h.mesh_ring(df, len(v)))
    sm, t_smooth = timed(lambda: h.mesh_smooth(dv, df, 5))
    q, t_q = timed(lambda: h.mesh_face_quality(sm, df))
    print("sphere129: %d faces, %d vertices, wall time, median of 5: mesh_ring %.2f ms, mesh_smooth (5 pairs, its own ring included) %.2f ms, "
          "mesh_face_quality %.2f ms" % (len(f), len(v), t_ring, t_smooth, t_q))
    want = rr.ring(f, len(v))
    assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(ring[:3], want[:3])) and list(ring[3]) == [0, 0]
    ref = rr.smooth(v, f, 5)
    assert _same_bits(sm.cpu().numpy(), ref) and _same_bits(q.cpu().numpy(), rr.face_quality(ref, f))
    q0 = rr.face_quality(v, f)
    print("sphere129: face quality p05 %.4f -> %.4f, median %.4f -> %.4f" % (np.quantile(q0, 0.05), np.quantile(q.cpu().numpy(), 0.05),
                                                                          np.median(q0), np.median(q.cpu().numpy())))


# ---- the fox runner ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fox_runner(rt, fox_state):
    runner, cfg, arrays = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    return runner, arrays


BOX = ([-1.0, -0.8, -0.9], [1.0, 0.7, 1.05])  # the box of tests/test_gpu_mesh_attrs.py::test_extract_mesh_attrs_on_the_fox
RES = 64


@pytest.fixture(scope="module")
def fox_level(fox_runner):
    runner, _ = fox_runner
    gn = runner.density_grid(BOX[0], BOX[1], RES).cpu().numpy()
    return float(np.quantile(gn[gn > 0], 0.5))  # a level the scene crosses


def _h_of(runner, points, level):
    """ln(sigma) - ln(level) as the projection forms it: query_density, two fp32 torch logs on the device, one subtraction"""
    return (torch.log(runner.query_density(points)) - torch.log(torch.full((1,), level, dtype=torch.float32, device="cuda"))).cpu().numpy()


def _move_bar(max_move, pts):
    """max_move and one fp32 rounding: of the clamp's arithmetic (2^-22 max_move) and of the coordinates it is stored in"""
    return max_move * (1 + 2.0 ** -22) + 0.87 * float(np.spacing(F32(np.abs(pts).max())))


def test_project_to_level_on_the_fox(rt, fox_runner, fox_level):
    runner, _ = fox_runner
    lo, hi = BOX
    level = fox_level
    step = rt.host().grid_spec(lo, hi, RES)[0]
    v, f = runner.extract_mesh(lo, hi, RES, level)
    max_step, max_move = float(F32(0.5) * F32(step)), float(F32(step))
    p = runner.project_to_level(v, level, 8, max_step, max_move, 1e-3)
    assert sorted(p) == ["evals", "h_in", "h_out", "points", "status"]
    pts, h_in, h_out, status, evals = (p[k].cpu().numpy() for k in ("points", "h_in", "h_out", "status", "evals"))
    vn = v.cpu().numpy()
    empty = (status & rr.EMPTY) != 0
    live = ~empty
    print("fox %d^3 at level %.3g: %d vertices, %.2f %% EMPTY, %.2f %% CONVERGED, %.2f %% MOVE_CLAMPED; field evaluations per vertex %.2f"
          % (RES, level, len(vn), 100 * empty.mean(), 100 * ((status & rr.CONVERGED) != 0).mean(), 100 * ((status & rr.MOVE_CLAMPED) != 0).mean(),
             evals.mean()))
    assert empty.mean() <= 0.05
    # the residuals are the field's own at the input and at the output points: the same kernels on the same points
    assert _same_bits(h_in, _h_of(runner, v, level)) and _same_bits(h_out, _h_of(runner, p["points"], level))
    assert (np.abs(h_out[live]) <= np.abs(h_in[live])).all()
    moved = np.linalg.norm(pts.astype(np.float64) - vn.astype(np.float64), axis=1)
    assert (moved <= _move_bar(max_move, vn)).all()
    assert _same_bits(pts[empty], vn[empty]) and (evals[empty] == 1).all() and (evals[live] >= 1).all() and evals.max() <= 8
    a_in, a_out = np.abs(h_in[live]), np.abs(h_out[live])
    print("fox: |ln(sigma/level)| over the non-EMPTY vertices: median %.4g -> %.4g, p90 %.4g -> %.4g; moved median %.3f, p90 %.3f, max %.3f grid steps"
          % (np.median(a_in), np.median(a_out), np.quantile(a_in, 0.9), np.quantile(a_out, 0.9), np.median(moved[live]) / step,
             np.quantile(moved[live], 0.9) / step, moved.max() / step))
    assert np.median(a_out) < np.median(a_in)
    again = runner.project_to_level(v, level, 8, max_step, max_move, 1e-3)
    assert all(_same_bits(again[k].cpu().numpy(), p[k].cpu().numpy()) for k in p)
    # the arguments that are refused
    for bad in ((0.0, 8, 1.0, 1.0, 1e-3), (-1.0, 8, 1.0, 1.0, 1e-3), (INF, 8, 1.0, 1.0, 1e-3), (level, 0, 1.0, 1.0, 1e-3), (level, 8, 0.0, 1.0, 1e-3),
                (level, 8, 1.0, -1.0, 1e-3), (level, 8, 1.0, 1.0, -1e-3)):
        with pytest.raises((ValueError, RuntimeError)):
            runner.project_to_level(v, *bad)
    none = runner.project_to_level(torch.zeros((0, 3), device="cuda"), level)
    assert none["points"].shape == (0, 3) and none["status"].shape == (0,)


def _view_dirs(normals):
    flat = (normals == 0).all(1)
    return np.where(flat[:, None], np.array([0.0, 0.0, -1.0], np.float32), -normals).astype(np.float32)


def _lower(x, q):
    e = np.sort(np.asarray(x, np.float64).reshape(-1))
    return float(e[int(np.floor(q * (len(e) - 1)))])


def test_extract_mesh_attrs_with_refine_on_the_fox(rt, fox_runner, fox_level):
    runner, _ = fox_runner
    h = rt.host()
    lo, hi = BOX
    level = fox_level
    g = runner.density_grid(lo, hi, RES)
    step = h.grid_spec(lo, hi, RES)[0]
    today = runner.extract_mesh_attrs(lo, hi, RES, level)
    plain = runner.extract_mesh_attrs(lo, hi, RES, level, refine=None)  # off: every output as it is today, bit for bit
    assert sorted(plain) == sorted(today) == ["colors", "faces", "normals", "verts"]
    assert all(_same_bits(plain[k].cpu().numpy(), today[k].cpu().numpy()) for k in today)
    for k, opts in ((0, {}), (2, {"smooth_passes": 1, "iters": 5, "max_step_steps": 0.25, "max_move_steps": 0.75, "tol": 1e-2, "lam": 0.4, "mu": -0.42}),
                    (0, {"project": False}), (0, {"smooth_passes": 0})):
        o = {"smooth_passes": 2, "lam": 0.5, "mu": -0.53, "project": True, "iters": 8, "max_step_steps": 0.5, "max_move_steps": 1.0, "tol": 1e-3}
        o.update(opts)
        base = runner.extract_mesh_attrs(lo, hi, RES, level, simplify=k)
        m = runner.extract_mesh_attrs(lo, hi, RES, level, simplify=k, refine=opts)
        assert sorted(m) == sorted(list(base) + ["refine"])
        v0, f = base["verts"], base["faces"]
        assert (m["faces"].cpu().numpy() == f.cpu().numpy()).all() and not _same_bits(m["verts"].cpu().numpy(), v0.cpu().numpy())
        # the stage by its parts: the clamps in grid steps, times simplify
        unit = float(F32(k) * F32(step)) if k >= 2 else step
        max_step, max_move = float(F32(o["max_step_steps"]) * F32(unit)), float(F32(o["max_move_steps"]) * F32(unit))
        st = m["refine"]
        assert st["max_step"] == max_step and st["max_move"] == max_move and st["points"] == len(v0)
        v = h.mesh_smooth(v0, f, o["smooth_passes"], o["lam"], o["mu"], max_move) if o["smooth_passes"] > 0 else v0
        if o["project"]:
            pr = runner.project_to_level(v, level, o["iters"], max_step, max_move, o["tol"], origins=v0)
            v = pr["points"]
            status = pr["status"].cpu().numpy()
            live = (status & rr.EMPTY) == 0
            assert st["empty"] == int((~live).sum()) and st["converged"] == int(((status & rr.CONVERGED) != 0).sum())
            assert st["step_clamped"] == int(((status & rr.STEP_CLAMPED) != 0).sum()) and st["move_clamped"] == int(((status & rr.MOVE_CLAMPED) != 0).sum())
            assert st["evals"] == int(pr["evals"].sum())
            a_in, a_out = np.abs(pr["h_in"].cpu().numpy()[live]), np.abs(pr["h_out"].cpu().numpy()[live])
            assert (st["h_median_before"], st["h_p90_before"]) == (_lower(a_in, 0.5), _lower(a_in, 0.9))
            assert (st["h_median_after"], st["h_p90_after"]) == (_lower(a_out, 0.5), _lower(a_out, 0.9))
        else:
            assert "h_median_before" not in st and "empty" not in st and st["project"] == 0
        mv, mn, mc = (m[key].cpu().numpy() for key in ("verts", "normals", "colors"))
        assert _same_bits(mv, v.cpu().numpy())
        moved = np.linalg.norm(mv.astype(np.float64) - v0.cpu().numpy().astype(np.float64), axis=1)
        assert (moved <= _move_bar(max_move, mv)).all() and moved.max() > 0
        assert abs(st["moved_max"] - moved.max() / step) <= 1e-9 * max(1.0, moved.max() / step) and st["moved_median"] <= st["moved_p90"] <= st["moved_max"]
        q0, q1 = h.mesh_face_quality(v0, f).cpu().numpy(), h.mesh_face_quality(m["verts"], f).cpu().numpy()
        assert (st["quality_median_before"], st["quality_p05_before"]) == (_lower(q0, 0.5), _lower(q0, 0.05))
        assert (st["quality_median_after"], st["quality_p05_after"]) == (_lower(q1, 0.5), _lower(q1, 0.05))
        fn = f.cpu().numpy()
        nb, na = rr.face_normals(v0.cpu().numpy(), fn), rr.face_normals(mv, fn)
        edges = h.mesh_ring(f, len(v0))[3]
        dots = (nb * na).sum(1)
        unsure = int((np.abs(dots) <= 1e-12 * np.linalg.norm(nb, axis=1) * np.linalg.norm(na, axis=1)).sum())  # (a sign that rounding decides)
        assert abs(st["flipped_faces"] - int((dots < 0).sum())) <= unsure and [st["boundary_edges"], st["nonmanifold_edges"]] == list(edges)
        print("fox simplify=%d refine=%r: %s" % (k, opts, json.dumps(st, sort_keys=True)))
        # the attributes are computed AT the refined vertices by the existing calls
        assert _same_bits(mn, h.grid_normals(g, m["verts"], lo, step).cpu().numpy())
        assert _same_bits(mc, runner.query_radiance(m["verts"], torch.from_numpy(_view_dirs(mn)).cuda())[1].cpu().numpy())
        if k == 0 and not opts:
            mfield = runner.extract_mesh_attrs(lo, hi, RES, level, normal_source="field", refine={})
            fnrm = runner.field_normals(m["verts"]).cpu().numpy()
            want = np.where((fnrm == 0).all(1, keepdims=True), mn, fnrm)
            assert _same_bits(mfield["verts"].cpu().numpy(), mv) and _same_bits(mfield["normals"].cpu().numpy(), want) and (fnrm != 0).any()
            assert _same_bits(mfield["colors"].cpu().numpy(),
                              runner.query_radiance(m["verts"], torch.from_numpy(_view_dirs(want)).cuda())[1].cpu().numpy())
    with pytest.raises((ValueError, RuntimeError)):
        runner.extract_mesh_attrs(lo, hi, RES, level, refine={"no_such_option": 1})
    for bad in ({"smooth_passes": -1}, {"iters": 0}, {"max_move_steps": 0.0}, {"max_step_steps": -1.0}, {"lam": float("nan")}, {"tol": -1.0}):
        with pytest.raises((ValueError, RuntimeError)):
            runner.extract_mesh_attrs(lo, hi, RES, level, refine=bad)
    again = runner.extract_mesh_attrs(lo, hi, RES, level)
    assert all(_same_bits(again[k].cpu().numpy(), today[k].cpu().numpy()) for k in today)


def test_refinement_has_no_effect_on_training(rt, fox_state):
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 4096, rng)) for _ in range(6)]

    def run(extract):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=15"], seed=3, table_init=0.3)
        runner.n_edge_pts = 512
        losses = []
        for k, b in enumerate(batches):
            if extract and k == 3:
                g = runner.density_grid([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 48).cpu().numpy()
                level = float(np.quantile(g[g > 0], 0.5))  # a level the scene crosses
                m = runner.extract_mesh_attrs([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 48, level, min_component_faces=20, simplify=2, refine={})
                assert len(m["faces"]) > 0 and m["colors"].shape == m["verts"].shape and m["refine"]["points"] == len(m["verts"])
                p = runner.project_to_level(m["verts"], level, 3, 0.01, 0.02)
                assert p["points"].shape == m["verts"].shape
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [t.detach().cpu().numpy().copy() for t in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))


def test_launcher_writes_the_refined_mesh(tmp_path, monkeypatch, capsys):
    """The synthetic rig of tests/test_gpu_mesh_simplify.py's launcher test: mesh.refine=true writes <name>_r.ply and <name>_r_refine.json and
    prints its line, the unrefined .ply keeps its bytes; the TSDF source smooths only; mesh.check then measures the refined mesh."""
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
    orig = mesh.extract

    def spy(runner, cfg, scene, exp_dir, dataset=None):  # a density level the scene crosses
        o = mesh.options(cfg)
        if o["source"] == "density":
            g = runner.density_grid(o["bbox_min"], o["bbox_max"], o["resolution"]).cpu().numpy()
            cfg["mesh"]["level"] = float(np.quantile(g[g > 0], 0.5)) if (g > 0).any() else 1.0
        return orig(runner, cfg, scene, exp_dir, dataset=dataset)

    monkeypatch.setattr(mesh, "extract", spy)
    meshes = tmp_path / "exp" / "rig" / "t" / "meshes"
    ex = common + ["mode=extract_mesh", "is_continue=true", "mesh.resolution=24"]
    chk = ["mesh.check=true", "check.res_level=2", "check.tau=0.0001", "check.min_opacity=0.0001", "check.max_views=5"]
    tsdf = ["mesh.source=tsdf", "tsdf.res_level=2", "tsdf.tau=0.0001", "tsdf.min_opacity=0.0001", "tsdf.min_weight=0.0001"]
    keys = {"smooth_passes", "project", "max_step", "max_move", "points", "empty", "converged", "step_clamped", "move_clamped", "evals",
            "h_median_before", "h_p90_before", "h_median_after", "h_p90_after", "moved_median", "moved_p90", "moved_max", "quality_median_before",
            "quality_p05_before", "quality_median_after", "quality_p05_after", "flipped_faces", "boundary_edges", "nonmanifold_edges"}
    projected = {"max_step", "empty", "converged", "step_clamped", "move_clamped", "evals", "h_median_before", "h_p90_before", "h_median_after",
                 "h_p90_after"}
    capsys.readouterr()
    for extra, name in (([], "60_24"), (["mesh.simplify=2"], "60_24_s2"), (tsdf, "60_24_tsdf")):
        assert run.main(ex + extra + chk) == 0
        plain_out = capsys.readouterr().out
        ply = open(meshes / (name + ".ply"), "rb").read()
        plain_check = json.load(open(meshes / (name + "_check.json")))
        assert not (meshes / (name + "_r.ply")).exists() and "Refine:" not in plain_out
        assert run.main(ex + extra + chk + ["mesh.refine=true"]) == 0
        out = capsys.readouterr().out
        assert open(meshes / (name + ".ply"), "rb").read() == ply  # the unrefined file: the same bytes
        pv, pf = test_mesh_cpu.read_ply(str(meshes / (name + ".ply")))
        rv, rf = test_mesh_cpu.read_ply(str(meshes / (name + "_r.ply")))
        st = json.load(open(meshes / (name + "_r_refine.json")))
        assert (rf == pf).all() and rv.shape == pv.shape and not _same_bits(rv, pv) and np.isfinite(rv).all()
        assert set(st) == (keys if "tsdf" not in name else keys - projected) and st["points"] == len(pv)
        line = [ln for ln in out.split("\n") if ln.startswith("Refine:")]
        assert len(line) == 1 and name + "_r.ply" in line[0] and name + "_r_refine.json" in line[0]
        assert [ln for ln in out.split("\n") if ln.startswith("Mesh:")] == [ln for ln in plain_out.split("\n") if ln.startswith("Mesh:")]
        # the check belongs to the refined mesh: its JSON carries the refined file's name, the unrefined one's stays as it was
        refined_check = json.load(open(meshes / (name + "_r_check.json")))
        assert json.load(open(meshes / (name + "_check.json"))) == plain_check and refined_check["n_faces"] == len(rf)
        assert name + "_r_check.json" in [ln for ln in out.split("\n") if ln.startswith("Check:")][0]
        with capsys.disabled():
            print(name, line[0])
            print("%s check: within_1 %.4f -> %.4f, median %.4f -> %.4f grid steps (unrefined -> refined; n_both %d -> %d)" % (
                name, plain_check["within_1"], refined_check["within_1"], plain_check["median"], refined_check["median"], plain_check["n_both"],
                refined_check["n_both"]))
    with pytest.raises(ValueError):
        run.main(ex + tsdf + ["mesh.refine=true", "refine.project=true"])
    with pytest.raises(ValueError):
        run.main(ex + ["mesh.refine=true", "refine.iters=0"])
