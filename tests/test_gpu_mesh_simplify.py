"""Mesh simplification on the MI355X (csrc/octree.hip, host/RendererQuery.cpp): the bodies of tests/test_mesh_simplify_cpu.py against
the device through host.mesh_simplify (twice in a row) and capi.mesh_simplify, bit for bit with the numpy restatement
(tests/mesh_simplify_ref.py); the device's own 129^3 sphere; extract_mesh_attrs(..., simplify=k) on the fox scene; no effect on training;
the launcher's mesh.simplify."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_attr_ref as ar  # noqa: E402
import mesh_ref as mr  # noqa: E402
import mesh_simplify_ref as sr  # noqa: E402
import test_mesh_simplify_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _gpu_mesh(rt, g, level=0.0, lo=(0.0, 0.0, 0.0), step=1.0):
    v, f = rt.host().mesh_from_grid(_dev(g, np.float32), level, list(lo), step)
    return v.cpu().numpy(), f.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def _host_fn(rt):
    def fn(v, f, cell, lo, lam):
        out = rt.host().mesh_simplify(_dev(v, np.float32).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3), cell,
                                      None if lo is None else [float(x) for x in lo], lam)
        return tuple(x.cpu().numpy() for x in out)
    return fn


def _capi_fn():
    from f2_nerf_amd import capi

    def fn(v, f, cell, lo, lam):
        out = capi.mesh_simplify(_dev(v, np.float32).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3), cell, lo, lam)
        return tuple(x.cpu().numpy() for x in out)
    return fn


@pytest.fixture(scope="module")
def device_mesher(rt):
    return lambda g, level: _gpu_mesh(rt, g, level)  # (one object: test_mesh_simplify_cpu.case_mesh makes every input mesh once)


@pytest.mark.parametrize("name", ["sphere33_k2", "sphere33_k3", "sphere65_k4", "plane24_k3", "random_k2", "torus32_k2", "torus32_k3"])
def test_device_matches_the_restatement(rt, device_mesher, name):
    v, f, cell, lo = cpu.case_mesh(name, device_mesher)
    host, capi = _host_fn(rt), _capi_fn()
    ov, of, vert_map = cpu.check_case_bits(name, v, f, cell, lo, host, False)
    cpu.check_case_bits(name, v, f, cell, lo, host, False)  # twice in a row
    cpu.check_case_bits(name, v, f, cell, lo, capi, False)
    cpu.check_known_answers(name, v, f, cell, lo, ov, of, vert_map)


def test_octahedron_and_contract_cases_on_the_device(rt, device_mesher):
    ref = sr.simplify(*cpu.octahedron(), 0.5)
    for fn in (_host_fn(rt), _capi_fn()):
        out = cpu.check_octahedron(fn)
        assert all(sr.same_bits(a, b) for a, b in zip(out, ref))
        cpu.check_contract(fn, RuntimeError, device_mesher)


def test_the_record_guard_on_the_device(rt):
    v, f = cpu.strip((1 << 18) // 3 + 20)
    with pytest.raises(RuntimeError) as e:
        _host_fn(rt)(v, f, 1.0, (0.0, 0.0, 0.0), 1e-3)
    assert "status -2" in str(e.value)
    n_ok = (1 << 18) // 3
    ov, of, vm = _host_fn(rt)(v[:n_ok + 2], f[:n_ok], 1.0, (0.0, 0.0, 0.0), 1e-3)
    assert len(of) == 0 and (vm == -1).all()  # one cluster: every face collapses


def test_the_devices_own_sphere(rt):
    """The 129^3 sphere mesh of tests/test_gpu_mesh_attrs.py (296 k faces) at k = 4: closed, manifold, the restatement's bits."""
    v, f = _gpu_mesh(rt, mr.sphere_grid(129, 0.4 * 128))
    assert len(f) > 290000
    ov, of, vm = _host_fn(rt)(v, f, 4.0, (0.0, 0.0, 0.0), 1e-3)
    rv, rf, rmap = sr.simplify(v, f, 4.0, (0.0, 0.0, 0.0))
    assert sr.same_bits(ov, rv) and sr.same_bits(of, rf) and sr.same_bits(vm, rmap)
    print("sphere129 at k = 4: %d -> %d faces, %d -> %d vertices" % (len(f), len(of), len(v), len(ov)))
    cpu.check_closed_manifold(ov, of)
    sr.check_structure(v, f, 4.0, (0.0, 0.0, 0.0), ov, of, vm)


@pytest.fixture(scope="module")
def fox_runner(rt, fox_state):
    runner, cfg, arrays = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    return runner, arrays


BOX = ([-1.0, -0.8, -0.9], [1.0, 0.7, 1.05])  # the box of tests/test_gpu_mesh_attrs.py::test_extract_mesh_attrs_on_the_fox


def _view_dirs(normals):
    flat = (normals == 0).all(1)
    return np.where(flat[:, None], np.array([0.0, 0.0, -1.0], np.float32), -normals).astype(np.float32)


def test_extract_mesh_attrs_with_simplify_on_the_fox(rt, fox_runner):
    runner, _ = fox_runner
    h = rt.host()
    lo, hi = BOX
    res = 64
    g = runner.density_grid(lo, hi, res)
    gn = g.cpu().numpy()
    level = float(np.quantile(gn[gn > 0], 0.5))  # a level the scene crosses
    step = h.grid_spec(lo, hi, res)[0]
    cell = float(F32(2) * F32(step))
    today = runner.extract_mesh_attrs(lo, hi, res, level)
    for k in (0, 1):  # off: every output as it is today, bit for bit
        m = runner.extract_mesh_attrs(lo, hi, res, level, simplify=k)
        assert sorted(m) == sorted(today) == ["colors", "faces", "normals", "verts"]
        assert all(_same_bits(m[key].cpu().numpy(), today[key].cpu().numpy()) for key in today)
    v, f = runner.extract_mesh(lo, hi, res, level)
    m = runner.extract_mesh_attrs(lo, hi, res, level, simplify=2)
    assert sorted(m) == ["colors", "faces", "faces_in", "normals", "verts", "verts_in"] and (m["verts_in"], m["faces_in"]) == (len(v), len(f))
    sv, sf, smap = h.mesh_simplify(v, f, cell, lo)
    mv, mf, mn, mc = (m[key].cpu().numpy() for key in ("verts", "faces", "normals", "colors"))
    print("fox %d^3 at level %.3g, simplify=2: %d -> %d faces, %d -> %d vertices" % (res, level, len(f), len(mf), len(v), len(mv)))
    assert 0 < len(mf) < len(f) and _same_bits(mv, sv.cpu().numpy()) and (mf == sf.cpu().numpy()).all()
    rv, rf, rmap = sr.simplify(v.cpu().numpy(), f.cpu().numpy(), cell, lo)
    assert sr.same_bits(mv, rv) and sr.same_bits(mf, rf) and sr.same_bits(smap.cpu().numpy(), rmap)
    # the attributes are computed AT the new vertices by the existing calls
    assert _same_bits(mn, h.grid_normals(g, m["verts"], lo, step).cpu().numpy())
    assert _same_bits(mc, runner.query_radiance(m["verts"], torch.from_numpy(_view_dirs(mn)).cuda())[1].cpu().numpy())
    mfield = runner.extract_mesh_attrs(lo, hi, res, level, normal_source="field", simplify=2)
    fn = runner.field_normals(m["verts"]).cpu().numpy()
    want = np.where((fn == 0).all(1, keepdims=True), mn, fn)
    assert _same_bits(mfield["verts"].cpu().numpy(), mv) and _same_bits(mfield["normals"].cpu().numpy(), want) and (fn != 0).any()
    assert _same_bits(mfield["colors"].cpu().numpy(), runner.query_radiance(m["verts"], torch.from_numpy(_view_dirs(want)).cuda())[1].cpu().numpy())
    # with the floater filter: the simplification of the filtered mesh
    sizes = sorted(ar.component_face_counts(f.cpu().numpy(), len(v)).values())
    assert len(sizes) > 1
    thr = max(2, sizes[len(sizes) // 2] + 1)
    fm = runner.extract_mesh_attrs(lo, hi, res, level, min_component_faces=thr, normals=False, colors=False, simplify=2)
    kv, kf, _ = h.mesh_filter_components(v, f, thr)
    assert len(kf) < len(f) and fm["faces_in"] == len(kf)
    sv, sf, _ = h.mesh_simplify(kv, kf, cell, lo)
    assert _same_bits(fm["verts"].cpu().numpy(), sv.cpu().numpy()) and (fm["faces"].cpu().numpy() == sf.cpu().numpy()).all()


def test_simplification_has_no_effect_on_training(rt, fox_state):
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
                m = runner.extract_mesh_attrs([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 48, level, min_component_faces=20, simplify=2)
                assert 0 < len(m["faces"]) < m["faces_in"] and m["colors"].shape == m["verts"].shape
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [t.detach().cpu().numpy().copy() for t in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))


def test_launcher_writes_the_simplified_mesh(tmp_path, monkeypatch, capsys):
    """The synthetic rig of tests/test_gpu_mesh_attrs.py::test_launcher_writes_attributes: mesh.simplify=2 writes <iter>_<res>_s2.ply with
    the runner's simplified mesh; without the option the old name carries the old bytes; the TSDF source gets <iter>_<res>_tsdf_s2.ply."""
    from PIL import Image
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh, rigs, run
    import test_mesh_attrs_cpu as attrs_cpu
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

    def spy(runner, cfg, scene, exp_dir, dataset=None):
        o = mesh.options(cfg)
        if o["source"] == "tsdf":
            return orig(runner, cfg, scene, exp_dir, dataset=dataset)
        g = runner.density_grid(o["bbox_min"], o["bbox_max"], o["resolution"]).cpu().numpy()
        cfg["mesh"]["level"] = float(np.quantile(g[g > 0], 0.5)) if (g > 0).any() else 1.0  # a level the scene crosses
        path = orig(runner, cfg, scene, exp_dir)
        o = mesh.options(cfg)
        box = (o["bbox_min"], o["bbox_max"], o["resolution"], o["level"])
        v, f = runner.extract_mesh(*box)
        m = runner.extract_mesh_attrs(*box, 0, False, False, "grid", 2)
        seen.update(path=path, o=o, plain_v=mesh.to_world(v.cpu().numpy(), scene["center"], scene["radius"]), plain_f=f.cpu().numpy(),
                    v=mesh.to_world(m["verts"].cpu().numpy(), scene["center"], scene["radius"]), f=m["faces"].cpu().numpy())
        return path

    monkeypatch.setattr(mesh, "extract", spy)
    ex = common + ["mode=extract_mesh", "is_continue=true", "mesh.resolution=40"]
    meshes = tmp_path / "exp" / "rig" / "t" / "meshes"
    assert run.main(ex + ["mesh.simplify=2"]) == 0
    assert seen["path"] == str(meshes / "60_40_s2.ply") and seen["o"]["simplify"] == 2 and not (meshes / "60_40.ply").exists()
    v, f = test_mesh_cpu.read_ply(seen["path"])
    assert 0 < len(f) < len(seen["plain_f"]) and _same_bits(v, seen["v"]) and (f == seen["f"]).all()
    assert "simplified from %d faces" % len(seen["plain_f"]) in capsys.readouterr().out
    # without the option: the old name with the bytes the plain writer has always written; the simplified file stays
    assert run.main(ex) == 0
    assert seen["path"] == str(meshes / "60_40.ply") and seen["o"]["simplify"] == 0 and (meshes / "60_40_s2.ply").exists()
    assert open(seen["path"], "rb").read() == attrs_cpu._ply_of_the_plain_writer(seen["plain_v"], seen["plain_f"])
    assert "simplified" not in capsys.readouterr().out
    # the TSDF source runs the same order (a scene trained for 60 iterations is translucent: thresholds low enough for rays to qualify)
    tsdf = ["mode=extract_mesh", "is_continue=true", "mesh.source=tsdf", "mesh.resolution=24", "tsdf.res_level=2", "tsdf.tau=0.0001",
            "tsdf.min_opacity=0.0001", "tsdf.min_weight=0.0001", "tsdf.views_per_batch=7"]
    assert run.main(common + tsdf) == 0 and run.main(common + tsdf + ["mesh.simplify=2"]) == 0
    pv, pf = test_mesh_cpu.read_ply(str(meshes / "60_24_tsdf.ply"))
    sv, sf = test_mesh_cpu.read_ply(str(meshes / "60_24_tsdf_s2.ply"))
    print("TSDF mesh of the tiny scene: %d -> %d faces, %d -> %d vertices" % (len(pf), len(sf), len(pv), len(sv)))
    assert len(pf) > 0 and len(sf) < len(pf) and len(sv) < len(pv) and np.isfinite(sv).all()
    assert sf.min(initial=0) >= 0 and sf.max(initial=-1) < len(sv) and len(np.unique(sf)) == len(sv)
