"""Mesh ray casting on the MI355X (csrc/octree.hip, host/RendererQuery.cpp): the bodies of tests/test_mesh_raycast_cpu.py against the device
through host.mesh_raycast (twice in a row) and capi.mesh_raycast, bit for bit with the numpy restatement (tests/mesh_raycast_ref.py);
the accelerated traversal against the device's own brute-force mode on the 129^3 sphere; mesh.render_mesh; the loop TSDF -> mesh -> ray
cast; mesh.check_mesh on the fox scene, its lack of effect on training and the launcher's mesh.check."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_raycast_ref as rr  # noqa: E402
import mesh_ref as mr  # noqa: E402
import test_mesh_raycast_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


def _dev(a, dt=F32):
    return torch.from_numpy(np.array(a, dtype=dt, order="C")).cuda()  # (a copy: the shared meshes and references are read-only)


def _np(out):
    return tuple(x.cpu().numpy() for x in out)


def _caster(build_fn, cast_fn):
    def build(v, f, cell=None, lo=None):
        return build_fn(_dev(v).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3), cell, None if lo is None else [float(x) for x in lo])

    def cast(v, f, accel, o, d, bounds=None):
        return _np(cast_fn(_dev(v).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3), accel, _dev(o).reshape(-1, 3), _dev(d).reshape(-1, 3),
                           None if bounds is None else _dev(bounds).reshape(-1, 2)))
    return cpu.Caster(build, cast, RuntimeError)


@pytest.fixture(scope="module")
def casters(rt):
    from f2_nerf_amd import capi
    h = rt.host()
    return _caster(h.mesh_raycast_build, h.mesh_raycast), _caster(capi.mesh_raycast_build, capi.mesh_raycast)


@pytest.fixture(scope="module")
def mesher(rt):
    def fn(g, level, lo=(0.0, 0.0, 0.0), step=1.0):
        v, f = rt.host().mesh_from_grid(_dev(g), level, [float(x) for x in lo], float(step))
        return v.cpu().numpy(), f.cpu().numpy()
    return fn  # (one object: get_mesh makes every input mesh once)


def test_watertight_from_inside(casters, mesher):
    """every third of the 8 930 rays against the restatement (2 977 rays x 4 464 faces), all of them for the misses: none"""
    host, capi = casters
    cpu.check_watertight(host, mesher, every=3, brute_rays=512)
    cpu.check_watertight(host, mesher, every=3)  # twice in a row
    cpu.check_watertight(capi, mesher, every=3)


@pytest.mark.parametrize("name", ["sphere17", "torus32"])
def test_lattice_rays(casters, mesher, name):
    host, capi = casters
    cpu.check_lattice(host, mesher, name, brute_rays=256)
    cpu.check_lattice(host, mesher, name)
    cpu.check_lattice(capi, mesher, name)


def test_known_answer(casters, mesher):
    """max |t - analytic| = 0.072 grid steps at 17^3 (400 rays); the bar is 0.2"""
    for rc in casters:
        cpu.check_known_answer(rc, mesher)


def test_the_acceleration_grid_does_not_change_a_bit(casters, mesher):
    host, capi = casters
    brute = cpu.check_grid_independence(host, mesher, "sphere17", side=40)
    v, f = cpu.get_mesh("sphere17", mesher)
    assert cpu.same(brute, cpu.reference(None, v, f, *cpu.camera_rays(17, 40)))
    cpu.check_grid_independence(capi, mesher, "sphere17", side=40)
    cpu.check_grid_independence(host, mesher, "sphere17", side=40, lo=cpu.FOX_LO, step=cpu.FOX_STEP)
    for rc in casters:
        cpu.check_cell_cap(rc, mesher)


def test_origins_windows_scaling_and_order(casters, mesher):
    for rc in casters:
        cpu.check_origins(rc, mesher)
        cpu.check_windows(rc, mesher)
        cpu.check_scaling_and_frame(rc, mesher)
        cpu.check_order_independence(rc, mesher)


def test_contract_cases(casters):
    for rc in casters:
        cpu.check_contract(rc)


def test_a_non_manifold_mesh(casters, mesher):
    host, capi = casters
    ref = cpu.check_non_manifold(host, mesher)
    cpu.check_non_manifold(host, mesher)
    cpu.check_non_manifold(capi, mesher)
    v, f = cpu.get_mesh("noise", mesher)
    rng = np.random.default_rng(13)
    o = rng.uniform(-3, 24, (1024, 3)).astype(F32)
    d = (rng.uniform(0, 20, (1024, 3)) - o).astype(F32)
    assert cpu.same(host.cast(v, f, None, o, d), ref)  # the device's brute-force mode over all 34 820 faces


def test_accelerated_against_brute_force_on_the_devices_own_sphere(casters, mesher):
    """The 129^3 sphere (296 k faces) with 16 384 camera-like rays: the traversal equals the brute-force mode bit for bit."""
    host, _ = casters
    v, f = cpu.get_mesh("sphere129", mesher)
    assert len(f) > 290000
    o, d = cpu.camera_rays(129, 128)
    brute = host.cast(v, f, None, o, d)
    accel = host.build(v, f)
    out = host.cast(v, f, accel, o, d)
    print("sphere129: %d faces, dims %s, cell %.3f, %d list entries; %d of %d rays hit" % (len(f), accel[2], accel[1], accel[4].numel(),
                                                                                          (out[1] >= 0).sum(), len(o)))
    assert cpu.same(out, brute) and (out[1] >= 0).sum() > 4000 and (out[1] < 0).sum() > 2000
    assert cpu.same(host.cast(v, f, host.build(v, f, 1.0, (0.0, 0.0, 0.0)), o, d), brute)
    r, c = 0.4 * 128, 64.0
    p = o[out[1] >= 0].astype(np.float64) + out[0][out[1] >= 0, None].astype(np.float64) * d[out[1] >= 0]
    assert np.abs(np.linalg.norm(p - c, axis=1) - r).max() < 0.2


def test_render_mesh(rt, mesher):
    """points, face_normals, facing and the attribute blends recomputed in numpy from (t, face, bary)"""
    from f2_nerf_amd import mesh
    v, f = cpu.get_mesh("sphere17", mesher)
    o, d = cpu.camera_rays(17, 40)
    o2, d2, _ = cpu.outside_rays(17, 64, seed=5)
    o, d = np.concatenate([o, o2, np.full((32, 3), 8.0, F32)]), np.concatenate([d, d2 * F32(3), d2[:32]])  # the last from inside: facing false
    rng = np.random.default_rng(3)
    vn = (v - 8.0) / np.linalg.norm(v - 8.0, axis=1, keepdims=True)
    vc = rng.uniform(0, 1, v.shape).astype(F32)
    b = np.stack([np.zeros(len(o), F32), np.full(len(o), 1e9, F32)], 1)
    out = mesh.render_mesh(_dev(v), _dev(f, np.int32), _dev(o), _dev(d), _dev(b), normals=_dev(vn), colors=_dev(vc))
    assert set(out) == {"hit", "t", "face", "bary", "points", "face_normals", "facing", "normals", "colors"}
    t, face, bary = (out[k].cpu().numpy() for k in ("t", "face", "bary"))
    assert cpu.same((t, face, bary), rr.raycast(v, f, o, d, b))
    ref = rr.render(v, f, o, d, t, face, bary, vn, vc)
    hit = out["hit"].cpu().numpy()
    assert (hit == ref["hit"]).all() and 400 < hit.sum() < len(o) and (out["facing"].cpu().numpy() == ref["facing"]).all()
    assert ref["facing"][:-32].sum() == hit[:-32].sum() and not ref["facing"][-32:].any() and hit[-32:].all()
    for k in ("points", "face_normals", "normals", "colors"):
        assert np.abs(out[k].cpu().numpy() - ref[k]).max() < 2e-5 * (20.0 if k == "points" else 1.0), k
        assert (out[k].cpu().numpy()[~hit] == 0).all()
    assert np.abs(np.linalg.norm(out["normals"].cpu().numpy()[hit], axis=1) - 1).max() < 1e-5
    # the geometric normal of an outward-wound sphere points away from the centre
    assert ((out["face_normals"].cpu().numpy()[hit] * (out["points"].cpu().numpy()[hit] - 8.0)).sum(1) > 0).all()
    plain = mesh.render_mesh(_dev(v), _dev(f, np.int32), _dev(o), _dev(d))
    assert set(plain) == {"hit", "t", "face", "bary", "points", "face_normals", "facing"} and (plain["face"].cpu().numpy() == face).all()
    none = mesh.render_mesh(_dev(v), _dev(np.zeros((0, 3)), np.int32), _dev(o), _dev(d), normals=_dev(vn))
    assert not none["hit"].any() and (none["points"] == 0).all() and (none["normals"] == 0).all()


def test_loop_closure(rt, casters, fox_state):
    """max |t_mesh - depth| = 0.39 grid steps (median 0.035) at 32^3; the bar is twice that"""
    from f2_nerf_amd import capi
    from test_tsdf_cpu import sphere_case
    c, _ = sphere_case(fox_state, 32)
    S, W = torch.zeros((32, 32, 32), device="cuda"), torch.zeros((32, 32, 32), device="cuda")
    capi.tsdf_integrate(S, W, c["lo"], float(c["step"]), _dev(c["poses"]), _dev(c["intri"]), _dev(c["dist"]), _dev(c["depth"]), _dev(c["conf"]),
                        float(c["trunc"]))
    g, valid = capi.tsdf_finalize(S, W, 1.0)
    v, f = rt.host().mesh_from_grid_masked(g, valid, [float(x) for x in c["lo"]], float(c["step"]), 0.0)
    for rc in casters:
        cpu.check_loop_closure(rc, (v.cpu().numpy(), f.cpu().numpy()), c)


# ---- the fox scene -----------------------------------------------------------------------------------------------------------------
BOX = ([-1.0, -0.8, -0.9], [1.0, 0.7, 1.05])  # the box of tests/test_gpu_mesh_attrs.py::test_extract_mesh_attrs_on_the_fox
CHECK = dict(res_level=16, tau=1e-3, min_opacity=1e-3, max_views=3)  # thresholds an untrained field can meet


def _fox_mesh(rt, runner, res=48):
    lo, hi = BOX
    g = runner.density_grid(lo, hi, res).cpu().numpy()
    level = float(np.quantile(g[g > 0], 0.5))  # a level the scene crosses
    v, f = runner.extract_mesh(lo, hi, res, level)
    return v, f, rt.host().grid_spec(lo, hi, res)[0]


def test_check_mesh_on_the_fox(rt, fox_state):
    from f2_nerf_amd import mesh
    st = fox_state
    runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    ds = rt.make_dataset(st)
    h = rt.host()
    v, f, step = _fox_mesh(rt, runner)
    assert len(f) > 1000
    o = dict(CHECK, step=step)
    res = mesh.check_mesh(runner, ds, st, v, f, o)
    assert res == mesh.check_mesh(runner, ds, st, v, f, o)
    keys = {"n_rays", "n_field", "n_mesh", "n_both", "completeness", "extra", "mean", "median", "p90", "max", "within_1", "within_2", "faces_seen",
            "normal_agreement", "n_views", "n_faces", "step", "res_level", "tau", "min_opacity", "views"}
    assert set(res) == keys and res["n_views"] == 3 == len(res["views"]) and res["n_faces"] == len(f)
    json.dumps(res)
    # the same from render_geometry and host.mesh_raycast in numpy
    accel = h.mesh_raycast_build(v, f)
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    pool, seen, agree = [[], [], [], []], np.zeros(len(fn), bool), []
    for k, idx in enumerate(int(x) for x in st["train_set"][:3]):
        ro, rd, b, _, _ = mesh.tsdf_camera_rays(ds, st["bounds"], idx, 16)
        g = runner.render_geometry(ro, rd, b, tau=o["tau"])
        hf = ((g["surf_idx"] >= 0) & (g["opacity"] >= o["min_opacity"])).cpu().numpy()
        out = h.mesh_raycast(v, f, accel, ro, rd, b)
        assert cpu.same(_np(out), _np(h.mesh_raycast(v, f, None, ro, rd, b)))  # the traversal equals the device's brute force
        t, face, bary = _np(out)
        hm = face >= 0
        r = rr.render(vn, fn, ro.cpu().numpy(), rd.cpu().numpy(), t, face, bary)
        seen[face[hm]] = True
        both = hf & hm
        a = np.abs((r["face_normals"][both] * g["surf_normals"].cpu().numpy()[both].astype(np.float64)).sum(1))
        agree.append(a)
        ref = rr.compare_depth(g["surf_t"].cpu().numpy(), hf, t, hm, step)
        view = res["views"][k]
        assert view["view"] == idx and all(abs(view[key] - ref[key]) <= 1e-6 * max(1.0, abs(ref[key])) for key in ref), (view, ref)
        assert abs(view["normal_agreement"] - (a.mean() if len(a) else 0.0)) < 1e-5
        for lst, x in zip(pool, (g["surf_t"].cpu().numpy(), hf, t, hm)):
            lst.append(x)
    ref = rr.compare_depth(*(np.concatenate(x) for x in pool), step)
    print("fox 48^3 (untrained table), 3 views at 1/16:", {k: res[k] for k in sorted(keys - {"views"})})
    assert all(abs(res[key] - ref[key]) <= 1e-6 * max(1.0, abs(ref[key])) for key in ref), (res, ref)
    assert res["faces_seen"] == seen.sum() / len(fn) and abs(res["normal_agreement"] - np.concatenate(agree).mean()) < 1e-5
    assert res["n_mesh"] > 0 and res["n_field"] > 0 and res["n_both"] > 0 and 0 < res["faces_seen"] < 1


def test_check_mesh_has_no_effect_on_training(rt, fox_state):
    from f2_nerf_amd import mesh
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 4096, rng)) for _ in range(6)]
    ds = rt.make_dataset(st)

    def run(check):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=15"], seed=3, table_init=0.3)
        runner.n_edge_pts = 512
        losses = []
        for k, b in enumerate(batches):
            if check and k == 3:
                v, f, step = _fox_mesh(rt, runner, 32)
                res = mesh.check_mesh(runner, ds, st, v, f, dict(CHECK, max_views=2, step=step))
                assert res["n_rays"] > 0 and res["n_mesh"] > 0
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [x.detach().cpu().numpy().copy() for x in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))


def test_launcher_writes_the_check(tmp_path, monkeypatch, capsys):
    """The synthetic rig of tests/test_gpu_mesh_simplify.py's launcher test: mesh.check=true writes <name>_check.json with the documented
    keys for source=density, source=tsdf and simplify=2, and prints its line; without the option the .ply carries the same bytes and there
    is no JSON."""
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
    keys = {"n_rays", "n_field", "n_mesh", "n_both", "completeness", "extra", "mean", "median", "p90", "max", "within_1", "within_2", "faces_seen",
            "normal_agreement", "n_views", "n_faces", "step", "res_level", "tau", "min_opacity", "views"}
    capsys.readouterr()
    for extra, name in (([], "60_24"), (["mesh.simplify=2"], "60_24_s2"), (tsdf, "60_24_tsdf"), (tsdf + ["mesh.simplify=2"], "60_24_tsdf_s2")):
        assert run.main(ex + extra) == 0
        plain_out = capsys.readouterr().out
        ply = open(meshes / (name + ".ply"), "rb").read()
        assert not (meshes / (name + "_check.json")).exists() and "Check:" not in plain_out
        assert run.main(ex + extra + chk) == 0
        out = capsys.readouterr().out
        assert open(meshes / (name + ".ply"), "rb").read() == ply
        res = json.load(open(meshes / (name + "_check.json")))
        assert set(res) == keys and res["n_views"] == 5 and res["n_rays"] == 5 * 24 * 32 and res["res_level"] == 2 and len(res["views"]) == 5
        line = [ln for ln in out.split("\n") if ln.startswith("Check:")]
        assert len(line) == 1 and all(w in line[0] for w in ("completeness", "median", "p90", "extra", "faces seen", name + "_check.json"))
        assert [ln for ln in out.split("\n") if ln.startswith("Mesh:")] == [ln for ln in plain_out.split("\n") if ln.startswith("Mesh:")]
        with capsys.disabled():
            print(name, line[0])
    with pytest.raises(ValueError):
        run.main(ex + ["mesh.check=true", "check.res_level=0"])
