"""Mesh-to-mesh distance on the MI355X (csrc/octree.hip, host/RendererQuery.cpp): the bodies of tests/test_mesh_distance_cpu.py against the
device through host.mesh_closest_point / host.mesh_sample_surface (twice in a row) and capi.*, bit for bit with the numpy restatement
(tests/mesh_distance_ref.py); the grid walk against the device's own brute-force mode on the 33^3 sphere; mesh.mesh_distance of that
sphere's simplified version; the launcher's mesh.distance and mesh.distance_to."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_ref as mr  # noqa: E402
import test_mesh_distance_cpu as cpu  # noqa: E402

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


def _closer(build_fn, closest_fn, sample_fn):
    def build(v, f, cell=None, lo=None):
        return build_fn(_dev(v).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3), cell, None if lo is None else [float(x) for x in lo])

    def closest(v, f, accel, p, max_dist=float("inf")):
        return _np(closest_fn(_dev(v).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3), accel, _dev(p).reshape(-1, 3), float(max_dist)))

    def sample(v, f, n, seed=0):
        return _np(sample_fn(_dev(v).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3), int(n), int(seed)))
    return cpu.Closer(build, closest, sample, RuntimeError)


@pytest.fixture(scope="module")
def closers(rt):
    from f2_nerf_amd import capi
    h = rt.host()
    return (_closer(h.mesh_raycast_build, h.mesh_closest_point, h.mesh_sample_surface),
            _closer(capi.mesh_raycast_build, capi.mesh_closest_point, capi.mesh_sample_surface))


def test_device_matches_the_restatement(closers):
    host, capi = closers
    cpu.check_against_restatement(host)
    cpu.check_against_restatement(host)  # twice in a row
    cpu.check_against_restatement(capi)


def test_point_and_face_order_and_the_cut_off(closers):
    for cl in closers:
        cpu.check_independence(cl)
        cpu.check_cutoff(cl)


def test_contract_cases(closers):
    for cl in closers:
        cpu.check_contract(cl)


def test_sampling(closers):
    host, capi = closers
    cpu.check_sampling(host)
    cpu.check_sampling(host)
    cpu.check_sampling(capi)


def test_mesh_distance_through_the_device(closers):
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    host, capi = closers
    cpu.check_mesh_distance(host)
    cpu.check_mesh_distance(capi)
    # the default backend (torch tensors or numpy arrays in, the same dict out)
    v, f = cpu.sphere_case()[:2]
    (va, fa), (vb, fb) = cpu.square(1.0, 0.0), cpu.square(3.0, 0.0, -1.0)
    want = mesh.mesh_distance(va, fa, vb, fb, n=1000, thresholds=(0.25,), backend=host)
    assert mesh.mesh_distance(va, fa, vb, fb, n=1000, thresholds=(0.25,)) == want
    assert mesh.mesh_distance(_dev(va), _dev(fa, np.int32), _dev(vb), _dev(fb, np.int32), n=1000, thresholds=(0.25,)) == want


@pytest.fixture(scope="module")
def sphere33(rt):
    """the 33^3 sphere of the simplifier's known answer (18 408 faces) and its simplify=2 version (1 548 faces)"""
    h = rt.host()
    v, f = h.mesh_from_grid(_dev(mr.sphere_grid(33, 0.4 * 32)), 0.0, [0.0, 0.0, 0.0], 1.0)
    sv, sf, _ = h.mesh_simplify(v, f, 2.0, [0.0, 0.0, 0.0])
    assert len(f) == 18408 and len(sf) == 1548
    return v, f, sv, sf


def test_grid_walk_against_brute_force_on_the_devices_own_sphere(rt, sphere33):
    """4 096 surface samples of the simplified 33^3 sphere against the unsimplified one (18 408 faces): the walk over the default grid and
    over a one-step grid equals the device's brute-force mode bit for bit, with and without a cut-off"""
    h = rt.host()
    v, f, sv, sf = sphere33
    p = h.mesh_sample_surface(sv, sf, 4096, 0)[0]
    brute = _np(h.mesh_closest_point(v, f, None, p))
    assert (brute[1] >= 0).all() and 0 < brute[0].max() < 2.0 * np.sqrt(3.0)
    for accel in (h.mesh_raycast_build(v, f), h.mesh_raycast_build(v, f, 1.0, [0.0, 0.0, 0.0])):
        assert cpu.same(_np(h.mesh_closest_point(v, f, accel, p)), brute)
    md = float(np.median(brute[0]))
    cut = _np(h.mesh_closest_point(v, f, None, p, md))
    assert 1000 < (cut[1] < 0).sum() < 3000 and cpu.same(_np(h.mesh_closest_point(v, f, h.mesh_raycast_build(v, f), p, md)), cut)
    # from far outside and from the centre: every face is as near as any other to within the sphere's facets
    far = _dev([[16.0, 16.0, 16.0], [200.0, 16.0, 16.0], [-50.0, -60.0, 300.0]])
    assert cpu.same(_np(h.mesh_closest_point(v, f, h.mesh_raycast_build(v, f), far)), _np(h.mesh_closest_point(v, f, None, far)))


def test_mesh_distance_of_the_simplified_sphere(rt, sphere33):
    """Finite and consistent: chamfer is the mean of the two means, the F-score does not decrease with the threshold, and a_to_b.max is at
    most the simplifier's cell diagonal 2 step sqrt(3): a simplified vertex never leaves its cell, and every cell it occupies holds an
    input vertex."""
    from f2_nerf_amd import mesh
    v, f, sv, sf = sphere33
    res = mesh.mesh_distance(sv, sf, v, f, n=20000, thresholds=(0.05, 0.1, 0.25, 0.5, 1.0))
    print("sphere 33^3, simplify=2 against the unsimplified mesh:", json.dumps(res))
    assert res == mesh.mesh_distance(sv, sf, v, f, n=20000, thresholds=(0.05, 0.1, 0.25, 0.5, 1.0))
    for side in ("a_to_b", "b_to_a"):
        s = res[side]
        assert s["n"] == 20000 and s["missed"] == 0 and all(np.isfinite(s[k]) for k in s)
        assert 0 < s["median"] <= s["p90"] <= s["p95"] <= s["max"] and 0 < s["mean"] <= s["rms"] <= s["max"]
    assert res["chamfer"] == 0.5 * (res["a_to_b"]["mean"] + res["b_to_a"]["mean"]) and res["hausdorff"] == max(res["a_to_b"]["max"], res["b_to_a"]["max"])
    assert res["a_to_b"]["max"] <= 2.0 * np.sqrt(3.0)
    assert all(a <= b for a, b in zip(res["fscore"], res["fscore"][1:])) and res["fscore"][-1] == 1.0 and res["fscore"][0] < 1.0
    assert res["n_faces_a"] == 1548 and res["n_faces_b"] == 18408
    half = mesh.mesh_distance(sv, sf, v, f, n=20000, unit=0.5)
    assert abs(half["hausdorff"] - 2.0 * res["hausdorff"]) < 1e-9 and abs(half["chamfer"] - 2.0 * res["chamfer"]) < 1e-9


def test_launcher_writes_the_distance(tmp_path, monkeypatch, capsys):
    """The synthetic rig of tests/test_gpu_mesh_simplify.py's launcher test.  Without the option the .ply and _check.json carry the same
    bytes and there is no _distance.json; mesh.simplify=2 mesh.distance=true writes <name>_distance.json with the documented keys and
    prints one Distance: line, for source=density and source=tsdf; mesh.distance_to=<the run's own unsimplified .ply> gives the figures
    of the built-in comparison within 1e-5 grid steps (the world-frame round trip through a float PLY; measured: 0, since both comparisons
    run on the float32 world vertices the .ply carries -- with the built-in one in the normalised frame a few of the 20 000 samples
    changed face and the figures were 5.9e-5 apart); mesh.distance=true alone raises."""
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
    chk = ["mesh.check=true", "check.res_level=2", "check.tau=0.0001", "check.min_opacity=0.0001", "check.max_views=3"]
    tsdf = ["mesh.source=tsdf", "tsdf.res_level=2", "tsdf.tau=0.0001", "tsdf.min_opacity=0.0001", "tsdf.min_weight=0.0001"]
    dist = ["distance.samples=20000", "distance.seed=1", "distance.thresholds=[0.25,1,4]"]
    keys = {"a_to_b", "b_to_a", "chamfer", "hausdorff", "thresholds", "precision", "recall", "fscore", "unit", "seed", "n_faces_a", "n_faces_b",
            "max_dist", "against"}
    stat_keys = {"n", "missed", "mean", "rms", "median", "p90", "p95", "max"}
    capsys.readouterr()
    results = {}
    for extra, name in (([], "60_24_s2"), (tsdf, "60_24_tsdf_s2")):
        assert run.main(ex + extra + ["mesh.simplify=2"] + chk) == 0
        plain_out = capsys.readouterr().out
        ply, check = open(meshes / (name + ".ply"), "rb").read(), open(meshes / (name + "_check.json"), "rb").read()
        assert not (meshes / (name + "_distance.json")).exists() and "Distance:" not in plain_out
        assert run.main(ex + extra + ["mesh.simplify=2", "mesh.distance=true"] + chk + dist) == 0
        out = capsys.readouterr().out
        assert open(meshes / (name + ".ply"), "rb").read() == ply and open(meshes / (name + "_check.json"), "rb").read() == check
        res = json.load(open(meshes / (name + "_distance.json")))
        assert set(res) == keys and set(res["a_to_b"]) == stat_keys == set(res["b_to_a"]) and res["against"] == "unsimplified"
        assert res["thresholds"] == [0.25, 1.0, 4.0] and res["seed"] == 1 and res["a_to_b"]["n"] == 20000 == res["b_to_a"]["n"]
        assert res["a_to_b"]["missed"] == 0 == res["b_to_a"]["missed"] and 0 < res["a_to_b"]["max"] and 0 < res["b_to_a"]["max"]
        assert all(0.0 <= a <= b <= 1.0 for a, b in zip(res["fscore"], res["fscore"][1:]))
        assert res["n_faces_a"] < res["n_faces_b"] and res["chamfer"] == 0.5 * (res["a_to_b"]["mean"] + res["b_to_a"]["mean"])
        line = [ln for ln in out.split("\n") if ln.startswith("Distance:")]
        assert len(line) == 1 and all(w in line[0] for w in ("chamfer", "p95", "hausdorff", "F-score", name + "_distance.json"))
        for head in ("Mesh:", "Check:"):
            assert [ln for ln in out.split("\n") if ln.startswith(head)] == [ln for ln in plain_out.split("\n") if ln.startswith(head)]
        results[name] = res
        with capsys.disabled():
            print(name, line[0])
    # against the run's own unsimplified .ply, in the world frame
    assert run.main(ex) == 0
    capsys.readouterr()
    assert run.main(ex + ["mesh.simplify=2", "mesh.distance_to=%s" % (meshes / "60_24.ply")] + dist) == 0
    out = capsys.readouterr().out
    res, want = json.load(open(meshes / "60_24_s2_distance.json")), results["60_24_s2"]
    assert res["against"].endswith("60_24.ply") and len([ln for ln in out.split("\n") if ln.startswith("Distance:")]) == 1
    assert res["n_faces_a"] == want["n_faces_a"] and res["n_faces_b"] == want["n_faces_b"]
    worst = 0.0
    for side in ("a_to_b", "b_to_a"):
        for k in stat_keys - {"n", "missed"}:
            worst = max(worst, abs(res[side][k] - want[side][k]))
        assert res[side]["missed"] == 0
    worst = max(worst, abs(res["chamfer"] - want["chamfer"]), abs(res["hausdorff"] - want["hausdorff"]))
    with capsys.disabled():
        print("distance_to against the built-in comparison: largest difference %.3g grid steps" % worst)
    assert worst <= 1e-5 and max(abs(a - b) for a, b in zip(res["fscore"], want["fscore"])) <= 1e-3
    with pytest.raises(ValueError):
        run.main(ex + ["mesh.distance=true"])
