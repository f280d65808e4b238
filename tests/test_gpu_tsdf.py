"""TSDF fusion on the MI355X: f2n_tsdf_integrate / f2n_tsdf_finalize through the ctypes binding against the float32 restatement of
tests/tsdf_ref.py (bit for bit, with the batching and second-call identities), the masked mesher through the host module, mesh.fuse_tsdf
on the fox scene against the entry point fed the same renders, no effect on training, and the launcher's mesh.source=tsdf."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tsdf_ref as tr  # noqa: E402
from test_tsdf_cpu import check_integrate, check_masked_mesher  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


def _dev(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def device_integrate(c, S, W, v0, v1, conf):
    """capi.tsdf_integrate of the views [v0, v1) into the host arrays S, W (up, launch, down)."""
    from f2_nerf_amd import capi
    cf = c["conf"] if isinstance(conf, str) else conf
    dS, dW = _dev(S), _dev(W)
    capi.tsdf_integrate(dS, dW, c["lo"], float(c["step"]), _dev(c["poses"][v0:v1]), _dev(c["intri"][v0:v1]), _dev(c["dist"][v0:v1]),
                        _dev(c["depth"][v0:v1]), None if cf is None else _dev(cf[v0:v1]), float(c["trunc"]))
    S[...] = dS.cpu().numpy()
    W[...] = dW.cpu().numpy()


def device_finalize(S, W, min_weight):
    from f2_nerf_amd import capi
    g, valid = capi.tsdf_finalize(_dev(S), _dev(W), min_weight)
    return g.cpu().numpy(), valid.cpu().numpy()


@pytest.mark.parametrize("dims,n_views,hw,with_conf", [((37, 21, 19), 5, (61, 45), True), ((37, 21, 19), 5, (61, 45), False),
                                                       ((130, 67, 33), 9, (120, 67), True)])
def test_entry_points_match_the_restatement(fox_state, dims, n_views, hw, with_conf):
    c = tr.synthetic_case(fox_state, dims=dims, n_views=n_views, hw=hw, with_conf=with_conf)
    assert c["depth"].shape == (n_views,) + hw and dims[0] * dims[1] * dims[2] % 256 != 0
    check_integrate(c, device_integrate, device_finalize)
    from f2_nerf_amd import capi
    with pytest.raises(capi.F2nError):
        bad = dict(c)
        bad["trunc"] = 0.0
        z = np.zeros((c["nz"], c["ny"], c["nx"]), F32)
        device_integrate(bad, z, z.copy(), 0, n_views, "case")


def test_masked_mesher_through_the_host_module(rt):
    host = rt.host()

    def mesh_fn(g, valid, level, lo, step):
        if valid is None:
            v, f = host.mesh_from_grid(_dev(g), level, list(lo), step)
        else:
            v, f = host.mesh_from_grid_masked(_dev(g), _dev(valid, np.uint8), list(lo), step, level)
        return dict(verts=v.cpu().numpy(), faces=f.cpu().numpy())

    check_masked_mesher(mesh_fn)
    # the ctypes binding gives the host module's mesh
    from f2_nerf_amd import capi
    from test_tsdf_cpu import mask_cases
    g, level, lo, step, masks = mask_cases()
    v, f = capi.mesh_from_grid_masked(_dev(g), _dev(masks["random"], np.uint8), lo, step, level)
    o = mesh_fn(g, masks["random"], level, lo, step)
    assert tr.same_bits(v.cpu().numpy(), o["verts"]) and (f.cpu().numpy() == o["faces"]).all()


def _fox_options(st, **kw):
    """A 32^3 box from the fox cameras to the point they look at; thresholds an untrained field can meet (a ray that meets the scene
    accumulates 1e-3 of weight within a few samples)."""
    ts = np.asarray(st["train_set"])
    focus = tr.axes_focus(st["poses"][ts])
    eye = st["poses"][ts][:, :, 3].astype(np.float64).mean(0)
    half = 0.75 * np.linalg.norm(focus - eye)
    mid = 0.5 * (focus + eye)
    o = dict(bbox_min=[float(v) for v in mid - half], bbox_max=[float(v) for v in mid + half], resolution=31, res_level=8, trunc_voxels=4.0,
             tau=1e-3, min_opacity=1e-3, min_weight=1e-3, views_per_batch=3, max_views=4)
    o.update(kw)
    return o


def test_fuse_tsdf_on_the_fox(rt, fox_state):
    from f2_nerf_amd import capi, mesh
    st = fox_state
    runner, cfg, arrays = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    ds = rt.make_dataset(st)
    o = _fox_options(st)
    t = mesh.fuse_tsdf(runner, ds, st, o)
    assert {"g", "valid", "S", "W", "lo", "step"} <= set(t)
    assert t["S"].shape == (32, 32, 32) and t["valid"].dtype == torch.uint8
    # the entry point fed the same renders: the first four training cameras on the sub-grid of tsdf_camera_rays
    views = [int(v) for v in st["train_set"][:4]]
    H, Wd = (int(v) for v in st["image_hw"])
    h, w = H // 8, Wd // 8
    depth, conf = [], []
    for idx in views:
        ro, rd, b, hh, ww = mesh.tsdf_camera_rays(ds, st["bounds"], idx, 8)
        assert (hh, ww) == (h, w) and ro.shape == (h * w, 3)
        g = runner.render_geometry(ro, rd, b, tau=o["tau"])
        hit = (g["surf_idx"] >= 0) & (g["opacity"] >= o["min_opacity"])
        depth.append(torch.where(hit, g["surf_t"], torch.zeros_like(g["surf_t"])).reshape(h, w))
        conf.append(g["opacity"].reshape(h, w))
    depth, conf = torch.stack(depth).contiguous(), torch.stack(conf).contiguous()
    S, W = torch.zeros((32, 32, 32), device="cuda"), torch.zeros((32, 32, 32), device="cuda")
    trunc = float(F32(o["trunc_voxels"]) * F32(t["step"]))
    intri = mesh.tsdf_intrinsics(st["intri"][views], 8)
    capi.tsdf_integrate(S, W, t["lo"], t["step"], _dev(st["poses"][views]), _dev(intri), _dev(st["dist_params"][views]), depth, conf, trunc)
    g, valid = capi.tsdf_finalize(S, W, o["min_weight"])
    n = lambda x: x.cpu().numpy()  # noqa: E731
    print("rays with a surface: %d of %d; grid points with weight: %d, known: %d of %d" % (
        int((depth > 0).sum()), depth.numel(), int((W > 0).sum()), int(valid.sum()), valid.numel()))
    assert (depth > 0).any() and (W > 0).any()  # (nothing is asserted about the surface of an untrained field)
    assert tr.same_bits(n(t["S"]), n(S)) and tr.same_bits(n(t["W"]), n(W)) and tr.same_bits(n(t["g"]), n(g)) and tr.same_bits(n(t["valid"]), n(valid))
    # ... and the restatement fed the same depth maps
    z = np.zeros((32, 32, 32), F32)
    rs, rw = tr.integrate(z, z, t["lo"], t["step"], 32, 32, 32, st["poses"][views], intri, st["dist_params"][views], n(depth), n(conf), trunc)
    assert tr.same_bits(n(S), rs) and tr.same_bits(n(W), rw)
    for vpb in (1, 4):  # the batch size does not show
        t2 = mesh.fuse_tsdf(runner, ds, st, _fox_options(st, views_per_batch=vpb))
        assert tr.same_bits(n(t2["S"]), n(S)) and tr.same_bits(n(t2["W"]), n(W)) and tr.same_bits(n(t2["g"]), n(g))
    v, f = rt.host().mesh_from_grid_masked(t["g"], t["valid"], t["lo"], t["step"], 0.0)
    tr.check_masked_mesh(n(v), n(f), n(g), 0.0, n(valid), t["lo"], t["step"])


def test_fuse_tsdf_has_no_effect_on_training(rt, fox_state):
    from f2_nerf_amd import mesh
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 4096, rng)) for _ in range(6)]
    ds = rt.make_dataset(st)

    def run(query):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=15"], seed=3, table_init=0.3)
        runner.n_edge_pts = 512
        losses = []
        for k, b in enumerate(batches):
            if query and k == 3:
                t = mesh.fuse_tsdf(runner, ds, st, _fox_options(st, max_views=2, views_per_batch=2))
                assert (t["W"] > 0).any()
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [x.detach().cpu().numpy().copy() for x in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))


def test_launcher_extract_mesh_from_the_tsdf(tmp_path):
    """mode=extract_mesh mesh.source=tsdf on the tiny scene of tests/test_gpu_mesh.py::test_launcher_extract_mesh.  A scene trained for
    60 iterations is translucent, so the thresholds are lowered until rays qualify; the file must be a PLY whose faces index its vertices."""
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
    assert run.main(common + opts) == 0 and os.path.exists(path)
    v, f = test_mesh_cpu.read_ply(path)
    print("TSDF mesh of the tiny scene: %d vertices, %d faces" % (len(v), len(f)))
    assert np.isfinite(v).all() and f.min(initial=0) >= 0 and f.max(initial=-1) < len(v) and len(np.unique(f)) == len(v)
    assert not os.path.exists(str(tmp_path / "exp" / "rig" / "t" / "meshes" / "60_24.ply"))
    # with floater removal, normals from the field and colours: the vertex element carries them, the faces still index it
    os.remove(path)
    assert run.main(common + opts + ["mesh.normals=true", "mesh.colors=true", "mesh.normal_source=field", "mesh.min_component_faces=2"]) == 0
    with open(path, "rb") as fh:
        head, body = fh.read().split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    nv, nf = (int([ln for ln in lines if ln.startswith("element " + e)][0].split()[-1]) for e in ("vertex", "face"))
    props = [ln.split()[1:] for ln in lines if ln.startswith("property") and not ln.startswith("property list")]
    vr = np.frombuffer(body, np.dtype([(name, {"float": "<f4", "uchar": "u1"}[ty]) for ty, name in props]), nv)
    rest = body[nv * vr.dtype.itemsize:]
    assert vr.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue") and nv == len(v) and nf == len(f)
    rec = np.frombuffer(rest, [("n", "u1"), ("idx", "<i4", (3,))])
    assert len(rec) == nf and (rec["n"] == 3).all() and rec["idx"].min(initial=0) >= 0 and rec["idx"].max(initial=-1) < len(vr)
    ln = np.sqrt(vr["nx"].astype(np.float64) ** 2 + vr["ny"].astype(np.float64) ** 2 + vr["nz"].astype(np.float64) ** 2)
    assert ((np.abs(ln - 1) < 1e-5) | (ln == 0)).all()
    with pytest.raises(ValueError):
        run.main(common + ["mode=extract_mesh", "is_continue=true", "mesh.source=points"])
