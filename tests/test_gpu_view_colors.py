"""View-colour fusion on the MI355X: f2n_view_colors_accumulate / f2n_view_colors_finalize through the ctypes binding against the float32
restatement of tests/view_colors_ref.py (bit for bit, with the batching and second-call identities and the error codes), the sphere's
known answer and the occlusion case through the host module, mesh.fuse_view_colors on the fox scene against the render it projects
into, no effect on training, and the launcher's mesh.color_source=views / texture.source=views."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tsdf_ref as tr  # noqa: E402
import view_colors_ref as vr  # noqa: E402
from test_view_colors_cpu import check_accumulate, check_error_codes  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


def _dev(a, dt=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _views(c, v0, v1, conf="case"):
    cf = c["conf"] if isinstance(conf, str) else conf
    return [_dev(c[k][v0:v1]) for k in ("poses", "intri", "dist", "depth")] + [None if cf is None else _dev(cf[v0:v1]), _dev(c["image"][v0:v1])]


def device_accumulate(c, acc, wsum, count, v0, v1, conf, normals):
    """capi.view_colors_accumulate of the views [v0, v1) into the host arrays acc, wsum, count (up, launch, down)."""
    from f2_nerf_amd import capi
    nr = c["normals"] if isinstance(normals, str) else normals
    da, dw, dc = _dev(acc), _dev(wsum), _dev(count, np.int32)
    capi.view_colors_accumulate(da, dw, dc, _dev(c["points"]), _dev(nr), *_views(c, v0, v1, conf), float(c["tol"]), float(c["cos_min"]))
    acc[...] = da.cpu().numpy()
    wsum[...] = dw.cpu().numpy()
    count[...] = dc.cpu().numpy()


def device_finalize(acc, wsum, count, min_views):
    from f2_nerf_amd import capi
    rgb, known = capi.view_colors_finalize(_dev(acc), _dev(wsum), _dev(count, np.int32), min_views)
    return rgb.cpu().numpy(), known.cpu().numpy()


@pytest.mark.parametrize("C", [1, 3, 4])
def test_entry_points_match_the_restatement(fox_state, C):
    check_accumulate(vr.grid_case(fox_state), C, device_accumulate, device_finalize)


def test_a_large_case_matches_the_restatement(fox_state):
    """200 003 random points against 9 views of 120 x 67: more than one block per compute unit's worth, no multiple of 256."""
    c = vr.big_case(fox_state)
    n = len(c["points"])
    assert n == 200003 and c["depth"].shape == (9, 120, 67)
    stats = {}
    ref = vr.accumulate(np.zeros((n, 3), F32), np.zeros(n, F32), np.zeros(n, np.int32), c["points"], c["normals"], c["poses"], c["intri"], c["dist"],
                        c["depth"], c["conf"], c["image"], c["tol"], c["cos_min"], stats)
    assert all(stats[k] > 0 for k in ("behind", "facing", "no_tap", "tap_outside", "no_depth", "depth_low", "depth_high", "conf0", "used_1", "used_4")), stats
    got = (np.zeros((n, 3), F32), np.zeros(n, F32), np.zeros(n, np.int32))
    device_accumulate(c, *got, 0, 9, "case", "case")
    assert all(tr.same_bits(a, b) for a, b in zip(got, ref))
    rgb, known = device_finalize(*got, 2)
    rr, rk = vr.finalize(*ref, 2)
    assert tr.same_bits(rgb, rr) and tr.same_bits(known, rk) and 0 < rk.mean() < 1


def test_error_codes_through_the_binding(fox_state):
    """The binding raises on every status the entry point refuses with, and passes the calls that touch nothing."""
    from f2_nerf_amd import capi
    c = vr.grid_case(fox_state)
    c = dict(c, image=vr.image_for(c, 3), points=c["points"][:300], normals=c["normals"][:300])
    state = dict(acc=torch.full((300, 3), 7.0, device="cuda"), wsum=torch.full((300,), 7.0, device="cuda"),
                 count=torch.full((300,), 7, dtype=torch.int32, device="cuda"))
    po, ki, di, de, cf, im = _views(c, 0, 5)
    dev = dict(points=_dev(c["points"]), normals=_dev(c["normals"]), poses=po, intri=ki, dist=di, depth=de, conf=cf, image=im, **state)

    def call(**raw):  # the raw entry point with the binding's pointers: the statuses themselves
        a = dict(n=300, V=5, C=3, h=c["h"], w=c["w"], tol=float(c["tol"]), cos_min=float(c["cos_min"]), **dev)
        a.update(raw)
        import ctypes
        p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
        return capi.lib().f2n_view_colors_accumulate(capi._stream(), ctypes.c_int64(a["n"]), p(a["points"]), p(a["normals"]), ctypes.c_int(a["V"]),
                                                     p(a["poses"]), p(a["intri"]), p(a["dist"]), p(a["depth"]), p(a["conf"]), p(a["image"]),
                                                     ctypes.c_int(a["C"]), ctypes.c_int(a["h"]), ctypes.c_int(a["w"]), ctypes.c_float(a["tol"]),
                                                     ctypes.c_float(a["cos_min"]), p(a["acc"]), p(a["wsum"]), p(a["count"]))

    check_error_codes(call)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in state.values())  # nothing was written by any of the calls above
    for bad in (dict(tol=0.0), dict(tol=float("inf")), dict(cos_min=float("nan"))):
        with pytest.raises(capi.F2nError):
            a = dict(tol=float(c["tol"]), cos_min=float(c["cos_min"]))
            a.update(bad)
            capi.view_colors_accumulate(state["acc"], state["wsum"], state["count"], dev["points"], dev["normals"], po, ki, di, de, cf, im, a["tol"], a["cos_min"])
    with pytest.raises(capi.F2nError):
        capi.view_colors_accumulate(state["acc"], state["wsum"], state["count"], dev["points"], dev["normals"], po, ki, di, de, cf, im[..., :2].contiguous(),
                                    0.1, 0.1)
    rgb, known = capi.view_colors_finalize(state["acc"][:0], state["wsum"][:0], state["count"][:0], 1)
    assert rgb.shape == (0, 3) and known.shape == (0,)


def host_fuse(rt):
    """vr.fuse's signature through the host module"""
    host = rt.host()

    def fuse(points, normals, case, C=3, min_views=1):
        n = len(points)
        acc, wsum = torch.zeros((n, C), device="cuda"), torch.zeros((n,), device="cuda")
        count = torch.zeros((n,), dtype=torch.int32, device="cuda")
        po, ki, di, de, cf, im = _views(case, 0, len(case["depth"]))
        host.view_colors_accumulate(acc, wsum, count, _dev(points), _dev(normals), po, ki, di, de, cf, im, float(case["tol"]), float(case["cos_min"]))
        rgb, known = host.view_colors_finalize(acc, wsum, count, min_views)
        return rgb.cpu().numpy(), known.cpu().numpy(), wsum.cpu().numpy(), count.cpu().numpy()
    return fuse


@pytest.fixture(scope="module")
def rig(fox_state):
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    return vr.sphere_rig(fox_state, mesh.view_intrinsics)


def test_sphere_colours_through_the_host_module(rt, rig):
    """The known answer of tests/test_view_colors_cpu.py on the device, under the same bound (vr.sphere_bound, 0.059), and the
    restatement's bits."""
    vr.check_sphere(rig, host_fuse(rt))
    for a, b in zip(vr.fuse(rig["points"], rig["normals"], rig), host_fuse(rt)(rig["points"], rig["normals"], rig)):
        assert tr.same_bits(a, b)


def test_occlusion_through_the_host_module(rt, rig):
    vr.check_occlusion(rig, host_fuse(rt))


def _fox_colors(**kw):
    """thresholds an untrained field can meet, as _fox_options of tests/test_gpu_tsdf.py; the tolerance is 2 steps of 0.05"""
    o = dict(color_source="views", res_level=8, tol_steps=2.0, cos_min=0.1, min_views=1, max_views=4, views_per_batch=8, tau=1e-3, min_opacity=1e-3,
             image="render", step=0.05)
    o.update(kw)
    return o


def test_fuse_view_colors_on_the_fox(rt, fox_state):
    """mesh.fuse_view_colors at the surface points of view 0's own rays, from view 0 alone: every point is known and takes its ray's
    rendered colour.  Tolerance: the point o + t d projects back to its pixel's centre (b + 0.5, a + 0.5) up to the float32 error of the
    round trip, eps pixels per axis: some 64 roundings of relative size 2^-24 on pixel coordinates of at most about 1.6 f, so
    eps <= 64 * 2^-24 * f_max (3.3e-4 pixels at f = 86; the restatement's own projection of these points is asserted to stay inside
    it).  The bilinear blend then gives the own pixel a weight of at least (1 - eps)^2 and its neighbours at most 2 eps together, so
    the colour moves by at most 2 eps * span, span = the range of the image's values, plus 4 * 2^-23 for the roundings of the blend
    itself.  The restatement fed the same maps gives the device's bits; the batch size does not show; image=photo gives the
    photographs' pixels under the same tolerance."""
    from f2_nerf_amd import mesh
    st = fox_state
    runner, cfg, arrays = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    H, Wd = (int(v) for v in st["image_hw"])
    gen = torch.Generator(device="cuda").manual_seed(3)
    photos = torch.rand((len(st["poses"]), H, Wd, 3), device="cuda", generator=gen)
    ds = rt.make_dataset(st, photos)
    views = [int(v) for v in st["train_set"][:4]]
    n = lambda x: x.cpu().numpy()  # noqa: E731
    ro, rd, b, h, w = mesh.tsdf_camera_rays(ds, st["bounds"], views[0], 8)
    g = runner.render_geometry(ro, rd, b, tau=1e-3)
    hit = (g["surf_idx"] >= 0) & (g["opacity"] >= 1e-3)
    pts, own = g["surf_points"][hit].contiguous(), n(g["colors"][hit])
    assert int(hit.sum()) > 100
    intri = mesh.view_intrinsics(st["intri"][views], 8)
    eps = 64 * 2.0 ** -24 * float(max(intri[0, 0, 0], intri[0, 1, 1]))
    _, _, x, y, _ = vr.project(n(pts), st["poses"][views[0]], intri[0], st["dist_params"][views[0]])
    a_own, b_own = np.divmod(np.flatnonzero(n(hit)), w)
    err_px = max(np.abs(x - (b_own + 0.5)).max(), np.abs(y - (a_own + 0.5)).max())
    print("%d surface points of %d rays; round-trip error %.3g pixels (bound %.3g)" % (len(own), hit.numel(), err_px, eps))
    assert err_px <= eps

    def tolerance(image):
        return 2 * eps * float(image.max() - image.min()) + 4 * 2.0 ** -23

    r = mesh.fuse_view_colors(runner, ds, st, pts, None, _fox_colors(max_views=1))
    assert {"colors", "known", "weight", "count", "n_views"} <= set(r) and r["n_views"] == 1 and r["colors"].shape == (len(own), 3)
    assert bool(r["known"].all()) and bool((r["count"] == 1).all())
    err = np.abs(n(r["colors"]) - own).max()
    print("colour error against the ray's own render: %.3g (tolerance %.3g)" % (err, tolerance(n(g["colors"]))))
    assert err <= tolerance(n(g["colors"]))
    # the restatement fed the same maps
    depth = n(torch.where(hit, g["surf_t"], torch.zeros_like(g["surf_t"])).reshape(1, h, w))
    case = dict(poses=st["poses"][views[:1]], intri=intri[:1], dist=st["dist_params"][views[:1]], depth=depth, conf=n(g["opacity"].reshape(1, h, w)),
                image=n(g["colors"].reshape(1, h, w, 3)), tol=r["tol"], cos_min=0.1)
    assert r["tol"] == float(F32(2.0) * F32(0.05))
    rgb, known, ws, cn = vr.fuse(n(pts), None, case)
    assert tr.same_bits(n(r["colors"]), rgb) and (n(r["known"]) == (known != 0)).all() and tr.same_bits(n(r["weight"]), ws) and tr.same_bits(n(r["count"]), cn)
    # four views, any batch size: the same bits
    base = mesh.fuse_view_colors(runner, ds, st, pts, None, _fox_colors(views_per_batch=4))
    assert base["n_views"] == 4 and bool((base["count"] >= 1).all())
    for vpb in (1, 3):
        other = mesh.fuse_view_colors(runner, ds, st, pts, None, _fox_colors(views_per_batch=vpb))
        assert all(tr.same_bits(n(other[k]), n(base[k])) for k in ("colors", "known", "weight", "count"))
    # the photographs in the place of the renders
    ij = mesh.tsdf_pixels(ds, 8)[0]
    photo = n(ds.gather_colors(torch.full((h * w,), views[0], dtype=torch.int32, device="cuda"), ij))
    assert tr.same_bits(photo, n(photos[views[0]][ij[:, 0].long(), ij[:, 1].long()]))
    p = mesh.fuse_view_colors(runner, ds, st, pts, None, _fox_colors(max_views=1, image="photo"))
    assert bool(p["known"].all()) and np.abs(n(p["colors"]) - photo[n(hit)]).max() <= tolerance(photo)
    assert tr.same_bits(n(p["weight"]), n(r["weight"]))


def test_fuse_view_colors_has_no_effect_on_training(rt, fox_state):
    from f2_nerf_amd import mesh
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 4096, rng)) for _ in range(6)]
    ds = rt.make_dataset(st)
    ts = np.asarray(st["train_set"])
    focus = tr.axes_focus(st["poses"][ts])
    pts = torch.from_numpy((focus[None] + rng.uniform(-0.3, 0.3, (2000, 3))).astype(F32)).cuda()

    def run(query):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=15"], seed=3, table_init=0.3)
        runner.n_edge_pts = 512
        losses = []
        for k, b in enumerate(batches):
            if query and k == 3:
                r = mesh.fuse_view_colors(runner, ds, st, pts, None, _fox_colors(max_views=2, views_per_batch=2, tol_steps=20.0))
                assert r["n_views"] == 2 and r["colors"].shape == (2000, 3)
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [x.detach().cpu().numpy().copy() for x in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))


# ---- the launcher -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """The tiny rig of tests/test_gpu_tsdf.py::test_launcher_extract_mesh_from_the_tsdf, trained for 60 iterations: (common options,
    the directory the meshes go to)."""
    from PIL import Image
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import rigs, run
    tmp_path = tmp_path_factory.mktemp("view_colors")
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
    return common + ["mode=extract_mesh", "is_continue=true", "mesh.resolution=24"], tmp_path / "exp" / "rig" / "t" / "meshes"


@pytest.fixture
def crossing_level(monkeypatch):
    """a density level the translucent scene crosses (as tests/test_gpu_mesh_texture.py sets it)"""
    from f2_nerf_amd import mesh
    orig = mesh.extract

    def spy(runner, cfg, scene, exp_dir, dataset=None):
        o = mesh.options(cfg)
        if o["source"] == "density":
            g = runner.density_grid(o["bbox_min"], o["bbox_max"], o["resolution"]).cpu().numpy()
            cfg["mesh"]["level"] = float(np.quantile(g[g > 0], 0.5)) if (g > 0).any() else 1.0
        return orig(runner, cfg, scene, exp_dir, dataset=dataset)

    monkeypatch.setattr(mesh, "extract", spy)


LOW = ["colors.tau=0.0001", "colors.min_opacity=0.0001"]  # (a 60-iteration field is translucent: thresholds its rays can meet)
TSDF = ["mesh.source=tsdf", "tsdf.res_level=2", "tsdf.tau=0.0001", "tsdf.min_opacity=0.0001", "tsdf.min_weight=0.0001"]


def _vertex_element(path):
    """(the names of the vertex properties, the vertex count) of a PLY's header"""
    with open(path, "rb") as fh:
        head = fh.read().split(b"end_header\n", 1)[0].decode("ascii").split("\n")
    return ([ln.split()[-1] for ln in head if ln.startswith("property") and not ln.startswith("property list")],
            int([ln for ln in head if ln.startswith("element vertex")][0].split()[-1]))


def _colors_line(out):
    line = [ln for ln in out.split("\n") if ln.startswith("Colors:")]
    assert len(line) == 1, out
    w = line[0].split()  # Colors: <known> of <n> vertices from <V> views (1/<res_level>, tol <t>)
    assert w[2] == "of" and w[4:6] == ["vertices", "from"] and w[7] == "views" and w[8] == "(1/2," and w[9] == "tol"
    return int(w[1]), int(w[3]), int(w[6])


@pytest.mark.parametrize("source", [[], TSDF, TSDF + ["tsdf.sparse=true", "mesh.normal_source=field"]], ids=["density", "tsdf", "tsdf_sparse"])
def test_launcher_colours_vertices_from_the_views(trained, crossing_level, capsys, source):
    from f2_nerf_amd import run
    ex, meshes = trained
    path = meshes / ("60_24_tsdf.ply" if source else "60_24.ply")
    capsys.readouterr()
    assert run.main(ex + source + LOW + ["mesh.colors=true", "mesh.color_source=views"]) == 0
    known, nv, n_views = _colors_line(capsys.readouterr().out)
    with capsys.disabled():
        print("%d of %d vertices coloured from %d views" % (known, nv, n_views))
    assert _vertex_element(path) == (["x", "y", "z", "red", "green", "blue"], nv)
    assert 1 <= known <= nv and n_views >= 2
    os.remove(path)


def test_launcher_colours_the_simplified_and_the_refined_vertices(trained, crossing_level, capsys):
    """mesh.sparse + mesh.simplify + mesh.refine: the colours are fused at the final vertices, and once more at the refined ones."""
    from f2_nerf_amd import run
    ex, meshes = trained
    capsys.readouterr()
    assert run.main(ex + LOW + ["mesh.colors=true", "mesh.color_source=views", "mesh.sparse=true", "mesh.normal_source=field", "mesh.simplify=2",
                                "mesh.refine=true"]) == 0
    lines = [ln.split() for ln in capsys.readouterr().out.split("\n") if ln.startswith("Colors:")]
    assert len(lines) == 2
    for w, name in zip(lines, ("60_24_s2.ply", "60_24_s2_r.ply")):
        assert _vertex_element(meshes / name) == (["x", "y", "z", "red", "green", "blue"], int(w[3])) and 1 <= int(w[1]) <= int(w[3])
        os.remove(meshes / name)


def test_launcher_default_colours_keep_their_bytes(trained, crossing_level, capsys):
    from f2_nerf_amd import run
    ex, meshes = trained
    path = meshes / "60_24.ply"
    capsys.readouterr()
    assert run.main(ex + ["mesh.colors=true"]) == 0
    absent, out = open(path, "rb").read(), capsys.readouterr().out
    os.remove(path)
    assert run.main(ex + ["mesh.colors=true", "mesh.color_source=radiance", "colors.res_level=4"]) == 0
    assert open(path, "rb").read() == absent and "Colors:" not in out and "Colors:" not in capsys.readouterr().out
    assert run.main(ex + LOW + ["mesh.colors=true", "mesh.color_source=views"]) == 0
    assert open(path, "rb").read() != absent  # (the views source does something)
    os.remove(path)
    with pytest.raises(ValueError):
        run.main(ex + ["mesh.colors=true", "mesh.color_source=photos"])


def test_launcher_bakes_a_texture_from_the_views(trained, crossing_level, capsys):
    from f2_nerf_amd import run
    ex, meshes = trained
    check = ["mesh.check=true", "check.res_level=2", "check.tau=0.0001", "check.min_opacity=0.0001", "check.max_views=5"]
    capsys.readouterr()
    assert run.main(ex + LOW + check + ["mesh.texture=true", "texture.source=views"]) == 0
    out = capsys.readouterr().out
    line = [ln for ln in out.split("\n") if ln.startswith("Texture:")]
    assert len(line) == 1 and "source views (" in line[0] and "texels from views)" in line[0] and "Colors:" not in out
    from_views = int(line[0].split("source views (")[1].split()[0])
    used = int(line[0].split(" texels used")[0].split()[-1])
    assert 1 <= from_views <= used
    assert all((meshes / ("60_24_tex" + ext)).exists() for ext in (".obj", ".mtl", ".png"))
    res = json.load(open(meshes / "60_24_check.json"))
    assert np.isfinite(res["texture_psnr"]) and res["n_texture_rays"] == res["n_both"] > 0
    with capsys.disabled():
        print(line[0], "texture_psnr %.2f over %d rays" % (res["texture_psnr"], res["n_texture_rays"]))
