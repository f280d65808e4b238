"""Texture baking on the MI355X (csrc/octree.hip, host/RendererQuery.cpp, mesh.py): the bodies of tests/test_atlas_cpu.py against the device
through host.mesh_atlas / mesh_atlas_texels / texture_sample (twice in a row) and their capi twins, bit for bit with the numpy restatement
(tests/atlas_ref.py); the device's own 33^3 sphere seen through mesh.render_mesh with a texture; runner.bake_texture on the fox scene, its
lack of effect on training; and the launcher's mesh.texture."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import atlas_ref as ar  # noqa: E402
import mesh_ref as mr  # noqa: E402
import test_atlas_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


def _dev(a, dt=F32):
    return torch.from_numpy(np.array(a, dtype=dt, order="C")).cuda()  # (a copy: the shared meshes and references are read-only)


def _atlas(mod):
    def atlas(v, f, density, max_size=8192, max_log=7):
        uv, size, b, d = mod.mesh_atlas(_dev(v).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3), float(density), int(max_size), int(max_log))
        return uv.cpu().numpy(), int(size), {k: x.cpu().numpy() for k, x in b.items()}, float(d)

    def texels(v, f, b, size, clamp):
        dt = {"offsets": np.int64}
        blocks = {k: _dev(x, dt.get(k, np.int32)) for k, x in b.items() if k != "size"}
        return tuple(x.cpu().numpy() for x in mod.mesh_atlas_texels(_dev(v).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3), blocks, int(size),
                                                                    bool(clamp)))

    def sample(tex, uv):
        return mod.texture_sample(_dev(tex), _dev(uv).reshape(-1, 2)).cpu().numpy()
    return cpu.Atlas(atlas, texels, sample)


@pytest.fixture(scope="module")
def atlases(rt):
    from f2_nerf_amd import capi
    return _atlas(rt.host()), _atlas(capi)


@pytest.mark.parametrize("name", cpu.MESHES)
def test_device_matches_the_restatement(atlases, name):
    host, capi = atlases
    cpu.check_mesh_case(host, name)
    cpu.check_mesh_case(host, name, n_random=4)  # twice in a row
    cpu.check_mesh_case(capi, name, n_random=4)


def test_face_order_halving_contract_and_lookup(atlases):
    for A in atlases:
        cpu.check_face_order(A, "strip")
        cpu.check_face_order(A, "odd")
        assert cpu.check_halving(A) == cpu.check_halving(cpu.ref_atlas())
        cpu.check_contract(A)
        cpu.check_sample(A)


# ---- the device's own sphere seen through a texture --------------------------------------------------------------------------------
def render_bound(S, density, grad):
    """What tex_colors may differ from c(points) by, for a mesh with coordinates and ray distances below 128 (ulp = 2^-17):
    the bound of the lookup itself (cpu.LINEAR_BOUND), plus the colour's gradient `grad` (per length unit) times
      the distance between the ray caster's point o + t d and the point its barycentrics name: the caster shears the vertices in fp32
      relative to the origin (one rounding of q = P - o and two of x, y per vertex: 3 x 0.5 ulp), t is one rounding of T / det
      (0.5 ulp) and o + t d two more (1 ulp): 3 ulp per coordinate, sqrt(3) x 3 ulp as a length -- doubled for the three
      barycentrics' own rounding: 8 sqrt(3) 2^-17 / 2 ~ 5.3e-5 ... taken as 8 ulp = 6.1e-5;
      and the uv blend of render_mesh in fp32 (three products and two sums of numbers below 1: 4 x 2^-24 of the atlas, S texels wide, a
      texel being 1 / density long on the surface at least)."""
    return cpu.LINEAR_BOUND + grad * (8.0 * 2.0 ** -17 + 4.0 * 2.0 ** -24 * S / density)


def outside_rays(n, count, seed=2):
    """unit rays from a shell of radius 2 n at points of a ball of radius 0.3 (n - 1) around the centre of the n^3 sphere: every one hits"""
    rng = np.random.default_rng(seed)
    c = (n - 1) / 2.0
    u = rng.standard_normal((count, 3))
    o = c + 2.0 * n * u / np.linalg.norm(u, axis=1, keepdims=True)
    w = rng.standard_normal((count, 3))
    tgt = c + 0.3 * (n - 1) * rng.uniform(0, 1, (count, 1)) ** (1 / 3) * w / np.linalg.norm(w, axis=1, keepdims=True)
    d = tgt - o
    return o.astype(F32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def check_textured_render(v, f, atlas_fn, texels_fn, render_fn, n=33, density=2.0, rays=4096):
    """atlas, texel map (clamp 0), the linear colour c baked from tex_pos, then the mesh seen along `rays` outside rays: tex_colors equals
    c(points) within render_bound.  render_fn(o, d, uv, texture) -> dict of numpy arrays (mesh.render_mesh's)."""
    key = "sphere%d@device" % n
    cpu._cache[key] = (v, f, density, 7)
    try:
        uv, S, blocks, used = atlas_fn(v, f, density)
        assert used == density
        tf, tb, tp = texels_fn(v, f, blocks, S, 0)
        c = cpu.linear_colour(key)
        grad = float(np.linalg.norm(c(np.eye(3)) - c(np.zeros((1, 3))), axis=1).max())
        texture = np.where(tf[..., None] >= 0, c(tp), 0.0).astype(F32)
        o, d = outside_rays(n, rays)
        out = render_fn(o, d, uv, texture)
        hit = out["hit"]
        assert hit.all() and out["tex_colors"].shape == (rays, 3) and out["uv"].shape == (rays, 2)
        err = float(np.abs(out["tex_colors"].astype(np.float64) - c(out["points"])).max())
        bound = render_bound(S, density, grad)
        print("sphere %d^3: %d faces, atlas %d, %d rays: max |tex_colors - c(points)| = %.3g, bound %.3g" % (n, len(f), S, rays, err, bound))
        assert err <= bound, (err, bound)
        return uv, S, texture, out
    finally:
        del cpu._cache[key]


def test_render_mesh_with_a_texture(rt):
    """max |tex_colors - c(points)| on the 33^3 sphere (4096 rays): see the printed line; the bound is render_bound's"""
    from f2_nerf_amd import mesh
    h = rt.host()
    v, f = h.mesh_from_grid(_dev(mr.sphere_grid(33, 0.4 * 32)), 0.0, [0.0, 0.0, 0.0], 1.0)
    A = _atlas(h)

    def render(o, d, uv, texture):
        return {k: x.cpu().numpy() for k, x in mesh.render_mesh(v, f, _dev(o), _dev(d), uv=_dev(uv), texture=_dev(texture)).items()}

    uv, S, texture, out = check_textured_render(v.cpu().numpy(), f.cpu().numpy(), A.atlas, A.texels, render)
    # the two new outputs restated: the blend of the hit face's corner uv, and the lookup there
    want = (uv[out["face"]].astype(np.float64) * out["bary"][:, :, None]).sum(1)
    assert np.abs(out["uv"] - want).max() < 4 * 2.0 ** -24
    assert cpu.same(out["tex_colors"], ar.sample(texture, out["uv"]))
    # rows without a hit are zero; without the new arguments the dict is what it was
    o, d = outside_rays(33, 64)
    miss = mesh.render_mesh(v, f, _dev(o), _dev(-d), uv=_dev(uv), texture=_dev(texture))
    assert not miss["hit"].any() and (miss["uv"] == 0).all() and (miss["tex_colors"] == 0).all()
    assert set(mesh.render_mesh(v, f, _dev(o), _dev(d))) == {"hit", "t", "face", "bary", "points", "face_normals", "facing"}
    assert set(mesh.render_mesh(v, f, _dev(o), _dev(d), uv=_dev(uv))) == {"hit", "t", "face", "bary", "points", "face_normals", "facing"}
    none = mesh.render_mesh(v, f[:0], _dev(o), _dev(d), uv=_dev(uv[:0]), texture=_dev(texture))
    assert (none["uv"] == 0).all() and none["tex_colors"].shape == (64, 3) and (none["tex_colors"] == 0).all()


# ---- the fox scene -----------------------------------------------------------------------------------------------------------------
BOX = ([-1.0, -0.8, -0.9], [1.0, 0.7, 1.05])  # the box of tests/test_gpu_mesh_attrs.py::test_extract_mesh_attrs_on_the_fox


@pytest.fixture(scope="module")
def fox_runner(rt, fox_state):
    runner, cfg, arrays = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    return runner


def _fox_attrs(rt, runner, res=48, box=BOX, **kw):
    lo, hi = box
    g = runner.density_grid(lo, hi, res).cpu().numpy()
    level = float(np.quantile(g[g > 0], 0.5))  # a level the scene crosses
    return runner.extract_mesh_attrs(lo, hi, res, level, simplify=2, **kw), rt.host().grid_spec(lo, hi, res)[0]


def test_bake_texture_on_the_fox(rt, fox_runner):
    """At the faces' corner texels the texture is the vertex colour: the largest difference is printed; the bar is 1e-3, the project's RGB
    bar."""
    runner = fox_runner
    m, step = _fox_attrs(rt, runner)
    v, f, n, col = m["verts"], m["faces"], m["normals"], m["colors"].cpu().numpy()
    assert len(f) > 500
    density = float(F32(2.0) / F32(step))
    r = runner.bake_texture(v, f, n, density)
    assert set(r) == {"uv", "size", "texture", "tex_face", "density_used", "texels_used"} and r["density_used"] == density
    S, tex, tf, uv = r["size"], r["texture"].cpu().numpy(), r["tex_face"].cpu().numpy(), r["uv"].cpu().numpy()
    assert tex.shape == (S, S, 3) and tf.shape == (S, S) and uv.shape == (len(f), 3, 2) and r["texels_used"] == (tf >= 0).sum() > 0
    # the atlas is host.mesh_atlas's and the restatement's
    ruv, rS, lay, rd = ar.atlas(v.cpu().numpy(), f.cpu().numpy(), density)
    assert rS == S and cpu.same(ruv, uv) and cpu.same(ar.texels(v.cpu().numpy(), f.cpu().numpy(), lay["rot"], lay, 1)[0], tf)
    own = tf >= 0
    assert np.isfinite(tex).all() and tex[own].min() >= 0.0 and tex[own].max() <= 1.0 and (tex[~own] == 0).all() and tex[own].max() > 0
    t = np.round(uv.astype(np.float64) * S - 0.5).astype(np.int64)
    fn = f.cpu().numpy()
    worst, n_good = 0.0, 0
    for j in range(3):
        good = tf[t[:, j, 1], t[:, j, 0]] == np.arange(len(fn))  # (a degenerate face owns no texel)
        n_good += int(good.sum())
        worst = max(worst, float(np.abs(tex[t[good, j, 1], t[good, j, 0]] - col[fn[good, j]]).max()))
    print("fox 48^3 simplify=2: %d faces, atlas %d, %d texels used (fill %.3f); corner texels against the vertex colours: max %.3g" % (
        len(fn), S, r["texels_used"], r["texels_used"] / float(S * S), worst))
    assert n_good >= 0.95 * 3 * len(fn) and ((lay["rot"] & 4) == 0).sum() * 3 == n_good
    assert worst <= 1e-3, worst
    # twice the same; the fit loop reports the density it used
    again = runner.bake_texture(v, f, n, density)
    assert cpu.same(again["texture"].cpu().numpy(), tex)
    small = runner.bake_texture(v, f, n, density, max_size=S // 2)
    assert small["size"] <= S // 2 and small["density_used"] < density and small["density_used"] * 2 ** round(np.log2(density / small["density_used"])) == density
    with pytest.raises(ValueError):
        runner.bake_texture(v, f, n, density, max_size=1000)
    with pytest.raises(ValueError):
        runner.bake_texture(v, f, n, density, max_size=4)
    with pytest.raises(ValueError):
        runner.bake_texture(v, f, n, density, source="ray")  # (needs the grid step)
    with pytest.raises(ValueError):
        runner.bake_texture(v, f, n, density, source="mesh")
    # source="ray"
    ray = runner.bake_texture(v, f, n, density, source="ray", step=step)
    rt_, rf = ray["texture"].cpu().numpy(), ray["tex_face"].cpu().numpy()
    assert (rf == tf).all() and np.isfinite(rt_).all() and rt_[own].min() >= 0.0 and rt_[own].max() <= 1.0 and (rt_[~own] == 0).all()
    print("source=ray: mean colour %.4f against %.4f of source=point" % (rt_[own].mean(), tex[own].mean()))


def test_baking_has_no_effect_on_training(rt, fox_state):
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 4096, rng)) for _ in range(6)]

    def run(bake):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=15"], seed=3, table_init=0.3)
        runner.n_edge_pts = 512
        losses = []
        for k, b in enumerate(batches):
            if bake and k == 3:
                m, step = _fox_attrs(rt, runner, 32, ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]), colors=False)
                for source in ("point", "ray"):
                    r = runner.bake_texture(m["verts"], m["faces"], m["normals"], 2.0 / step, source=source, step=step)
                    assert r["texels_used"] > 0 and torch.isfinite(r["texture"]).all()
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [x.detach().cpu().numpy().copy() for x in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))


def test_launcher_writes_the_texture(tmp_path, monkeypatch, capsys):
    """The synthetic rig of tests/test_gpu_mesh_raycast.py's launcher test: mesh.texture=true mesh.simplify=2 mesh.check=true at resolution
    48 writes _tex.obj, _tex.mtl and _tex.png and adds texture_psnr to the check; the .ply and every earlier key of the JSON are those of
    a run without the option, which writes no _tex file."""
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
    ex = common + ["mode=extract_mesh", "is_continue=true", "mesh.resolution=48", "mesh.simplify=2", "mesh.check=true", "check.res_level=2",
                   "check.tau=0.0001", "check.min_opacity=0.0001", "check.max_views=5"]
    name = "60_48_s2"
    capsys.readouterr()
    assert run.main(ex) == 0
    plain_out = capsys.readouterr().out
    ply, before = open(meshes / (name + ".ply"), "rb").read(), json.load(open(meshes / (name + "_check.json")))
    assert not [p for p in os.listdir(meshes) if "_tex" in p] and "Texture:" not in plain_out and "texture_psnr" not in before
    assert run.main(ex + ["mesh.texture=true"]) == 0
    out = capsys.readouterr().out
    assert open(meshes / (name + ".ply"), "rb").read() == ply
    after = json.load(open(meshes / (name + "_check.json")))
    assert set(after) == set(before) | {"texture_psnr", "n_texture_rays"} and all(after[k] == before[k] for k in before)
    assert np.isfinite(after["texture_psnr"]) and after["n_texture_rays"] == after["n_both"]
    line = [ln for ln in out.split("\n") if ln.startswith("Texture:")]
    assert len(line) == 1 and all(w in line[0] for w in ("atlas", "texels used", "texels per unit", name + "_tex.obj")) and "halved" not in line[0]
    keep = lambda text: [ln for ln in text.split("\n") if ln.startswith(("Mesh:", "Check:"))]  # noqa: E731
    assert keep(out) == keep(plain_out)
    with capsys.disabled():
        print(line[0], "texture_psnr %.2f over %d rays" % (after["texture_psnr"], after["n_texture_rays"]))
    o = cpu.parse_obj(str(meshes / (name + "_tex.obj")))
    import test_mesh_cpu
    pv, pf = test_mesh_cpu.read_ply(str(meshes / (name + ".ply")))
    assert cpu.same(np.array(o["v"], F32), pv) and (np.array(o["f"])[:, :, 0] - 1 == pf).all() and len(o["vt"]) == 3 * len(pf) and len(o["vn"]) == len(pv)
    assert o["mtllib"] == name + "_tex.mtl" and ("map_Kd %s_tex.png" % name) in open(meshes / (name + "_tex.mtl")).read()
    img = np.asarray(Image.open(meshes / (name + "_tex.png")))
    assert img.ndim == 3 and img.shape[0] == img.shape[1] and img.shape[2] == 3 and img.dtype == np.uint8 and img.max() > 0
    assert (cpu.decode_png(open(meshes / (name + "_tex.png"), "rb").read()) == img).all()
    vt = np.array(o["vt"], F32)
    assert vt.min() > 0 and vt.max() < 1
    # a smaller atlas: the line says that the density was halved; the TSDF source and the ray source run
    assert run.main(ex + ["mesh.texture=true", "texture.max_size=%d" % (img.shape[0] // 2), "texture.source=ray"]) == 0
    line = [ln for ln in capsys.readouterr().out.split("\n") if ln.startswith("Texture:")]
    assert len(line) == 1 and "halved" in line[0] and "source ray" in line[0]
    assert np.asarray(Image.open(meshes / (name + "_tex.png"))).shape[0] <= img.shape[0] // 2
    tsdf = common + ["mode=extract_mesh", "is_continue=true", "mesh.resolution=24", "mesh.source=tsdf", "tsdf.res_level=2", "tsdf.tau=0.0001",
                     "tsdf.min_opacity=0.0001", "tsdf.min_weight=0.0001", "mesh.texture=true"]
    assert run.main(tsdf) == 0
    assert all((meshes / ("60_24_tsdf_tex" + ext)).exists() for ext in (".obj", ".mtl", ".png"))
    with pytest.raises(ValueError):
        run.main(ex + ["mesh.texture=true", "texture.max_size=1000"])
    with pytest.raises(ValueError):
        run.main(ex + ["mesh.texture=true", "texture.source=mesh"])
