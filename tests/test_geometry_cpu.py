"""Render geometry buffers without a GPU: f2n_composite_geometry (csrc/render.hip) under the wavefront emulator (tests/wave_emul) against
f2n_density_grad_scatter (the per-sample half: bit for bit, one shared device function) and against the float32 restatement of
tests/geometry_ref.py (the per-ray half: bit for bit, both builds use -ffp-contract=off); the point-cloud PLY writer and the launcher's
points.* options."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import geometry_ref as gr  # noqa: E402

F32 = np.float32
INVALID = -1  # F2N_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def emul_geometry(L, c, want_grad=True, want_normal=True, tau=None):
    R, M = len(c["se"]), len(c["t"])
    out = dict(opacity=np.full(R, np.nan, F32), normals=np.full((R, 3), np.nan, F32), surf_idx=np.full(R, -7, np.int32),
               surf_t=np.full(R, np.nan, F32), surf_points=np.full((R, 3), np.nan, F32), surf_normals=np.full((R, 3), np.nan, F32),
               sample_grad=np.full((M, 3), np.nan, F32) if want_grad else None,
               sample_normals=np.full((M, 3), np.nan, F32) if want_normal else None)
    rc = L.f2n_composite_geometry(None, R, _vp(c["se"]), _vp(c["weights"]), _vp(c["t"]), _vp(c["rays_o"]), _vp(c["rays_d"]), _vp(c["anchors"]),
                                  _vp(c["transes"]), _vp(c["df0_dw"]), ctypes.c_float(c["tau"] if tau is None else tau), _vp(out["opacity"]),
                                  _vp(out["normals"]), _vp(out["surf_idx"]), _vp(out["surf_t"]), _vp(out["surf_points"]),
                                  _vp(out["surf_normals"]), _vp(out["sample_grad"]), _vp(out["sample_normals"]))
    assert rc == 0, rc
    return out


def emul_scatter(L, c):
    """f2n_density_grad_scatter on the samples' world points with f0 = 3: density exactly 1, grad = J^T df0_dw."""
    M = len(c["t"])
    x = gr.world_points(c["rays_o"], c["rays_d"], c["t"], c["se"])
    se = np.stack([np.arange(M), np.arange(M) + 1], 1).astype(np.int32)
    f0 = np.full(M, 3.0, F32)
    dens, grad, nrm = np.full(M, np.nan, F32), np.full((M, 3), np.nan, F32), np.full((M, 3), np.nan, F32)
    assert L.f2n_density_grad_scatter(None, M, _vp(x), _vp(c["anchors"]), _vp(se), _vp(c["transes"]), _vp(f0), _vp(c["df0_dw"]), _vp(dens),
                                      _vp(grad), _vp(nrm)) == 0
    assert (dens == 1).all()
    return dens, grad, nrm


def check_case(c, out, scatter):
    """The checks both the emulated and the GPU run of the entry point make (tests/test_gpu_geometry.py calls this as well)."""
    dens, grad, nrm = scatter
    with np.errstate(invalid="ignore"):
        assert gr.same_bits((out["sample_grad"] * dens[:, None]).astype(F32), grad)
    assert gr.same_bits(out["sample_normals"], nrm)
    ln = np.sqrt((out["sample_normals"].astype(np.float64) ** 2).sum(1))
    assert ((np.abs(ln - 1) < 1e-6) | (ln == 0)).all()
    ref = gr.ray_buffers(c["se"], c["weights"], c["t"], c["rays_o"], c["rays_d"], out["sample_normals"], c["tau"])
    assert (out["surf_idx"] == ref["surf_idx"]).all()
    for k in ("opacity", "normals", "surf_t", "surf_points", "surf_normals"):
        assert gr.same_bits(out[k], ref[k]), k
    empty = c["se"][:, 0] == c["se"][:, 1]
    none = out["surf_idx"] < 0
    assert (none[empty]).all() and (out["opacity"][empty] == 0).all() and (out["normals"][empty] == 0).all()
    for k in ("surf_t", "surf_points", "surf_normals"):
        assert (out[k][none] == 0).all() and not np.signbit(out[k][none]).any(), k
    return ref


def test_composite_geometry_on_the_emulator(emul, fox_state):
    c = gr.synthetic_case(fox_state["pers_trans"], n_rays=37, seed=5)
    se, w = c["se"], c["weights"]
    assert tuple(se[:7, 1] - se[:7, 0]) == gr.LENGTHS and len(se) % 16 != 0
    out = emul_geometry(emul, c)
    ref = check_case(c, out, emul_scatter(emul, c))
    # the special rays do what they were built for
    assert out["surf_idx"][0] == -1 and out["surf_idx"][7] == -1 and 0 < out["opacity"][7] < c["tau"]
    assert out["surf_idx"][8] == se[8, 0]
    incl = np.cumsum(w[se[9, 0]:se[9, 1]], dtype=F32)
    assert incl[2] == F32(c["tau"]) and incl[1] < c["tau"] and out["surf_idx"][9] == se[9, 0] + 2
    s = se[10, 0]
    assert (out["sample_normals"][s + 3] == 0).all() and (out["sample_grad"][s + 3] == 0).all()
    assert (out["sample_normals"][s + 17] == 0).all() and not np.isfinite(out["sample_grad"][s + 17]).all()
    assert len(np.unique(c["anchors"][se[11, 0]:se[11, 1], 0])) >= 3
    assert (out["surf_idx"] >= 0).sum() >= 8 and (out["surf_idx"] < 0).sum() >= 3
    assert np.isfinite(out["normals"]).all() and (np.abs(np.linalg.norm(out["normals"][~(out["normals"] == 0).all(1)], axis=1) - 1) < 1e-6).all()
    hit = out["surf_idx"] >= 0
    x = gr.world_points(c["rays_o"], c["rays_d"], c["t"], se)
    assert gr.same_bits(out["surf_points"][hit], x[out["surf_idx"][hit]])
    # NULL optional outputs change nothing; a second call gives the same bits
    for kw in (dict(want_grad=False), dict(want_normal=False), dict(want_grad=False, want_normal=False), dict()):
        o2 = emul_geometry(emul, c, **kw)
        for k, v in out.items():
            if o2[k] is not None:
                assert gr.same_bits(o2[k], v), (kw, k)
    # another threshold moves the surface, not the sums; tau = 1 is allowed
    o3 = emul_geometry(emul, c, tau=1.0)
    assert gr.same_bits(o3["opacity"], out["opacity"]) and gr.same_bits(o3["normals"], out["normals"])
    ref3 = gr.ray_buffers(se, w, c["t"], c["rays_o"], c["rays_d"], out["sample_normals"], 1.0)
    assert (o3["surf_idx"] == ref3["surf_idx"]).all() and (ref3["surf_idx"] != ref["surf_idx"]).any()


def test_error_codes_and_no_rays(emul, fox_state):
    c = gr.synthetic_case(fox_state["pers_trans"], n_rays=12, seed=6, max_len=20)
    R = len(c["se"])
    o = dict(opacity=np.full(R, 7, F32), normals=np.full((R, 3), 7, F32), surf_idx=np.full(R, 7, np.int32), surf_t=np.full(R, 7, F32),
             surf_points=np.full((R, 3), 7, F32), surf_normals=np.full((R, 3), 7, F32))

    def call(n, tau, **repl):
        a = dict(se=c["se"], weights=c["weights"], t=c["t"], rays_o=c["rays_o"], rays_d=c["rays_d"], anchors=c["anchors"], transes=c["transes"],
                 df0_dw=c["df0_dw"], **o)
        a.update(repl)
        return emul.f2n_composite_geometry(None, n, _vp(a["se"]), _vp(a["weights"]), _vp(a["t"]), _vp(a["rays_o"]), _vp(a["rays_d"]),
                                           _vp(a["anchors"]), _vp(a["transes"]), _vp(a["df0_dw"]), ctypes.c_float(tau), _vp(a["opacity"]),
                                           _vp(a["normals"]), _vp(a["surf_idx"]), _vp(a["surf_t"]), _vp(a["surf_points"]),
                                           _vp(a["surf_normals"]), None, None)

    assert call(-1, 0.5) == INVALID
    for tau in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        assert call(R, tau) == INVALID, tau
    for k in ("se", "weights", "t", "rays_o", "rays_d", "anchors", "transes", "df0_dw", "opacity", "normals", "surf_idx", "surf_t",
              "surf_points", "surf_normals"):
        assert call(R, 0.5, **{k: None}) == INVALID, k
    assert call(0, 0.5) == 0
    assert all((v == 7).all() for v in o.values())  # nothing was written by any of the calls above
    assert emul.f2n_composite_geometry(None, 0, *([None] * 8), ctypes.c_float(0.5), *([None] * 8)) == 0
    assert call(R, 0.5) == 0 and (o["surf_idx"] != 7).all()


def _read_ply(path):
    with open(path, "rb") as f:
        raw = f.read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    n = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
    dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[ty]) for ty, name in props])
    return lines, np.frombuffer(body, dt, n), body[n * dt.itemsize:]


def test_write_points_ply_round_trips(tmp_path):
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    rng = np.random.default_rng(2)
    p = rng.standard_normal((11, 3)).astype(F32)
    nr = rng.standard_normal((11, 3)).astype(F32)
    col = rng.uniform(-0.2, 1.2, (11, 3)).astype(F32)
    for normals, colors in ((None, None), (nr, None), (None, col), (nr, col)):
        lines, v, rest = _read_ply(mesh.write_points_ply(str(tmp_path / "sub" / "p.ply"), p, normals, colors))
        assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and rest == b"" and not any("face" in ln for ln in lines)
        assert (np.stack([v["x"], v["y"], v["z"]], 1) == p).all()
        assert ("nx" in v.dtype.names) == (normals is not None) and ("red" in v.dtype.names) == (colors is not None)
        if normals is not None:
            assert (np.stack([v["nx"], v["ny"], v["nz"]], 1) == nr).all()
        if colors is not None:
            assert (np.stack([v["red"], v["green"], v["blue"]], 1) == mesh.quantize_colors(col)).all()
    lines, v, rest = _read_ply(mesh.write_points_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), F32), np.zeros((0, 3), F32)))
    assert len(v) == 0 and rest == b""
    with pytest.raises(ValueError):
        mesh.write_points_ply(str(tmp_path / "bad.ply"), p, nr[:5])


def test_write_ply_bytes_are_unchanged(tmp_path):
    """A fixed mesh: the file write_ply wrote before the point-cloud writer existed, byte for byte (header spelled out here)."""
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]], F32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    nr = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1]], F32)
    col = np.array([[0, 0.5, 1], [1.2, -1, 0.25], [0.1, 0.2, 0.3], [1, 1, 1]], F32)
    faces = b"".join(b"\x03" + np.asarray(r, "<i4").tobytes() for r in f)
    tail = "element face 2\nproperty list uchar int vertex_indices\nend_header\n"
    plain = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n" + tail).encode() + \
        v.astype("<f4").tobytes() + faces
    assert open(mesh.write_ply(str(tmp_path / "a.ply"), v, f), "rb").read() == plain
    q = np.array([[0, 127, 255], [255, 0, 63], [25, 51, 76], [255, 255, 255]], np.uint8)
    assert (mesh.quantize_colors(col) == q).all()
    full = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n" + tail).encode() + \
        b"".join(v[i].astype("<f4").tobytes() + nr[i].astype("<f4").tobytes() + q[i].tobytes() for i in range(4)) + faces
    assert open(mesh.write_ply(str(tmp_path / "b.ply"), v, f, nr, col), "rb").read() == full


def test_points_options_parse_and_default():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    o = mesh.points_options(config.preset("wanjinyou", []))
    assert o == {"res_level": 4, "min_opacity": 0.5, "tau": 0.5, "normals": "surface", "max_points": 2000000}
    o = mesh.points_options(config.preset("wanjinyou", ["points.res_level=2", "points.min_opacity=0.25", "points.normals=composited",
                                                         "points.max_points=1000", "points.tau=0.75"]))
    assert o == {"res_level": 2, "min_opacity": 0.25, "tau": 0.75, "normals": "composited", "max_points": 1000}
    for bad in ("field", "Surface normals", "true", ""):
        with pytest.raises(ValueError) as e:
            mesh.points_options(config.preset("wanjinyou", ["points.normals=%s" % bad]))
        assert "surface" in str(e.value) and "composited" in str(e.value)
    for bad in ("points.res_level=0", "points.max_points=0", "points.tau=0", "points.tau=1.5"):
        with pytest.raises(ValueError):
            mesh.points_options(config.preset("wanjinyou", [bad]))
    # the fixed stride that caps the cloud: no random draw, never more than max_points, everything when it fits
    assert (mesh.stride_subset(10, 10) == np.arange(10)).all() and (mesh.stride_subset(10, 100) == np.arange(10)).all()
    for n, cap in ((11, 10), (1000, 7), (2000001, 2000000), (5, 1)):
        idx = mesh.stride_subset(n, cap)
        assert cap // 2 <= len(idx) <= cap and idx[0] == 0 and len(set(np.diff(idx).tolist())) <= 1
        assert idx.max() < n
