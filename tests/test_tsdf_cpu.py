"""TSDF fusion without a GPU: f2n_tsdf_integrate (csrc/dataset.hip), f2n_tsdf_finalize and f2n_mesh_count_masked (csrc/octree.hip) under
the wavefront emulator (tests/wave_emul) against the float32 restatement of tests/tsdf_ref.py, bit for bit (both builds use
-ffp-contract=off); the algorithm's known answer on analytic depth maps of a sphere (restatement alone); the tsdf.* / mesh.source options."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import mesh_ref as mr  # noqa: E402
import tsdf_ref as tr  # noqa: E402

F32 = np.float32
INVALID = -1  # F2N_ERR_INVALID_ARG
_f, _i = ctypes.c_float, ctypes.c_int


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _lo3(lo):
    return (_f * 3)(*(float(v) for v in lo))


def emul_integrate(L, c, S, W, v0=0, v1=None, conf="case"):
    """f2n_tsdf_integrate of the views [v0, v1) of case c into S, W (host arrays, in place)."""
    v1 = len(c["depth"]) if v1 is None else v1
    cf = c["conf"] if isinstance(conf, str) else conf
    a = [np.ascontiguousarray(c[k][v0:v1], F32) for k in ("poses", "intri", "dist", "depth")] + [None if cf is None else np.ascontiguousarray(cf[v0:v1], F32)]
    return L.f2n_tsdf_integrate(None, _lo3(c["lo"]), _f(c["step"]), _i(c["nx"]), _i(c["ny"]), _i(c["nz"]), _i(v1 - v0), *(_vp(x) for x in a),
                                _i(c["h"]), _i(c["w"]), _f(c["trunc"]), _vp(S), _vp(W))


def emul_finalize(L, S, W, min_weight):
    g, valid = np.full(S.shape, np.nan, F32), np.full(S.shape, 7, np.uint8)
    assert L.f2n_tsdf_finalize(None, ctypes.c_int64(S.size), _vp(S), _vp(W), _f(min_weight), _vp(g), _vp(valid)) == 0
    return g, valid


def emul_mesh(L, g, valid, level, lo=(0.0, 0.0, 0.0), step=1.0):
    """f2n_mesh_count (valid None) or f2n_mesh_count_masked, then f2n_mesh_emit: every output."""
    g = np.ascontiguousarray(g, F32)
    nz, ny, nx = g.shape
    n, c = nx * ny * nz, (nx - 1) * (ny - 1) * (nz - 1)
    o = dict(edge_mask=np.full(n, 255, np.uint8), vc=np.full(n, -7, np.int32), vse=np.full((n, 2), -7, np.int32), fc=np.full(c, -7, np.int32),
             fse=np.full((c, 2), -7, np.int32), totals=np.full(2, -7, np.int32))
    outs = [_vp(o[k]) for k in ("edge_mask", "vc", "vse", "fc", "fse", "totals")]
    if valid is None:
        assert L.f2n_mesh_count(None, nx, ny, nz, _vp(g), _f(level), *outs) == 0
    else:
        assert L.f2n_mesh_count_masked(None, nx, ny, nz, _vp(g), _f(level), _vp(np.ascontiguousarray(valid, np.uint8)), *outs) == 0
    nv, nf = (int(v) for v in o["totals"])
    o["verts"], o["faces"] = np.full((nv, 3), np.nan, F32), np.full((nf, 3), -7, np.int32)
    if nv or nf:
        assert L.f2n_mesh_emit(None, nx, ny, nz, _vp(g), _f(level), _lo3(lo), _f(step), _vp(o["edge_mask"]), _vp(o["vse"]), _vp(o["fse"]),
                               _vp(o["verts"]), _vp(o["faces"])) == 0
    return o


def check_integrate(c, integrate, finalize):
    """The identities of f2n_tsdf_integrate / f2n_tsdf_finalize on case c; integrate(c, S, W, v0, v1, conf) updates host arrays in place
    (the emulator here, the device in tests/test_gpu_tsdf.py)."""
    shape = (c["nz"], c["ny"], c["nx"])
    V = len(c["depth"])
    rng = np.random.default_rng(1)
    S0, W0 = rng.standard_normal(shape).astype(F32), rng.uniform(0, 2, shape).astype(F32)  # a state that is not zero
    for s0, w0 in ((np.zeros(shape, F32), np.zeros(shape, F32)), (S0, W0)):
        stats = {}
        rs, rw = tr.integrate(s0, w0, c["lo"], c["step"], c["nx"], c["ny"], c["nz"], c["poses"], c["intri"], c["dist"], c["depth"], c["conf"],
                              c["trunc"], stats)
        S, W = s0.copy(), w0.copy()
        integrate(c, S, W, 0, V, "case")
        assert tr.same_bits(S, rs) and tr.same_bits(W, rw)
        S2, W2 = s0.copy(), w0.copy()  # in two batches: the same bits
        integrate(c, S2, W2, 0, 2, "case")
        assert not tr.same_bits(W2, W)
        integrate(c, S2, W2, 2, V, "case")
        assert tr.same_bits(S2, S) and tr.same_bits(W2, W)
        S3, W3 = s0.copy(), w0.copy()  # a second call on fresh state
        integrate(c, S3, W3, 0, V, "case")
        assert tr.same_bits(S3, S) and tr.same_bits(W3, W)
    # the case does what it was built for: every exit of the twelve steps is taken
    assert all(stats[k] > 0 for k in ("behind", "outside", "no_depth", "far_behind", "used")), stats
    assert stats["at_minus_trunc"] >= 3 and stats["clamped"] >= 3, stats
    assert (stats["no_conf"] > 0) == (c["conf"] is not None)
    for mw in (0.0, 2.5, 1.0):
        g, valid = finalize(S, W, mw)
        rg, rv = tr.finalize(rs, rw, mw)
        assert tr.same_bits(g, rg) and tr.same_bits(valid, rv)
    assert 0 < rv.mean() < 1 and (rg[rv != 0] > 0).any() and (rg[rv != 0] < 0).any() and (rg[rv == 0] == 0).all()
    # NULL conf is conf == 1
    Sa, Wa, Sb, Wb = (np.zeros(shape, F32) for _ in range(4))
    integrate(c, Sa, Wa, 0, V, None)
    integrate(c, Sb, Wb, 0, V, np.ones_like(c["depth"]))
    assert tr.same_bits(Sa, Sb) and tr.same_bits(Wa, Wb) and (Wa == np.round(Wa)).all() and Wa.max() >= 2
    # no views: the state is not touched
    Sp, Wp = np.full(shape, 7, F32), np.full(shape, np.nan, F32)
    integrate(c, Sp, Wp, 2, 2, "case")
    assert (Sp == 7).all() and np.isnan(Wp).all()
    return S, W


def _emul_checked(L):
    def integrate(c, S, W, v0, v1, conf):
        assert emul_integrate(L, c, S, W, v0, v1, conf) == 0
    return integrate, lambda S, W, mw: emul_finalize(L, S, W, mw)


@pytest.mark.parametrize("with_conf", [True, False])
def test_integrate_and_finalize_on_the_emulator(emul, fox_state, with_conf):
    c = tr.synthetic_case(fox_state, with_conf=with_conf)
    assert (c["nx"], c["ny"], c["nz"]) == (37, 21, 19) and c["depth"].shape == (5, 61, 45)
    d = c["depth"]
    assert (d == 0).any() and (d < 0).any() and np.isnan(d).any() and np.isposinf(d).any()
    check_integrate(c, *_emul_checked(emul))


def test_error_codes(emul, fox_state):
    c = tr.synthetic_case(fox_state, dims=(9, 7, 5))
    shape = (c["nz"], c["ny"], c["nx"])
    S, W = np.full(shape, 7, F32), np.full(shape, 7, F32)

    def call(**repl):
        a = dict(lo=_lo3(c["lo"]), step=c["step"], nx=c["nx"], ny=c["ny"], nz=c["nz"], V=len(c["depth"]), poses=c["poses"], intri=c["intri"],
                 dist=c["dist"], depth=c["depth"], conf=c["conf"], h=c["h"], w=c["w"], trunc=c["trunc"], S=S, W=W)
        a.update(repl)
        return emul.f2n_tsdf_integrate(None, a["lo"], _f(a["step"]), _i(a["nx"]), _i(a["ny"]), _i(a["nz"]), _i(a["V"]), _vp(a["poses"]),
                                       _vp(a["intri"]), _vp(a["dist"]), _vp(a["depth"]), _vp(a["conf"]), _i(a["h"]), _i(a["w"]), _f(a["trunc"]),
                                       _vp(a["S"]), _vp(a["W"]))

    for trunc in (0.0, -0.5, float("nan"), float("inf")):
        assert call(trunc=trunc) == INVALID, trunc
    for k in ("nx", "ny", "nz", "V", "h", "w"):
        assert call(**{k: -1}) == INVALID, k
    assert call(h=0) == INVALID and call(w=0) == INVALID and call(h=(1 << 24) + 1) == INVALID
    for k in ("lo", "poses", "intri", "dist", "depth", "S", "W"):
        assert call(**{k: None}) == INVALID, k
    assert call(V=0) == 0 and call(nz=0) == 0 and call(V=0, poses=None, depth=None, S=None, W=None) == 0
    assert (S == 7).all() and (W == 7).all()  # nothing was written by any of the calls above
    assert call() == 0 and (W != 7).any()
    g, valid = np.full(shape, 7, F32), np.full(shape, 7, np.uint8)
    fin = lambda n, s, w, mw, og, ov: emul.f2n_tsdf_finalize(None, ctypes.c_int64(n), _vp(s), _vp(w), _f(mw), _vp(og), _vp(ov))  # noqa: E731
    assert fin(-1, S, W, 1.0, g, valid) == INVALID and fin(S.size, S, W, float("nan"), g, valid) == INVALID
    for k in range(4):
        args = [S, W, g, valid]
        args[k] = None
        assert fin(S.size, args[0], args[1], 1.0, args[2], args[3]) == INVALID
    assert fin(0, None, None, 1.0, None, None) == 0 and (g == 7).all() and (valid == 7).all()
    gr = np.zeros((3, 3, 3), F32)
    outs = [np.zeros(27, np.uint8), np.zeros(27, np.int32), np.zeros((27, 2), np.int32), np.zeros(8, np.int32), np.zeros((8, 2), np.int32), np.zeros(2, np.int32)]
    assert emul.f2n_mesh_count_masked(None, 3, 3, 3, _vp(gr), _f(0.0), None, *(_vp(o) for o in outs)) == INVALID
    assert emul.f2n_mesh_count_masked(None, 3, 3, 1, _vp(gr), _f(0.0), _vp(np.ones(27, np.uint8)), *(_vp(o) for o in outs)) == INVALID
    assert emul.f2n_mesh_count_masked(None, 3, 3, 3, _vp(gr), _f(0.0), _vp(np.ones(27, np.uint8)), *(_vp(o) for o in outs)) == 0


def mask_cases(shape=(7, 8, 9), seed=4):
    """(grid [nz, ny, nx], level, lo, step) and the masks the masked mesher is held to: all ones, random, a half space."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(shape).astype(F32)
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return g, 0.1, (0.5, -1.0, 2.0), 0.25, {"ones": np.ones(shape, np.uint8), "random": (rng.uniform(size=shape) < 0.8).astype(np.uint8),
                                              "half": (x + 2 * y - z < 12).astype(np.uint8) * 3}


def check_masked_mesher(mesh_fn, count_fn=None):
    """mesh_fn(g, valid or None, level, lo, step) -> dict with verts, faces (and, where count_fn is None, every output of the count
    entry points): the checks the emulated and the device run share."""
    g, level, lo, step, masks = mask_cases()
    assert g.shape == (7, 8, 9)
    plain = mesh_fn(g, None, level, lo, step)
    ones = mesh_fn(g, masks["ones"], level, lo, step)
    for k, v in plain.items():  # valid all ones: every output of f2n_mesh_count, bit for bit
        assert tr.same_bits(ones[k], v), k
    rv, rf = mr.marching_tets(g, level, lo, step)
    assert len(rf) > 100 and tr.same_bits(ones["verts"], rv) and (ones["faces"] == rf).all()
    for name in ("random", "half"):
        valid = masks[name]
        o = mesh_fn(g, valid, level, lo, step)
        v, f, keys, cells, edge_mask = tr.marching_tets_masked(g, level, valid, lo, step)
        assert 0 < len(f) < len(rf) and 0 < len(v) < len(rv)
        assert tr.same_bits(o["verts"], v) and (o["faces"] == f).all(), name
        if "edge_mask" in o:
            assert (o["edge_mask"] == edge_mask).all() and o["totals"].tolist() == [len(v), len(f)]
            assert (o["fc"] == np.bincount(cells, minlength=len(o["fc"]))).all()
            assert ((o["edge_mask"] & ~plain["edge_mask"]) == 0).all() and (o["fc"] <= plain["fc"]).all()
        tr.check_masked_mesh(o["verts"], o["faces"], g, level, valid, lo, step)
        assert 1 in set(mr.edge_face_counts(o["faces"]).values())  # open where observation ends


def test_masked_mesher_on_the_emulator(emul):
    check_masked_mesher(lambda g, valid, level, lo, step: emul_mesh(emul, g, valid, level, lo, step))


def sphere_case(st, n=48):
    """The known-answer case: the fox training cameras, analytic depth maps of a sphere of radius 0.15 around the point their optical axes
    meet, at 1/8 of the resolution, conf = 1 where the ray meets the sphere at a cosine >= 0.5; a grid of n^3 points over centre +- 0.25."""
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    ts = np.asarray(st["train_set"])
    centre = tr.axes_focus(st["poses"][ts])
    assert np.abs(centre - np.array([0.7326, 0.1673, 0.7898])).max() < 1e-3
    H, Wd = (int(v) for v in st["image_hw"])
    h, w = H // 8, Wd // 8
    intri = mesh.tsdf_intrinsics(st["intri"][ts], 8)
    depth, conf = tr.sphere_depth_maps(st["poses"][ts], intri, st["dist_params"][ts], h, w, centre, 0.15, 0.5)
    step = F32(0.5 / (n - 1))
    return dict(lo=(centre - 0.25).astype(F32), step=step, nx=n, ny=n, nz=n, poses=np.ascontiguousarray(st["poses"][ts], F32), intri=intri,
                dist=np.ascontiguousarray(st["dist_params"][ts], F32), depth=depth, conf=conf, trunc=F32(3) * step, h=h, w=w), centre


def test_fused_sphere_lies_within_a_voxel_of_the_sphere(fox_state):
    """The algorithm's known answer, on the restatement alone: every vertex of the fused mesh within ONE grid step of the sphere, the mesh
    not empty and open (no camera sees the sphere's back).  A float64 prototype of this case gave 0.52 step at most (median 0.07) on the
    axis edges at 48^3."""
    c, centre = sphere_case(fox_state, 48)
    assert (c["conf"] > 0).any(axis=(1, 2)).all() and c["depth"].shape[1:] == (120, 67)
    z = np.zeros((48, 48, 48), F32)
    S, W = tr.integrate(z, z, c["lo"], c["step"], 48, 48, 48, c["poses"], c["intri"], c["dist"], c["depth"], c["conf"], c["trunc"])
    g, valid = tr.finalize(S, W, 1.0)
    v, f, _, _, _ = tr.marching_tets_masked(g, 0.0, valid, c["lo"], c["step"])
    err = np.abs(np.linalg.norm(v.astype(np.float64) - centre[None], axis=1) - 0.15) / float(c["step"])
    print("%d vertices, %d faces; distance to the sphere in steps: max %.3f, median %.3f; %d of %d grid points known" % (
        len(v), len(f), err.max(), np.median(err), int(valid.sum()), valid.size))
    assert len(f) > 1000
    tr.check_masked_mesh(v, f, g, 0.0, valid, c["lo"], c["step"])
    assert 1 in set(mr.edge_face_counts(f).values())  # open
    assert err.max() <= 1.0, err.max()


def test_options_parse_and_default():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    assert mesh.options(config.preset("wanjinyou", []))["source"] == "density"
    assert mesh.options(config.preset("wanjinyou", ["mesh.source=tsdf"]))["source"] == "tsdf"
    assert mesh.options(config.preset("wanjinyou", ["mesh.source=TSDF "]))["source"] == "tsdf"
    for bad in ("sdf", "true", "", "density tsdf"):
        with pytest.raises(ValueError) as e:
            mesh.options(config.preset("wanjinyou", ["mesh.source=%s" % bad]))
        assert "density" in str(e.value) and "tsdf" in str(e.value)
    o = mesh.tsdf_options(config.preset("wanjinyou", []))
    assert o == {"res_level": 4, "trunc_voxels": 4.0, "tau": 0.5, "min_opacity": 0.5, "min_weight": 1.0, "views_per_batch": 8, "max_views": 0}
    o = mesh.tsdf_options(config.preset("wanjinyou", ["tsdf.res_level=8", "tsdf.trunc_voxels=2.5", "tsdf.tau=0.25", "tsdf.min_opacity=0.1",
                                                       "tsdf.min_weight=3", "tsdf.views_per_batch=3", "tsdf.max_views=4"]))
    assert o == {"res_level": 8, "trunc_voxels": 2.5, "tau": 0.25, "min_opacity": 0.1, "min_weight": 3.0, "views_per_batch": 3, "max_views": 4}
    for bad in ("tsdf.res_level=0", "tsdf.views_per_batch=0", "tsdf.max_views=-1", "tsdf.tau=0", "tsdf.tau=1.5", "tsdf.trunc_voxels=0",
                "tsdf.trunc_voxels=-1", "tsdf.min_weight=-1", "tsdf.min_opacity=-0.5"):
        with pytest.raises(ValueError):
            mesh.tsdf_options(config.preset("wanjinyou", [bad]))
    assert "tsdf" not in config.GROUP_DEFAULTS
    k = mesh.tsdf_intrinsics(np.array([[[8.0, 0, 4.0], [0, 6.0, 2.0], [0, 0, 1.0]]]), 4)
    assert k.dtype == F32 and k.tolist() == [[[2.0, 0, 1.0], [0, 1.5, 0.5], [0, 0, 1.0]]]


def test_a_density_export_writes_the_bytes_it_wrote_before(tmp_path):
    """mesh.source defaults to density: extract() asks the runner for the density mesh alone and writes <iter>_<res>.ply with the bytes
    write_ply always wrote (the header is spelled out here); a TSDF export without a data set is refused before anything is rendered."""
    import torch
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]], F32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)

    class Runner:
        iter_step = 60
        calls = []

        def extract_mesh(self, lo, hi, res, level):
            self.calls.append((lo, hi, res, level))
            return torch.from_numpy(v), torch.from_numpy(f)

    scene = {"center": np.zeros(3, F32), "radius": 1.0}
    r = Runner()
    path = mesh.extract(r, config.preset("wanjinyou", ["mesh.resolution=16"]), scene, str(tmp_path))
    assert path == os.path.join(str(tmp_path), "meshes", "60_16.ply") and r.calls == [([-1.0] * 3, [1.0] * 3, 16, mesh.DEFAULT_LEVEL)]
    faces = b"".join(b"\x03" + np.asarray(row, "<i4").tobytes() for row in f)
    plain = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
             "element face 2\nproperty list uchar int vertex_indices\nend_header\n").encode() + v.astype("<f4").tobytes() + faces
    assert open(path, "rb").read() == plain
    with pytest.raises(ValueError):
        mesh.extract(r, config.preset("wanjinyou", ["mesh.source=tsdf"]), scene, str(tmp_path))
    assert len(r.calls) == 1
