"""View-colour fusion without a GPU: f2n_view_colors_accumulate / f2n_view_colors_finalize (csrc/dataset.hip) under the wavefront emulator
(tests/wave_emul) against the float32 restatement of tests/view_colors_ref.py, bit for bit (both builds use -ffp-contract=off); the
algorithm's known answer and its occlusion test on analytic maps of a sphere (the restatement alone, then the emulator); the
mesh.color_source / colors.* options."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import tsdf_ref as tr  # noqa: E402
import view_colors_ref as vr  # noqa: E402

F32 = np.float32
INVALID = -1  # F2N_ERR_INVALID_ARG
_f, _i, _l = ctypes.c_float, ctypes.c_int, ctypes.c_int64


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


@pytest.fixture(scope="module")
def rig(fox_state):
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    return vr.sphere_rig(fox_state, mesh.view_intrinsics)


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def emul_accumulate(L, c, acc, wsum, count, v0=0, v1=None, conf="case", normals="case", raw=None):
    """f2n_view_colors_accumulate of the views [v0, v1) of case c into acc, wsum, count (host arrays, in place); raw (a dict) replaces
    raw arguments (the error-code test)."""
    v1 = len(c["depth"]) if v1 is None else v1
    cf = c["conf"] if isinstance(conf, str) else conf
    nr = c["normals"] if isinstance(normals, str) else normals
    cut = lambda a: None if a is None else np.ascontiguousarray(a[v0:v1], F32)  # noqa: E731
    a = dict(n=len(c["points"]), points=np.ascontiguousarray(c["points"], F32), normals=None if nr is None else np.ascontiguousarray(nr, F32),
             V=v1 - v0, poses=cut(c["poses"]), intri=cut(c["intri"]), dist=cut(c["dist"]), depth=cut(c["depth"]), conf=cut(cf), image=cut(c["image"]),
             C=acc.shape[1], h=c["h"], w=c["w"], tol=c["tol"], cos_min=c["cos_min"], acc=acc, wsum=wsum, count=count)
    a.update(raw or {})
    return L.f2n_view_colors_accumulate(None, _l(a["n"]), _vp(a["points"]), _vp(a["normals"]), _i(a["V"]), _vp(a["poses"]), _vp(a["intri"]),
                                        _vp(a["dist"]), _vp(a["depth"]), _vp(a["conf"]), _vp(a["image"]), _i(a["C"]), _i(a["h"]), _i(a["w"]),
                                        _f(a["tol"]), _f(a["cos_min"]), _vp(a["acc"]), _vp(a["wsum"]), _vp(a["count"]))


def emul_finalize(L, acc, wsum, count, min_views):
    rgb, known = np.full(acc.shape, np.nan, F32), np.full(len(acc), 7, np.uint8)
    assert L.f2n_view_colors_finalize(None, _l(len(acc)), _i(acc.shape[1]), _vp(acc), _vp(wsum), _vp(count), _i(min_views), _vp(rgb), _vp(known)) == 0
    return rgb, known


def check_accumulate(c, C, accumulate, finalize):
    """The identities of f2n_view_colors_accumulate / _finalize on the grid case c with an image of C channels;
    accumulate(c, acc, wsum, count, v0, v1, conf, normals) updates host arrays in place (the emulator here, the device in
    tests/test_gpu_view_colors.py)."""
    c = dict(c, image=vr.image_for(c, C))
    n, V = len(c["points"]), len(c["depth"])
    rng = np.random.default_rng(1)
    zero = (np.zeros((n, C), F32), np.zeros(n, F32), np.zeros(n, np.int32))
    busy = (rng.standard_normal((n, C)).astype(F32), rng.uniform(0, 2, n).astype(F32), rng.integers(0, 3, n).astype(np.int32))  # a state that is not zero
    same = lambda x, y: all(tr.same_bits(a, b) for a, b in zip(x, y))  # noqa: E731
    for s0 in (zero, busy):
        stats = {}
        ref = vr.accumulate(*s0, c["points"], c["normals"], c["poses"], c["intri"], c["dist"], c["depth"], c["conf"], c["image"], c["tol"],
                            c["cos_min"], stats)
        one = tuple(a.copy() for a in s0)
        accumulate(c, *one, 0, V, "case", "case")
        assert same(one, ref)
        two = tuple(a.copy() for a in s0)  # in two batches: the same bits
        accumulate(c, *two, 0, 2, "case", "case")
        assert not tr.same_bits(two[1], one[1])
        accumulate(c, *two, 2, V, "case", "case")
        assert same(two, one)
        again = tuple(a.copy() for a in s0)  # a second call on fresh state
        accumulate(c, *again, 0, V, "case", "case")
        assert same(again, one)
    # the case does what it was built for: every exit is taken, the planted ones at least three times
    assert all(stats[k] > 0 for k in ("behind", "facing", "no_tap", "tap_outside", "no_depth", "depth_low", "depth_high", "conf0", "used_1",
                                      "used_2", "used_3", "used_4")), stats
    assert stats["at_minus_tol"] >= 3 and stats["at_plus_tol"] >= 3 and stats["used_4"] >= 3 and stats["used_3"] >= 3, stats
    shares = []  # (the last state: counts of 0..2 before the five views, so that min_views = 6 still leaves some points known)
    for mv in (1, 2, 6):
        rgb, known = finalize(*one, mv)
        rr, rk = vr.finalize(*ref, mv)
        assert tr.same_bits(rgb, rr) and tr.same_bits(known, rk)
        assert (rr[rk == 0] == 0).all() and (rr[rk != 0] != 0).any()
        shares.append(rk.mean())
    assert 1 > shares[0] > shares[1] > shares[2] > 0, shares
    # NULL conf is conf == 1; NULL normals are zero normals
    a, b = tuple(x.copy() for x in zero), tuple(x.copy() for x in zero)
    accumulate(c, *a, 0, V, None, "case")
    accumulate(c, *b, 0, V, np.ones_like(c["depth"]), "case")
    assert same(a, b) and not same(a, one) and a[2].max() >= 2
    a, b = tuple(x.copy() for x in zero), tuple(x.copy() for x in zero)
    accumulate(c, *a, 0, V, "case", None)
    accumulate(c, *b, 0, V, "case", np.zeros_like(c["normals"]))
    assert same(a, b) and not same(a, one)
    assert same(a, vr.accumulate(*zero, c["points"], None, c["poses"], c["intri"], c["dist"], c["depth"], c["conf"], c["image"], c["tol"], c["cos_min"]))
    # no views: the state is not touched
    keep = (np.full((n, C), 7, F32), np.full(n, np.nan, F32), np.full(n, -3, np.int32))
    accumulate(c, *keep, 2, 2, "case", "case")
    assert (keep[0] == 7).all() and np.isnan(keep[1]).all() and (keep[2] == -3).all()


def _emul_checked(L):
    def accumulate(c, acc, wsum, count, v0, v1, conf, normals):
        assert emul_accumulate(L, c, acc, wsum, count, v0, v1, conf, normals) == 0
    return accumulate, lambda acc, wsum, count, mv: emul_finalize(L, acc, wsum, count, mv)


@pytest.fixture(scope="module")
def grid_case(fox_state):
    c = vr.grid_case(fox_state)
    assert len(c["points"]) == 14763 and c["depth"].shape == (5, 61, 45) and float(c["tol"]) == 0.0625
    d, nr = c["depth"], c["normals"]
    assert (d == 0).any() and (d < 0).any() and np.isnan(d).any() and np.isposinf(d).any() and (c["conf"] == 0).any()
    assert (nr == 0).all(1).any() and np.isnan(nr).any(1).any() and np.isinf(nr).any(1).any()
    return c


@pytest.mark.parametrize("C", [1, 3, 4])
def test_accumulate_and_finalize_on_the_emulator(emul, grid_case, C):
    check_accumulate(grid_case, C, *_emul_checked(emul))


def check_error_codes(call):
    """Every error code of f2n_view_colors_accumulate, and the calls that touch nothing; call(**replaced raw arguments) returns the status."""
    for tol in (0.0, -0.5, float("nan"), float("inf")):
        assert call(tol=tol) == INVALID, tol
    assert call(cos_min=float("nan")) == INVALID
    for k in ("n", "V", "h", "w"):
        assert call(**{k: -1}) == INVALID, k
    for bad in (0, 5, -1):
        assert call(C=bad) == INVALID, bad
    assert call(h=0) == INVALID and call(w=0) == INVALID and call(h=(1 << 24) + 1) == INVALID
    for k in ("points", "poses", "intri", "dist", "depth", "image", "acc", "wsum", "count"):
        assert call(**{k: None}) == INVALID, k
    assert call(V=0) == 0 and call(n=0) == 0 and call(V=0, poses=None, depth=None, image=None, acc=None) == 0 and call(n=0, points=None, wsum=None) == 0


def test_error_codes(emul, grid_case):
    c = dict(grid_case, image=vr.image_for(grid_case, 3))
    c["points"], c["normals"] = c["points"][:300], c["normals"][:300]
    acc, wsum, count = np.full((300, 3), 7, F32), np.full(300, 7, F32), np.full(300, 7, np.int32)
    call = lambda **raw: emul_accumulate(emul, c, acc, wsum, count, raw=raw)  # noqa: E731
    check_error_codes(call)
    assert (acc == 7).all() and (wsum == 7).all() and (count == 7).all()  # nothing was written by any of the calls above
    assert call(cos_min=-float("inf")) == 0 and call(normals=None, conf=None) == 0 and (count != 7).any()
    rgb, known = np.full((300, 3), 7, F32), np.full(300, 7, np.uint8)
    fin = lambda n, C, a, w, k, mv, og, ok: emul.f2n_view_colors_finalize(None, _l(n), _i(C), _vp(a), _vp(w), _vp(k), _i(mv), _vp(og), _vp(ok))  # noqa: E731
    assert fin(-1, 3, acc, wsum, count, 1, rgb, known) == INVALID and fin(300, 0, acc, wsum, count, 1, rgb, known) == INVALID
    assert fin(300, 5, acc, wsum, count, 1, rgb, known) == INVALID
    for k in range(5):
        args = [acc, wsum, count, rgb, known]
        args[k] = None
        assert fin(300, 3, args[0], args[1], args[2], 1, args[3], args[4]) == INVALID
    assert fin(0, 3, None, None, None, 1, None, None) == 0 and (rgb == 7).all() and (known == 7).all()
    assert fin(300, 3, acc, wsum, count, -5, rgb, known) == 0 and (known != 7).all()


def emul_fuse(L):
    """vr.fuse's signature on the emulator"""
    def fuse(points, normals, case, C=3, min_views=1):
        c = dict(case, points=points, normals=normals)
        n = len(points)
        acc, wsum, count = np.zeros((n, C), F32), np.zeros(n, F32), np.zeros(n, np.int32)
        assert emul_accumulate(L, c, acc, wsum, count) == 0
        return emul_finalize(L, acc, wsum, count, min_views) + (wsum, count)
    return fuse


def test_sphere_colours_are_the_painted_normals(emul, rig):
    """The algorithm's known answer (vr.sphere_rig): every point of the sphere that some view sees by a margin is known, and its colour is
    0.5 + 0.5 n within vr.sphere_bound -- derived there from the pixel footprint at the grazing limit times the colour's gradient
    0.5 / R (0.059 for this rig; the restatement gives 3.2e-4 at most) --; every point no view sees by a margin is unknown; at most 15 %
    of the points are in neither class (11.4 %).  The restatement alone first, then the emulator under the same bound, which must also
    give the restatement's bits."""
    assert rig["depth"].shape == (6, 480, 270) and len(rig["points"]) == 4000
    assert (rig["depth"] > 0).any(axis=(1, 2)).all() and abs(vr.sphere_bound(rig) - 0.0588) < 1e-3
    vr.check_sphere(rig, vr.fuse)
    vr.check_sphere(rig, emul_fuse(emul))
    for a, b in zip(vr.fuse(rig["points"], rig["normals"], rig), emul_fuse(emul)(rig["points"], rig["normals"], rig)):
        assert tr.same_bits(a, b)


def test_an_occluded_view_does_not_colour_the_point(emul, rig):
    """A disc in front of the sphere in view 0's depth map only, view 0 painted (1, 0, 0) and view 1 (0, 1, 0): the points hidden behind
    the disc in view 0 and seen by view 1 come out (0, 1, 0) within 1e-6 from one view (vr.check_occlusion)."""
    vr.check_occlusion(rig, vr.fuse)
    vr.check_occlusion(rig, emul_fuse(emul))


def test_options_parse_and_default():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    o = mesh.view_color_options(config.preset("wanjinyou", []))
    assert o == {"color_source": "radiance", "res_level": 2, "tol_steps": 2.0, "cos_min": 0.1, "min_views": 1, "max_views": 0, "views_per_batch": 8,
                 "tau": 0.5, "min_opacity": 0.5, "image": "render"}
    o = mesh.view_color_options(config.preset("wanjinyou", ["mesh.color_source=Views ", "colors.res_level=4", "colors.tol_steps=1.5", "colors.cos_min=0.3",
                                                            "colors.min_views=2", "colors.max_views=5", "colors.views_per_batch=3", "colors.tau=0.25",
                                                            "colors.min_opacity=0.1", "colors.image=photo"]))
    assert o == {"color_source": "views", "res_level": 4, "tol_steps": 1.5, "cos_min": 0.3, "min_views": 2, "max_views": 5, "views_per_batch": 3,
                 "tau": 0.25, "min_opacity": 0.1, "image": "photo"}
    for bad in ("mesh.color_source=view", "mesh.color_source=true", "colors.image=photos", "colors.res_level=0", "colors.views_per_batch=0",
                "colors.max_views=-1", "colors.min_views=0", "colors.tau=0", "colors.tau=1.5", "colors.tol_steps=0", "colors.tol_steps=-1",
                "colors.tol_steps=inf", "colors.cos_min=1", "colors.cos_min=-1.5", "colors.cos_min=nan", "colors.min_opacity=-0.5"):
        with pytest.raises(ValueError):
            mesh.view_color_options(config.preset("wanjinyou", [bad]))
    assert "colors" not in config.GROUP_DEFAULTS
    # the other parsers return what they returned before, with or without the new keys in the configuration
    for extra in ([], ["mesh.color_source=views", "colors.res_level=4"]):
        cfg = config.preset("wanjinyou", extra)
        assert mesh.options(cfg) == {"resolution": 256, "level": mesh.DEFAULT_LEVEL, "bbox_min": mesh.options(cfg)["bbox_min"],
                                     "bbox_max": mesh.options(cfg)["bbox_max"], "normals": False, "colors": False, "min_component_faces": 0,
                                     "normal_source": "grid", "source": "density", "simplify": 0, "refine": None, "sparse": 0}
        assert mesh.texture_options(cfg) == {"texture": False, "texels_per_step": 2.0, "max_size": 8192, "max_block_log2": 7, "source": "point",
                                             "ray_steps": 4.0}
        assert mesh.tsdf_options(cfg) == {"res_level": 4, "trunc_voxels": 4.0, "tau": 0.5, "min_opacity": 0.5, "min_weight": 1.0,
                                          "views_per_batch": 8, "max_views": 0}
        assert mesh.check_options(cfg) == {"check": False, "res_level": 4, "tau": 0.5, "min_opacity": 0.5, "max_views": 0}
    assert mesh.TEXTURE_SOURCES == ("point", "ray", "views")
    assert mesh.texture_options(config.preset("wanjinyou", ["texture.source=views"]))["source"] == "views"
    with pytest.raises(ValueError):
        mesh.texture_options(config.preset("wanjinyou", ["texture.source=view"]))
    # the pixel-centre convention: entry (a, b) of the maps looks through the centre of full-resolution pixel (a s + s // 2, b s + s // 2)
    k = mesh.view_intrinsics(np.array([[[8.0, 0, 4.5], [0, 6.0, 2.5], [0, 0, 1.0]]]), 4)
    assert k.dtype == F32 and k.tolist() == [[[2.0, 0, 1.0], [0, 1.5, 0.5], [0, 0, 1.0]]]
    for s in (1, 2, 3, 8):  # the ray of entry b projects to b + 0.5
        fx, cx = 517.25, 271.125
        kk = mesh.view_intrinsics(np.array([[[fx, 0, cx], [0, fx, cx], [0, 0, 1.0]]]), s)[0]
        for b in (0, 5):
            u = (b * s + s // 2 + 0.5 - cx) / fx  # f2n_img2world_rays: pixel j looks through j + 0.5
            assert abs(float(kk[0, 0]) * u + float(kk[0, 2]) - (b + 0.5)) < 1e-4


def test_bake_texture_refuses_views_without_a_function():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    with pytest.raises(ValueError) as e:
        mesh.bake_texture(None, None, None, None, 1.0, source="views")
    assert "view_colors" in str(e.value)
