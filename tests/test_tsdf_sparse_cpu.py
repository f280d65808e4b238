"""Sparse TSDF fusion on bricks without a GPU: f2n_tsdf_brick_mark, f2n_tsdf_integrate_bricks (csrc/dataset.hip),
f2n_brick_mesh_count_masked / _emit_masked (csrc/octree.hip) and their host wrappers (csrc/host/RendererQuery.cpp) under the wavefront
emulator (tests/wave_emul), against the numpy restatement of tests/tsdf_sparse_ref.py and against the dense kernels' own output
(f2n_tsdf_integrate -> f2n_tsdf_finalize -> f2n_mesh_count_masked -> f2n_mesh_emit), bit for bit.  The checks are functions of an `impl`
(numpy in, numpy out): tests/test_gpu_tsdf_sparse.py runs them on the device through host.* and capi.*.  The check_huge_* bodies run the
listed-brick kernels on windows of virtual grids whose corner indices and brick ids need more than 32 bits (tests/mesh_sparse_ref.py)."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import mesh_ref as mr  # noqa: E402
import mesh_sparse_ref as sr  # noqa: E402
import tsdf_ref as tr  # noqa: E402
import tsdf_sparse_ref as ts  # noqa: E402
from test_tsdf_cpu import mask_cases, sphere_case  # noqa: E402
from test_mesh_sparse_cpu import huge_case  # noqa: E402

F32 = np.float32
INVALID, UNSUPPORTED = -1, -2  # F2N_ERR_INVALID_ARG, F2N_ERR_UNSUPPORTED
_f, _i = ctypes.c_float, ctypes.c_int

# (case, B) -> (flagged bricks, bricks) of the restatement, computed on the CPU when the cases were chosen
ACTIVE = {("sphere", 4): (112, 512), ("sphere", 8): (27, 64), ("sphere", 16): (8, 8), ("synth_conf", 4): (187, 225), ("synth_conf", 8): (45, 45),
          ("synth", 4): (189, 225), ("synth", 8): (45, 45)}
# case -> (min_weight, vertices, faces) of the dense masked mesh, from the restatement
MESHES = {"sphere": (0.5, 2643, 5058), "synth_conf": (1e-4, 2940, 3864)}

_CASES, _REF = {}, {}


def case(st, name):
    """sphere: test_tsdf_cpu.sphere_case at 33^3 (43 views, 120 x 67 maps); synth / synth_conf: tsdf_ref.synthetic_case at (37, 21, 19),
    5 views, 61 x 45 maps with NaN, inf, zero and negative depths and planted sdf == -trunc pixels, without / with conf.  Built once."""
    if name not in _CASES:
        _CASES[name] = sphere_case(st, 33)[0] if name == "sphere" else tr.synthetic_case(st, with_conf=name == "synth_conf")
    return _CASES[name]


def dims(c):
    return (c["nx"], c["ny"], c["nz"])


def ref(st, name, what, *args):
    """the restatement's results per case, computed once and never modified"""
    key = (name, what) + args
    if key not in _REF:
        c = case(st, name)
        if what == "flags":
            _REF[key] = ts.brick_mark(c, *args)
        elif what == "sums":  # f2n_tsdf_integrate from zero
            z = np.zeros(dims(c)[::-1], F32)
            _REF[key] = tr.integrate(z, z, c["lo"], c["step"], c["nx"], c["ny"], c["nz"], c["poses"], c["intri"], c["dist"], c["depth"], c["conf"],
                                     c["trunc"])
        elif what == "mesh":  # (g, valid, verts, faces) of the dense chain at min_weight args[0]
            S, W = ref(st, name, "sums")
            g, valid = tr.finalize(S, W, args[0])
            v, f = tr.marching_tets_masked(g, 0.0, valid, c["lo"], c["step"])[:2]
            _REF[key] = (g, valid, v, f)
        for a in _REF[key] if isinstance(_REF[key], tuple) else (_REF[key],):
            a.setflags(write=False)
    return _REF[key]


def all_bricks(c, B):
    return np.arange(int(np.prod(sr.n_bricks(dims(c), B))), dtype=np.int32)


# ---- 1. flags ----------------------------------------------------------------------------------------------------------------------
def check_mark(impl, st, name, B):
    c = case(st, name)
    want = ref(st, name, "flags", B)
    flags = impl.mark(c, B)
    active, total = ACTIVE[(name, B)]
    print("%s B=%d: %d of %d bricks flagged" % (name, B, int(flags.sum()), flags.size))
    assert flags.dtype == np.uint8 and flags.shape == want.shape and (flags == want).all()
    assert int(want.sum()) == active and want.size == total and 0 < active and set(np.unique(flags)) <= {0, 1}
    if (name, B) in (("sphere", 4), ("sphere", 8), ("synth_conf", 4), ("synth", 4)):
        assert 0 < int(flags.sum()) < flags.size
    return flags


def check_mark_cases_do_what_they_were_built_for(st):
    """the synthetic grid has the border-plane owner case (x, y extents multiples of 4), a partial brick (z), and planted sdf == -trunc
    pixels whose voxels count as hits"""
    c = case(st, "synth_conf")
    assert (c["nx"] - 1) % 4 == 0 and (c["ny"] - 1) % 4 == 0 and (c["nz"] - 1) % 4 != 0
    stats = {}
    z = np.zeros(dims(c)[::-1], F32)
    tr.integrate(z, z, c["lo"], c["step"], c["nx"], c["ny"], c["nz"], c["poses"], c["intri"], c["dist"], c["depth"], c["conf"], c["trunc"], stats)
    assert stats["at_minus_trunc"] >= 3 and stats["far_behind"] > 0 and stats["no_conf"] > 0 and stats["no_depth"] > 0
    d = c["depth"]
    assert (d == 0).any() and (d < 0).any() and np.isnan(d).any() and np.isposinf(d).any()


def check_mark_few_views(impl, st):
    c = case(st, "synth_conf")
    one = impl.mark(c, 4, 1, 2)
    assert (one == ts.brick_mark(c, 4, 1, 2)).all() and 0 < one.sum() < ref(st, "synth_conf", "flags", 4).sum()
    none = impl.mark(c, 4, 2, 2)
    assert none.shape == one.shape and (none == 0).all()
    assert (impl.mark(c, 4, conf=None) == ts.brick_mark(c, 4, conf=None)).all()  # NULL conf


# ---- 2. brick integration ----------------------------------------------------------------------------------------------------------
def check_integrate_bricks(impl, st, name, B):
    c = case(st, name)
    n, V = dims(c), len(c["depth"])
    P = (B + 1) ** 3
    ids = all_bricks(c, B)
    z = np.zeros(n[::-1], F32)
    dS, dW = impl.integrate(c, z, z.copy())  # the dense kernel itself
    rs, rw = ref(st, name, "sums")
    assert tr.same_bits(dS, rs) and tr.same_bits(dW, rw)  # (the dense entry point still gives the restatement's bits)
    sent = np.full((len(ids), P), -7.5, F32)  # every existing corner starts from zero, the others from a sentinel
    S0, W0 = ts.brick_rows(z, ids, n, B, sent), ts.brick_rows(z, ids, n, B, sent)
    assert (S0 == -7.5).any() == any((n[k] - 1) % B for k in range(3))
    S, W = impl.integrate_bricks(c, S0, W0, ids, B)
    assert tr.same_bits(S, ts.brick_rows(dS, ids, n, B, sent)) and tr.same_bits(W, ts.brick_rows(dW, ids, n, B, sent))
    # ... which is mesh_sparse_ref.brick_values of the dense grids, the sentinel where a corner does not exist
    assert tr.same_bits(S, sr.brick_values(dS, ids, B, -7.5)) and (W > 0).any()
    # views [0, k) then [k, V): the bits of one call
    S2, W2 = impl.integrate_bricks(c, S0, W0, ids, B, 0, 2)
    assert not tr.same_bits(W2, W)
    S2, W2 = impl.integrate_bricks(c, S2, W2, ids, B, 2, V)
    assert tr.same_bits(S2, S) and tr.same_bits(W2, W)
    # no views: untouched
    S3, W3 = impl.integrate_bricks(c, S0, W0, ids, B, 2, 2)
    assert tr.same_bits(S3, S0) and tr.same_bits(W3, W0)
    # a permuted subset, each id once: the same rows
    rng = np.random.default_rng(B)
    sub = rng.permutation(ids)[:max(3, len(ids) // 3)].astype(np.int32)
    Sp, Wp = impl.integrate_bricks(c, S0[sub], W0[sub], sub, B)
    assert tr.same_bits(Sp, S[sub]) and tr.same_bits(Wp, W[sub])


def check_integrate_bricks_leaves_foreign_rows(raw, st):
    """raw(c, S, W, ids, B) = the C entry point on host arrays, ids unchecked: a brick id outside the grid keeps its whole row"""
    c = case(st, "synth_conf")
    B, n = 4, dims(c)
    total = int(np.prod(sr.n_bricks(n, B)))
    ids = np.array([3, total, -1, 7, 2 ** 31 - 1], np.int32)
    S, W = np.full((5, 125), -7.5, F32), np.full((5, 125), -7.5, F32)
    assert raw(c, S, W, ids, B) == 0
    assert (S[[1, 2, 4]] == -7.5).all() and (W[[1, 2, 4]] == -7.5).all() and (W[[0, 3]] != -7.5).any()


# ---- 4. the masked brick mesher ----------------------------------------------------------------------------------------------------
def check_masked_brick_mesher(impl, B):
    shapes = [(7, 8, 9), {4: (5, 9, 13), 8: (9, 9, 17)}[B]]  # the second: every extent (n - 1) a multiple of B
    for shape in shapes:
        g, level, lo, step, masks = mask_cases(shape)
        nz, ny, nx = g.shape
        n = (nx, ny, nz)
        if shape != (7, 8, 9):
            assert all((k - 1) % B == 0 for k in n)
        ids = all_bricks(dict(nx=nx, ny=ny, nz=nz), B)
        values = sr.brick_values(g, ids, B)  # (NaN where a corner does not exist: never read)
        for name, valid in masks.items():
            ok = ts.brick_rows(valid, ids, n, B, np.full((len(ids), (B + 1) ** 3), 9, np.uint8))  # (9 where no corner exists: never read)
            dv, df = impl.mesh_masked_grid(g, valid, level, lo, step)
            assert len(df) > 0
            for batch in (0, 1, 2):
                v, f = impl.mesh_masked_bricks(values, ok, ids, n, lo, step, level, B, batch)
                assert v.dtype == F32 and f.dtype == np.int32
                assert tr.same_bits(v, dv) and tr.same_bits(f, df), (shape, name, B, batch)
            if name == "ones":
                pv, pf = impl.mesh_bricks(values, ids, n, lo, step, level, B, 0)
                assert tr.same_bits(v, pv) and tr.same_bits(f, pf)
            else:  # the emitted vertices are a superset of the dense masked rule's: some are dropped
                keys = ts.masked_brick_vertex_keys(g, valid, level, ids, B)
                assert len(keys) > len(dv)
                if shape == (7, 8, 9):  # (the dense kernels' own footing: the restatement's masked mesh)
                    rv, rf = tr.marching_tets_masked(g, level, valid, lo, step)[:2]
                    assert tr.same_bits(dv, rv) and tr.same_bits(df, rf)


def check_flagged_bricks_give_the_dense_mesh(impl, st, name, B):
    """over the hit-flagged bricks only: f2n_tsdf_integrate_bricks from zero -> f2n_tsdf_finalize -> the masked brick mesher = the dense
    masked mesh (the restatement's, and the dense kernels')"""
    c = case(st, name)
    n = dims(c)
    mw, nv, nf = MESHES[name]
    g, valid, rv, rf = ref(st, name, "mesh", mw)
    assert (len(rv), len(rf)) == (nv, nf)
    ids = np.flatnonzero(ref(st, name, "flags", B).reshape(-1)).astype(np.int32)
    z = np.zeros((len(ids), (B + 1) ** 3), F32)
    S, W = impl.integrate_bricks(c, z, z.copy(), ids, B)
    bg, bvalid = impl.finalize(S, W, mw)
    for batch in (0, max(1, len(ids) // 3)):
        v, f = impl.mesh_masked_bricks(bg, bvalid, ids, n, c["lo"], float(c["step"]), 0.0, B, batch)
        assert tr.same_bits(v, rv) and tr.same_bits(f, rf), (name, B, batch)
    dv, df = impl.mesh_masked_grid(g, valid, 0.0, c["lo"], float(c["step"]))
    assert tr.same_bits(dv, rv) and tr.same_bits(df, rf)


def check_value_errors(impl, st):
    c = case(st, "synth_conf")
    n = dims(c)
    ids = all_bricks(c, 4)[:4]
    z = np.zeros((4, 125), F32)
    with pytest.raises(ValueError):
        impl.mark(c, 5)
    with pytest.raises(ValueError):
        impl.integrate_bricks(c, np.zeros((4, 216), F32), np.zeros((4, 216), F32), ids, 5)
    total = int(np.prod(sr.n_bricks(n, 4)))
    for bad in (total, -1, 1):  # outside the grid, outside, listed twice
        with pytest.raises(ValueError):
            impl.integrate_bricks(c, z, z.copy(), np.array([0, 1, 2, bad], np.int32), 4)
        with pytest.raises(ValueError):
            impl.mesh_masked_bricks(z, np.ones((4, 125), np.uint8), np.array([0, 1, 2, bad], np.int32), n, c["lo"], float(c["step"]), 0.0, 4, 0)
    for trunc in (0.0, -1.0, float("nan"), float("inf")):
        bad = dict(c)
        bad["trunc"] = trunc
        with pytest.raises(ValueError):
            impl.mark(bad, 4)
        with pytest.raises(ValueError):
            impl.integrate_bricks(bad, z, z.copy(), ids, 4)


# ---- virtual grids whose indices need more than 32 bits (tests/mesh_sparse_ref.py, HUGE_GRIDS) -----------------------------------
def check_huge_masked_mesher(impl, name):
    """mesh_from_bricks_masked over a window of a huge virtual grid = mesh_from_grid_masked on the window's dense sub-grid with the
    translated lo, bit for bit -- the list ascending and shuffled, in one batch and in three; the dense masked mesh is the restatement's"""
    for which in ("far", "inner"):
        w, g, values, rv, rf = huge_case(name, which)
        n, B, lo, step, m = w["n"], w["B"], w["lo"], w["step"], w["m"]
        valid = (np.random.default_rng(len(name) + B).random(g.shape) > 0.04).astype(np.uint8)
        ok = ts.brick_rows(valid, w["local_ids"], m, B, np.full(values.shape, 9, np.uint8))  # (9 where no corner exists: never read)
        dv, df = impl.mesh_masked_grid(g, valid, 0.0, w["lo_w"], step)
        assert 0 < len(df) < len(rf)  # (the mask removes faces of the sphere, not all of them)
        mv, mf = tr.marching_tets_masked(g, 0.0, valid, w["lo_w"], step)[:2]
        assert tr.same_bits(df, mf) and dv.shape == mv.shape and np.abs(dv - mv).max() <= 1e-6 * step * max(1.0, np.abs(mv).max())
        ids = w["ids"]
        mixed = np.random.default_rng(B).permutation(len(ids))
        third = -(-len(ids) // 3)
        for order, batch in ((np.arange(len(ids)), 0), (mixed, 0), (np.arange(len(ids)), third), (mixed, third)):
            v, f = impl.mesh_masked_bricks(values[order], ok[order], ids[order], n, lo, step, 0.0, B, batch)
            assert v.dtype == F32 and f.dtype == np.int32
            assert tr.same_bits(v, dv) and tr.same_bits(f, df), (name, which, batch)


_HUGE_TSDF = {}


def huge_tsdf_case(st, name, which):
    """(window, the small case that is the window's dense sub-grid, the same views on the huge grid): tsdf_ref.synthetic_case at the
    window's size with a power-of-two step and lo a multiple of it, so that the translation to the huge grid's lo is exact"""
    if (name, which) not in _HUGE_TSDF:
        m = sr.huge_window(name, which)["m"]
        c = tr.synthetic_case(st, dims=m, pow2=True)
        w = sr.huge_window(name, which, lo_w=c["lo"], step=float(c["step"]))
        big = dict(c, nx=w["n"][0], ny=w["n"][1], nz=w["n"][2], lo=np.array(w["lo"], F32))
        _HUGE_TSDF[(name, which)] = (w, c, big)
    return _HUGE_TSDF[(name, which)]


def check_huge_integrate_bricks(impl, st, name):
    """f2n_tsdf_integrate_bricks over a window of a huge virtual grid: the S and W rows are f2n_tsdf_integrate's on the window's dense
    sub-grid, bit for bit; the rows of corners that do not exist are untouched"""
    for which in ("far", "inner"):
        w, c, big = huge_tsdf_case(st, name, which)
        B, m = w["B"], w["m"]
        z = np.zeros(m[::-1], F32)
        dS, dW = impl.integrate(c, z, z.copy())  # the dense kernel on the small grid
        assert (dW > 0).any() and (dW == 0).any()
        sent = np.full((len(w["ids"]), (B + 1) ** 3), -7.5, F32)
        S0 = ts.brick_rows(z, w["local_ids"], m, B, sent)  # every existing corner starts from zero, the others from a sentinel
        assert (S0 == -7.5).any() == (name == "full" and which == "far")  # (the clipped last brick along x)
        wantS, wantW = ts.brick_rows(dS, w["local_ids"], m, B, sent), ts.brick_rows(dW, w["local_ids"], m, B, sent)
        for order in (np.arange(len(w["ids"])), np.random.default_rng(B).permutation(len(w["ids"]))):
            S, W = impl.integrate_bricks(big, S0[order], S0[order], w["ids"][order], B)
            assert tr.same_bits(S, wantS[order]) and tr.same_bits(W, wantW[order]), (name, which)


def check_huge_value_errors(impl, st):
    """exactly 2^31 bricks: refused before anything is allocated or launched"""
    (nx, ny, nz), B = sr.HUGE_REFUSED
    w, c, big = huge_tsdf_case(st, "full", "inner")
    bad = dict(big, nx=nx, ny=ny, nz=nz)
    z = np.zeros((len(w["ids"]), (B + 1) ** 3), F32)
    with pytest.raises(ValueError):
        impl.mark(bad, B)
    with pytest.raises(ValueError):
        impl.integrate_bricks(bad, z, z.copy(), w["ids"], B)
    with pytest.raises(ValueError):
        impl.mesh_masked_bricks(z, np.ones(z.shape, np.uint8), w["ids"], (nx, ny, nz), w["lo"], w["step"], 0.0, B, 0)


# ---- impls -------------------------------------------------------------------------------------------------------------------------
def _views(c, v0, v1, conf, wrap):
    v1 = len(c["depth"]) if v1 is None else v1
    cf = c["conf"] if isinstance(conf, str) else conf
    a = [wrap(np.ascontiguousarray(c[k][v0:v1], F32)) for k in ("poses", "intri", "dist", "depth")]
    return a + [None if cf is None else wrap(np.ascontiguousarray(cf[v0:v1], F32))]


def _lo(c):
    return [float(v) for v in c["lo"]]


def module_impl(m, wrap, unwrap):
    """impl over the host module (the emulated one here, the product's on the device) or over the ctypes binding, which takes the same
    arguments; wrap / unwrap: numpy <-> its tensors"""
    L = lambda v: [float(x) for x in v]  # noqa: E731
    N = lambda v: [int(x) for x in v]  # noqa: E731

    def mark(c, B, v0=0, v1=None, conf="case"):
        return unwrap(m.tsdf_brick_mark(_lo(c), float(c["step"]), N(dims(c)), B, *_views(c, v0, v1, conf, wrap), float(c["trunc"])))

    def integrate_bricks(c, S, W, ids, B, v0=0, v1=None, conf="case"):
        tS, tW = wrap(np.array(S, F32)), wrap(np.array(W, F32))  # (copies: updated in place)
        m.tsdf_integrate_bricks(tS, tW, wrap(np.asarray(ids, np.int32)), _lo(c), float(c["step"]), N(dims(c)), B, *_views(c, v0, v1, conf, wrap),
                                float(c["trunc"]))
        return unwrap(tS), unwrap(tW)

    def integrate(c, S, W):
        tS, tW = wrap(np.array(S, F32)), wrap(np.array(W, F32))
        m.tsdf_integrate(tS, tW, _lo(c), float(c["step"]), *_views(c, 0, None, "case", wrap), float(c["trunc"]))
        return unwrap(tS), unwrap(tW)

    def finalize(S, W, mw):
        g, valid = m.tsdf_finalize(wrap(np.ascontiguousarray(S, F32)), wrap(np.ascontiguousarray(W, F32)), float(mw))
        return unwrap(g), unwrap(valid)

    def mesh_masked_bricks(values, valid, ids, n, lo, step, level, B, batch):
        v, f = m.mesh_from_bricks_masked(wrap(np.ascontiguousarray(values, F32)), wrap(np.ascontiguousarray(valid, np.uint8)),
                                         wrap(np.asarray(ids, np.int32)), N(n), L(lo), float(step), float(level), B, batch)
        return unwrap(v), unwrap(f)

    def mesh_bricks(values, ids, n, lo, step, level, B, batch):
        v, f = m.mesh_from_bricks(wrap(np.ascontiguousarray(values, F32)), wrap(np.asarray(ids, np.int32)), N(n), L(lo), float(step), float(level),
                                  B, batch)
        return unwrap(v), unwrap(f)

    def mesh_masked_grid(g, valid, level, lo, step):
        v, f = m.mesh_from_grid_masked(wrap(np.ascontiguousarray(g, F32)), wrap(np.ascontiguousarray(valid, np.uint8)), L(lo), float(step), float(level))
        return unwrap(v), unwrap(f)

    return types.SimpleNamespace(mark=mark, integrate_bricks=integrate_bricks, integrate=integrate, finalize=finalize,
                                 mesh_masked_bricks=mesh_masked_bricks, mesh_bricks=mesh_bricks, mesh_masked_grid=mesh_masked_grid)


# ---- the emulator ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


@pytest.fixture(scope="module")
def impl(emul):
    """the C++ host layer compiled against the emulated kernel library: on CPU tensors"""
    import importlib.util
    import torch
    import wemu_build
    path = wemu_build.build_host()
    spec = importlib.util.spec_from_file_location("_f2n_host_emul", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return module_impl(mod, lambda a: torch.from_numpy(np.array(a, order="C")), lambda t: t.numpy())  # (a copy: the references are read-only)


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _lo3(lo):
    return (_f * 3)(*(float(v) for v in lo))


def emul_args(c, **repl):
    a = dict(lo=_lo3(c["lo"]), step=c["step"], nx=c["nx"], ny=c["ny"], nz=c["nz"], B=4, V=len(c["depth"]), poses=c["poses"], intri=c["intri"],
             dist=c["dist"], depth=c["depth"], conf=c["conf"], h=c["h"], w=c["w"], trunc=c["trunc"])
    a.update(repl)
    return a


def emul_mark(L, c, flags, **repl):
    a = emul_args(c, **repl)
    return L.f2n_tsdf_brick_mark(None, a["lo"], _f(a["step"]), _i(a["nx"]), _i(a["ny"]), _i(a["nz"]), _i(a["B"]), _i(a["V"]), _vp(a["poses"]),
                                 _vp(a["intri"]), _vp(a["dist"]), _vp(a["depth"]), _vp(a["conf"]), _i(a["h"]), _i(a["w"]), _f(a["trunc"]), _vp(flags))


def emul_integrate_bricks(L, c, S, W, ids, **repl):
    a = emul_args(c, **repl)
    nb = a.get("n_bricks", 0 if ids is None else len(ids))
    return L.f2n_tsdf_integrate_bricks(None, a["lo"], _f(a["step"]), _i(a["nx"]), _i(a["ny"]), _i(a["nz"]), _i(a["B"]), _i(nb), _vp(ids), _i(a["V"]),
                                       _vp(a["poses"]), _vp(a["intri"]), _vp(a["dist"]), _vp(a["depth"]), _vp(a["conf"]), _i(a["h"]), _i(a["w"]),
                                       _f(a["trunc"]), _vp(S), _vp(W))


@pytest.mark.parametrize("name,B", [("synth_conf", 4), ("synth", 4), ("synth_conf", 8), ("synth", 8), ("sphere", 4), ("sphere", 8), ("sphere", 16)])
def test_flags_equal_the_restatement(impl, emul, fox_state, name, B):
    flags = check_mark(impl, fox_state, name, B)
    if name == "synth_conf":  # the C entry point itself
        direct = np.full(flags.shape, 7, np.uint8)
        assert emul_mark(emul, case(fox_state, name), direct, B=B) == 0 and (direct == flags).all()


def test_flags_of_one_view_and_of_none(impl, fox_state):
    check_mark_cases_do_what_they_were_built_for(fox_state)
    check_mark_few_views(impl, fox_state)


@pytest.mark.parametrize("name,B", [("synth_conf", 4), ("synth", 8)])
def test_brick_integration_equals_the_dense_kernel(impl, fox_state, name, B):
    check_integrate_bricks(impl, fox_state, name, B)


def test_brick_integration_leaves_rows_of_foreign_ids(emul, fox_state):
    check_integrate_bricks_leaves_foreign_rows(lambda c, S, W, ids, B: emul_integrate_bricks(emul, c, S, W, ids, B=B), fox_state)


@pytest.mark.parametrize("B", [4, 8])
def test_masked_brick_mesher_equals_the_dense_masked_mesher(impl, B):
    check_masked_brick_mesher(impl, B)


@pytest.mark.parametrize("name,B", [("synth_conf", 4), ("synth_conf", 8), ("sphere", 4), ("sphere", 8)])
def test_flagged_bricks_give_the_dense_mesh(impl, fox_state, name, B):
    check_flagged_bricks_give_the_dense_mesh(impl, fox_state, name, B)


def test_error_codes(impl, emul, fox_state):
    check_value_errors(impl, fox_state)
    c = tr.synthetic_case(fox_state, dims=(9, 7, 5))
    nb = sr.n_bricks((9, 7, 5), 4)
    flags = np.full(nb[::-1], 7, np.uint8)
    ids = np.arange(2, dtype=np.int32)
    S, W = np.full((2, 125), 7, F32), np.full((2, 125), 7, F32)
    mark = lambda **r: emul_mark(emul, c, r.pop("flags", flags), **r)  # noqa: E731
    integ = lambda **r: emul_integrate_bricks(emul, c, r.pop("S", S), r.pop("W", W), r.pop("ids", ids), **r)  # noqa: E731
    for call in (mark, integ):
        for B in (0, 5, 32, -4):
            assert call(B=B) == INVALID, B
        for trunc in (0.0, -0.5, float("nan"), float("inf")):
            assert call(trunc=trunc) == INVALID, trunc
        for k in ("nx", "ny", "nz", "V", "h", "w"):
            assert call(**{k: -1}) == INVALID, k
        assert call(h=0) == INVALID and call(w=0) == INVALID and call(h=(1 << 24) + 1) == INVALID and call(w=(1 << 24) + 1) == INVALID
        assert call(nx=1) == INVALID and call(nz=(1 << 19) + 1) == INVALID
        for k in ("lo", "poses", "intri", "dist", "depth"):
            assert call(**{k: None}) == INVALID, k
        assert call(V=0) == 0 and call(V=0, poses=None, depth=None) == 0
    assert mark(flags=None) == INVALID and mark(nx=1 << 19, ny=1 << 19, nz=1 << 19) == UNSUPPORTED
    assert integ(S=None) == INVALID and integ(W=None) == INVALID and integ(ids=None, n_bricks=2) == INVALID and integ(n_bricks=-1) == INVALID
    assert integ(n_bricks=0) == 0 and integ(n_bricks=0, ids=None, S=None, W=None) == 0
    assert (flags == 7).all() and (S == 7).all() and (W == 7).all()  # nothing was written by any of the calls above
    assert mark() == 0 and set(np.unique(flags)) <= {0, 1} and integ() == 0 and (W != 7).any()
    # the masked brick mesher: the unmasked entry points' codes, and valid == NULL
    vals, ok = np.zeros((2, 125), F32), np.ones((2, 125), np.uint8)
    vc, fc = np.full(2, 7, np.int32), np.full(2, 7, np.int32)
    count = lambda B=4, n=2, i=ids, v=vals, o=ok, nx=9: emul.f2n_brick_mesh_count_masked(  # noqa: E731
        None, _i(nx), _i(7), _i(5), _i(B), _i(n), _vp(i), _vp(v), _vp(o), _f(0.0), _vp(vc), _vp(fc))
    assert count(B=5) == INVALID and count(n=-1) == INVALID and count(o=None) == INVALID and count(v=None) == INVALID and count(i=None) == INVALID
    assert count(nx=1) == INVALID and count(n=0) == 0 and (vc == 7).all()
    assert count() == 0 and (vc == 0).all() and (fc == 0).all()
    vs, fs = np.zeros(2, np.int64), np.zeros(2, np.int64)
    vk, vv, fk, fv = np.full(1, 7, np.int64), np.full((1, 3), 7, F32), np.full(1, 7, np.int64), np.full((1, 3), 7, np.int64)
    emit = lambda B=4, n=2, o=ok, lo=_lo3(c["lo"]), out=vk: emul.f2n_brick_mesh_emit_masked(  # noqa: E731
        None, _i(9), _i(7), _i(5), _i(B), _i(n), _vp(ids), _vp(vals), _vp(o), _f(0.0), lo, _f(c["step"]), _vp(vs), _vp(fs), _vp(out), _vp(vv),
        _vp(fk), _vp(fv))
    assert emit(B=5) == INVALID and emit(n=-1) == INVALID and emit(o=None) == INVALID and emit(lo=None) == INVALID and emit(out=None) == INVALID
    assert emit(n=0) == 0 and emit() == 0 and (vk == 7).all() and (fk == 7).all()  # (no crossing: nothing to write)


def test_options():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    assert "sparse" not in mesh.tsdf_options(config.preset("wanjinyou", []))
    for v, want in (("true", 8), ("4", 4), ("8", 8), ("16", 16), ("false", 0)):
        assert mesh.tsdf_options(config.preset("wanjinyou", ["tsdf.sparse=%s" % v]))["sparse"] == want
    for bad in ("5", "32", "maybe"):
        with pytest.raises(ValueError) as e:
            mesh.tsdf_options(config.preset("wanjinyou", ["tsdf.sparse=%s" % bad]))
        assert "tsdf.sparse" in str(e.value)


def test_the_launcher_refuses_before_anything_is_rendered(tmp_path):
    """tsdf.sparse with grid normals, colours or a texture, a brick size that does not exist, and mesh.sparse with mesh.source=tsdf: a
    ValueError before a view is rendered (the runner and the data set of this test cannot render) and nothing is written"""
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the export touched %s" % name)

    scene = {"center": np.zeros(3, F32), "radius": 1.0}
    base = ["mesh.source=tsdf", "mesh.resolution=16"]
    for extra in (["tsdf.sparse=8", "mesh.normals=true"], ["tsdf.sparse=8", "mesh.colors=true"], ["tsdf.sparse=true", "mesh.texture=true"],
                  ["tsdf.sparse=4", "mesh.normals=true", "mesh.normal_source=grid"], ["tsdf.sparse=5"], ["tsdf.sparse=5", "mesh.normal_source=field"],
                  ["mesh.sparse=8"], ["mesh.sparse=8", "tsdf.sparse=8"]):
        with pytest.raises(ValueError):
            mesh.extract(Untouchable(), config.preset("wanjinyou", base + extra), scene, str(tmp_path), Untouchable())
    assert not os.path.exists(os.path.join(str(tmp_path), "meshes"))


@pytest.mark.parametrize("name", sorted(sr.HUGE_GRIDS))
def test_masked_brick_mesher_on_a_huge_virtual_grid(impl, name):
    check_huge_masked_mesher(impl, name)


@pytest.mark.parametrize("name", sorted(sr.HUGE_GRIDS))
def test_brick_integration_on_a_huge_virtual_grid(impl, fox_state, name):
    check_huge_integrate_bricks(impl, fox_state, name)


def test_two_to_the_31_bricks_are_refused(impl, emul, fox_state):
    check_huge_value_errors(impl, fox_state)
    (nx, ny, nz), B = sr.HUGE_REFUSED
    w, c, big = huge_tsdf_case(fox_state, "full", "inner")
    flags, ids = np.full(8, 7, np.uint8), np.ascontiguousarray(w["ids"][:2])
    S, W = np.full((2, 125), 7, F32), np.full((2, 125), 7, F32)
    assert emul_mark(emul, big, flags, nx=nx, ny=ny, nz=nz, B=B) == UNSUPPORTED
    assert emul_integrate_bricks(emul, big, S, W, ids, nx=nx, ny=ny, nz=nz, B=B) == UNSUPPORTED
    assert (flags == 7).all() and (S == 7).all() and (W == 7).all()  # nothing was written
    assert emul_integrate_bricks(emul, big, S, W, ids, B=B) == 0 and (W != 7).any()  # the full grid, 2^31 - 262144 bricks, is accepted
