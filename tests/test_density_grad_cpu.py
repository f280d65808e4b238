"""The analytic density gradient without a GPU: the float64 restatement (tests/density_grad_ref.py) checks itself against central
differences of its own forward, the kernels of f2n_field_density_grad / f2n_hash_pos_grad / f2n_density_grad_scatter run under the
wavefront emulator (tests/wave_emul) against it, and the launcher's mesh.normal_source option.

Error metric everywhere: max_i |g_i - g_ref64,i| / S_i with S the sum of the absolute values of all addends of the component.  Bar of
the kernels: 8 x the restatement's own float32-vs-float64 discrepancy on the same inputs (the margin of
tests/test_mesh_attrs_cpu.py::test_normals_on_the_emulator_match_the_restatement), computed inside the test.  Points with a ReLU tie
(|(W1 x)_j| <= 2^-20 sum_k |W1[j,k] x_k| for some hidden unit, float64) are left out; at most 1 % may be."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import density_grad_ref as dr  # noqa: E402
from oracle import capi as oc, pipeline as op  # noqa: E402

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


@pytest.fixture(scope="module")
def fox(fox_state):
    """The fox scene's grid (2^14 entries per level, a trained-looking table) and field network, as the fox runner of the GPU tests."""
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, runtime
    cfg = config.preset("wanjinyou", ["field.log2_table_size=14"])
    arrays = runtime.initial_states(fox_state, cfg, 1, 0.3)
    grid = op.HashGrid(arrays[4], arrays[5], arrays[6], int(arrays[7][0]), 14)
    return grid, np.asarray(arrays[8], F32)


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _hash_args(grid):
    keep = [np.ascontiguousarray(grid.table_h, np.uint16), np.ascontiguousarray(grid.prim_pool, np.int32), np.ascontiguousarray(grid.local_idx, np.int32),
            np.ascontiguousarray(grid.local_size, np.int32), np.ascontiguousarray(grid.bias_pool, F32), np.ascontiguousarray(grid.scales, F32)]
    return keep


def emul_density_grad(L, grid, params, w32, vol, x_h, want_dx=True):
    n = len(w32)
    a = _hash_args(grid)
    ph = oc.f2h(params)
    w32, vol, x_h = np.ascontiguousarray(w32, F32), np.ascontiguousarray(vol, np.int32), np.ascontiguousarray(x_h, np.uint16)
    dx = np.full((n, 32), np.nan, F32) if want_dx else None
    g = np.full((n, 3), np.nan, F32)
    rc = L.f2n_field_density_grad(None, n, grid.n_volumes, *[_vp(v) for v in a], _vp(w32), _vp(vol), 1, _vp(ph), _vp(x_h), _vp(dx), _vp(g))
    assert rc == 0
    return dx, g


def emul_pos_grad(L, grid, w32, vol, dx):
    n = len(w32)
    a = _hash_args(grid)
    w32, vol, dx = np.ascontiguousarray(w32, F32), np.ascontiguousarray(vol, np.int32), np.ascontiguousarray(dx, F32)
    g = np.full((n, 3), np.nan, F32)
    assert L.f2n_hash_pos_grad(None, n, grid.n_volumes, *[_vp(v) for v in a], _vp(w32), _vp(vol), 1, _vp(dx), _vp(g)) == 0
    return g


def _points(rng, grid, n, lo=-1.0, hi=1.0):
    return rng.uniform(lo, hi, (n, 3)).astype(F32), rng.integers(0, grid.n_volumes, n).astype(np.int32)


def test_the_restatement_checks_itself(fox):
    """Float64 central differences of the restatement's own float64 forward (the same h16 table and weights, no activation rounding)
    against its analytic df0/dw, at points at least 1e-3 of a finest-level cell away from every cell face: 1e-6 relative to S.  The step
    is 1e-6 of a finest cell; a point where a hidden unit changes sign inside the stencil is left out with the ReLU ties (the forward has
    a kink there: no difference quotient is the derivative; the analytic derivative takes its mask from the h16 features, the stencil's
    forward from its own unrounded ones).  Measured: 1964 of 2000 points away from the faces, 11 left out (0.56 %), error 2.05e-8 of S;
    |f0_64 - oracle f0| <= 1.9e-4 (the oracle rounds features and activations to h16)."""
    grid, params = fox
    rng = np.random.default_rng(11)
    w, vol = _points(rng, grid, 2000)
    cells = dr.Cells(grid, w, vol)
    away = cells.face_distance() >= 1e-3
    assert away.sum() > 1000
    w, vol = w[away], vol[away]
    c = dr.field_chain(grid, params, w, vol)
    cells, W1, w2 = c["cells"], c["W1"], c["w2"]
    f0 = dr.forward64(cells, W1, w2)
    ref_f0 = op.field_fwd(grid, params, w, vol)[:, 0]
    print("max |f0_64 - oracle f0| = %.3g" % np.abs(f0 - ref_f0).max())
    assert np.abs(f0 - ref_f0).max() <= 2e-3
    h = 1e-6 * 2.0 / float(grid.scales[15])
    fd = np.empty((len(w), 3))
    kink = c["ties"].copy()
    w64 = w.astype(F64)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        fd[:, k] = (dr.forward64(cells, W1, w2, w64 + e) - dr.forward64(cells, W1, w2, w64 - e)) / (2 * h)
        for sgn in (-1.0, 1.0):
            f = cells.frac(w64 + sgn * e, F64)
            x = (dr._weights(f)[..., None] * cells.v).sum(2).reshape(len(w), 32)
            kink |= (((x @ W1.T) > 0) != ((oc.h2f(c["x_h"]).astype(F64) @ W1.T) > 0)).any(1)
    # (the analytic derivative takes the mask of the h16 features x; the forward of the stencil that of its own unrounded features)
    g64, S = dr.df0_dw(cells, c["dx"], F64, c["S_dx"])
    err = dr.rel_err(fd, g64, S, ~kink)
    print("%d points, %d left out, central differences vs analytic: %.3g of S" % (len(w), kink.sum(), err))
    assert kink.mean() <= 0.01
    assert err <= 1e-6, err
    assert np.ptp(g64, axis=0).min() > 1.0  # a gradient that varies


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_field_density_grad_on_the_emulator(emul, fox, n):
    """f2n_field_density_grad and f2n_hash_pos_grad on the emulated wavefront, fed the oracle's x_h, against the float64 restatement.
    Measured (restatement float32-vs-float64 discrepancy -> bar = 8 x that; the emulated kernel's error):
      df0/dw  n = 1: 7.16e-6 -> 5.73e-5; 7.16e-6     n = 63: 9.28e-6 -> 7.42e-5; 9.28e-6     n = 64: 1.12e-5 -> 8.95e-5; 1.12e-5
              n = 65: 9.09e-6 -> 7.27e-5; 9.09e-6    n = 1000: 1.91e-5 -> 1.53e-4; 1.91e-5
      df0/dx  n = 1: 5.05e-8 -> 4.04e-7; 5.05e-8     n = 63: 1.17e-7 -> 9.37e-7; 1.17e-7     n = 64: 1.31e-7 -> 1.04e-6; 1.31e-7
              n = 65: 1.34e-7 -> 1.07e-6; 1.34e-7    n = 1000: 1.76e-7 -> 1.41e-6; 1.76e-7
    The kernel's error equals the discrepancy: the float32 evaluation of the restatement is in the kernels' operation order.  df0/dw's
    is dominated by the float32 fraction of q (q reaches ~2000 at the finest level, so a fraction is off by up to 1e-4 of a cell), an
    input rounding the forward's features share.  No point
    of these inputs has a ReLU tie."""
    grid, params = fox
    rng = np.random.default_rng(100 + n)
    w, vol = _points(rng, grid, n)
    c = dr.field_chain(grid, params, w, vol)
    keep = ~c["ties"]
    assert (~keep).mean() <= 0.01
    dx, g = emul_density_grad(emul, grid, params, w, vol, c["x_h"])
    assert np.isfinite(dx).all() and np.isfinite(g).all()
    for name, got, ref32, ref64, S in (("df0/dx", dx, c["dx32"], c["dx"], c["S_dx"]), ("df0/dw", g, c["g32"], c["g"], c["S_g"])):
        disc = dr.rel_err(ref32, ref64, S, keep)
        err = dr.rel_err(got, ref64, S, keep)
        print("n = %d %s: restatement f32-vs-f64 %.3g, bar %.3g, emulated kernel %.3g, left out %.4f" % (n, name, disc, 8 * disc, err, (~keep).mean()))
        assert disc < 2.0 ** -10  # (what dominates it: the float32 fraction of q < 2^14 is off by up to an ulp of q, 2^-10 of a cell)
        assert err <= 8.0 * disc, (name, err, 8.0 * disc)
    # out_dx through the fused entry is what f2n_hash_pos_grad takes: the same df0/dw, bit for bit; and out_dx = NULL changes nothing
    g2 = emul_pos_grad(emul, grid, w, vol, dx)
    assert (g2.view(np.uint32) == g.view(np.uint32)).all()
    _, g3 = emul_density_grad(emul, grid, params, w, vol, c["x_h"], want_dx=False)
    assert (g3.view(np.uint32) == g.view(np.uint32)).all()


def test_no_points_is_a_no_op(emul, fox):
    grid, params = fox
    a = _hash_args(grid)
    ph = oc.f2h(params)
    guard = np.full((4, 3), 7.0, F32)
    assert emul.f2n_field_density_grad(None, 0, grid.n_volumes, *[_vp(v) for v in a], None, None, 1, _vp(ph), None, None, _vp(guard)) == 0
    assert emul.f2n_hash_pos_grad(None, 0, grid.n_volumes, *[_vp(v) for v in a], None, None, 1, None, _vp(guard)) == 0
    assert emul.f2n_density_grad_scatter(None, 0, None, None, None, None, None, None, None, None, None) == 0
    assert (guard == 7.0).all()
    assert emul.f2n_field_density_grad(None, -1, grid.n_volumes, *[_vp(v) for v in a], None, None, 1, _vp(ph), None, None, _vp(guard)) != 0


def test_cell_faces_and_saturation(emul, fox):
    """Points whose level-0 coordinate q_0 is an integer on an axis (fraction exactly 0: the derivative of the cell floorf chose, i.e.
    the one on the + side of the face), and points with q < 0 (warped coordinates far below -1: the cell index saturates at 0 as in the
    forward, the fraction stays q - floor(q)).  Same metric and bar as above.  Measured: faces 9.31e-6 -> bar 7.44e-5, kernel 9.31e-6;
    saturation 1.37e-5 -> bar 1.10e-4, kernel 1.37e-5."""
    grid, params = fox
    rng = np.random.default_rng(21)
    V = grid.n_volumes
    bias0 = np.asarray(grid.bias_pool, F32).reshape(16, V, 3)[0]
    s0 = grid.scales[0]
    # -- faces: solve p01 * s0 + bias = m for an integer m, keep the candidates for which the float32 evaluation hits m exactly
    w, vol = _points(rng, grid, 4000)
    axis = rng.integers(0, 3, len(w))
    rows = np.arange(len(w))
    m = np.floor(((w[rows, axis] + F32(1.)) * F32(.5)) * s0 + bias0[vol, axis]).astype(F32)
    p01 = ((m - bias0[vol, axis]) / s0).astype(F32)
    w[rows, axis] = (p01 * F32(2.) - F32(1.)).astype(F32)
    q = (((w + F32(1.)) * F32(.5)).astype(F32) * s0 + bias0[vol]).astype(F32)
    on_face = q[rows, axis] == np.floor(q[rows, axis])
    assert on_face.sum() >= 200
    w, vol, axis = w[on_face][:300], vol[on_face][:300], axis[on_face][:300]
    c = dr.field_chain(grid, params, w, vol)
    assert (c["cells"].frac(w, F32)[np.arange(len(w)), 0, axis] == 0).all()
    keep = ~c["ties"]
    assert (~keep).mean() <= 0.01
    _, g = emul_density_grad(emul, grid, params, w, vol, c["x_h"])
    disc, err = dr.rel_err(c["g32"], c["g"], c["S_g"], keep), dr.rel_err(g, c["g"], c["S_g"], keep)
    print("faces: %d points, discrepancy %.3g, bar %.3g, kernel %.3g" % (len(w), disc, 8 * disc, err))
    assert err <= 8.0 * disc
    # -- saturation
    w, vol = _points(rng, grid, 300, -6.0, -3.5)  # (the biases are positive and below ~1100: the fine levels go negative here)
    c = dr.field_chain(grid, params, w, vol)
    q0 = c["cells"].fl[:, 15]
    assert (q0 < 0).any(1).mean() > 0.5 and (c["cells"].fl[:, 0] >= 0).any()  # saturated and ordinary levels side by side
    keep = ~c["ties"]
    assert (~keep).mean() <= 0.01
    _, g = emul_density_grad(emul, grid, params, w, vol, c["x_h"])
    disc, err = dr.rel_err(c["g32"], c["g"], c["S_g"], keep), dr.rel_err(g, c["g"], c["S_g"], keep)
    print("saturation: %d points (%d with q_15 < 0), discrepancy %.3g, bar %.3g, kernel %.3g" % (len(w), (q0 < 0).any(1).sum(), disc, 8 * disc, err))
    assert np.isfinite(g).all() and err <= 8.0 * disc


def test_density_grad_scatter_on_the_emulator(emul, fox_state):
    """f2n_density_grad_scatter: exact zeros for the empty points; sigma (f2n_density_scatter's bits) and sigma J^T g of the restatement
    for the others, J = the oracle's Jacobian, bar 8 x the restatement's float32-vs-float64 discrepancy.  Measured: discrepancy 1.33e-7,
    bar 1.06e-6, kernel 1.33e-7.  The optional normals are -grad / |grad|, 0 for the empty points."""
    st = fox_state
    rng = np.random.default_rng(31)
    tr = np.ascontiguousarray(st["pers_trans"]).view(np.uint8).reshape(-1, 544)
    centers = np.ascontiguousarray(tr[:, 528:540]).view(F32).reshape(-1, 3)
    n = 333
    t = rng.integers(0, len(tr), n).astype(np.int32)
    pts = (centers[t] + rng.uniform(-0.02, 0.02, (n, 3))).astype(F32)
    empty = rng.random(n) < 0.3
    anchors = np.stack([np.where(empty, -1, t), np.where(empty, -1, rng.integers(0, 1000, n)), np.zeros(n, np.int64)], 1).astype(np.int32)
    se = np.zeros((n, 2), np.int32)
    se[:, 1] = np.cumsum(~empty)
    se[:, 0] = se[:, 1] - (~empty)
    m = int((~empty).sum())
    assert 0 < m < n
    f0 = rng.uniform(-2.0, 9.0, m).astype(F32)
    g = (rng.standard_normal((m, 3)) * 50).astype(F32)
    dens, grad, nrm, dens0 = np.full(n, np.nan, F32), np.full((n, 3), np.nan, F32), np.full((n, 3), np.nan, F32), np.full(n, np.nan, F32)
    args = (None, n, _vp(pts), _vp(anchors), _vp(se), _vp(tr), _vp(f0), _vp(g), _vp(dens), _vp(grad))
    assert emul.f2n_density_grad_scatter(*args, _vp(nrm)) == 0
    assert emul.f2n_density_scatter(None, n, _vp(anchors), _vp(se), _vp(f0), _vp(dens0)) == 0
    assert (dens.view(np.uint32) == dens0.view(np.uint32)).all()
    assert (dens[empty] == 0).all() and (grad[empty] == 0).all() and (nrm[empty] == 0).all()
    _, jac = oc.warp(st["pers_trans"], t[~empty], pts[~empty])
    assert np.isfinite(jac).all()
    ref64, S = dr.grad_sigma(dens[~empty], jac, g, F64)
    ref32, _ = dr.grad_sigma(dens[~empty], jac, g, F32)
    disc, err = dr.rel_err(ref32, ref64, S), dr.rel_err(grad[~empty], ref64, S)
    print("scatter: %d of %d points non-empty, discrepancy %.3g, bar %.3g, kernel %.3g" % (m, n, disc, 8 * disc, err))
    assert err <= 8.0 * disc
    ln = np.sqrt((grad[~empty].astype(F64) ** 2).sum(1))
    assert (ln > 0).all()
    assert np.abs(nrm[~empty] + grad[~empty] / ln[:, None]).max() < 1e-6
    grad2 = np.full((n, 3), np.nan, F32)
    assert emul.f2n_density_grad_scatter(None, n, _vp(pts), _vp(anchors), _vp(se), _vp(tr), _vp(f0), _vp(g), _vp(dens), _vp(grad2), None) == 0
    assert (grad2.view(np.uint32) == grad.view(np.uint32)).all()


def test_normal_source_option_parses_and_defaults():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    assert mesh.options(config.preset("wanjinyou", []))["normal_source"] == "grid"
    assert mesh.options(config.preset("wanjinyou", ["mesh.normals=true"]))["normal_source"] == "grid"
    assert mesh.options(config.preset("wanjinyou", ["mesh.normal_source=field"]))["normal_source"] == "field"
    assert mesh.options(config.preset("wanjinyou", ["mesh.normal_source=grid", "mesh.normals=true"]))["normal_source"] == "grid"
    for bad in ("mesh", "Field normals", "true", ""):
        with pytest.raises(ValueError) as e:
            mesh.options(config.preset("wanjinyou", ["mesh.normal_source=%s" % bad]))
        assert "grid" in str(e.value) and "field" in str(e.value)
