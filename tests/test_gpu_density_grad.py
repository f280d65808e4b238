"""The analytic density gradient on the MI355X (csrc/field.hip, csrc/octree.hip, host/RendererQuery.cpp): the kernels and
runner.query_density_grad against the float64 restatement (tests/density_grad_ref.py), a field shape without the fused kernels, the mesh
export with normal_source="field", and no effect on training.

Error metric: max_i |g_i - g_ref64,i| / S_i (S = the sum of the absolute values of all addends of the component); bar: 8 x the
restatement's own float32-vs-float64 discrepancy on the same inputs, computed on the CPU inside the test; points with a ReLU tie are left
out, at most 1 % may be (tests/test_density_grad_cpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import density_grad_ref as dr  # noqa: E402
from oracle import capi as oc, pipeline as op  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
BOX = ([-1.0, -0.8, -0.9], [1.0, 0.7, 1.05])


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def fox_runner(rt, fox_state):
    runner, cfg, arrays = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    return runner, arrays


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _same_bits(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def _grid_of(arrays):
    return op.HashGrid(arrays[4], arrays[5], arrays[6], int(arrays[7][0]), 14)


def _device_grad(grid, params, w, vol, x_h, want_dx=True):
    from f2_nerf_amd import capi
    n = len(w)
    gd = dict(table=_dev(grid.table_h.view(np.float16), np.float16), prim=_dev(grid.prim_pool, np.int32), lidx=_dev(grid.local_idx, np.int32),
              lsize=_dev(grid.local_size, np.int32), bias=_dev(grid.bias_pool, F32), scale=_dev(grid.scales, F32))
    ph = _dev(oc.f2h(params).view(np.float16), np.float16)
    wd, vd, xd = _dev(w, F32), _dev(vol, np.int32), _dev(np.asarray(x_h, np.uint16).view(np.float16), np.float16)
    hargs = (n, grid.n_volumes, gd["table"], gd["prim"], gd["lidx"], gd["lsize"], gd["bias"], gd["scale"], wd, vd, 1)
    dx = torch.full((n, 32), float("nan"), device="cuda") if want_dx else None
    g = torch.full((n, 3), float("nan"), device="cuda")
    capi.field_density_grad(*hargs, ph, xd, dx, g)
    g2 = None
    if want_dx:
        g2 = torch.full((n, 3), float("nan"), device="cuda")
        capi.hash_pos_grad(*hargs, dx, g2)
        g2 = g2.cpu().numpy()
    return (dx.cpu().numpy() if want_dx else None), g.cpu().numpy(), g2


@pytest.mark.parametrize("n", [65, 4097, 20000, 50000])  # one ragged tile; several tiles, constants from memory; constants staged in LDS
def test_kernels_match_the_restatement(fox_runner, n):
    """f2n_field_density_grad / f2n_hash_pos_grad fed the oracle's x_h; the test prints discrepancy, bar and device error.  With the
    emulated wavefront as the device (restatement float32-vs-float64 discrepancy -> bar; error): df0/dw n = 65: 4.94e-6 -> 3.95e-5;
    4.94e-6, n = 4097: 2.07e-5 -> 1.66e-4; 2.07e-5; df0/dx 1.41e-7 -> 1.13e-6; 1.41e-7 and 2.1e-7 -> 1.68e-6; 2.1e-7."""
    _, arrays = fox_runner
    grid, params = _grid_of(arrays), np.asarray(arrays[8], F32)
    rng = np.random.default_rng(200 + n)
    w = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    vol = rng.integers(0, grid.n_volumes, n).astype(np.int32)
    c = dr.field_chain(grid, params, w, vol)
    keep = ~c["ties"]
    assert (~keep).mean() <= 0.01
    dx, g, g2 = _device_grad(grid, params, w, vol, c["x_h"])
    assert np.isfinite(dx).all() and np.isfinite(g).all()
    for name, got, ref32, ref64, S in (("df0/dx", dx, c["dx32"], c["dx"], c["S_dx"]), ("df0/dw", g, c["g32"], c["g"], c["S_g"])):
        disc, err = dr.rel_err(ref32, ref64, S, keep), dr.rel_err(got, ref64, S, keep)
        print("n = %d %s: restatement f32-vs-f64 %.3g, bar %.3g, device %.3g, left out %.5f" % (n, name, disc, 8 * disc, err, (~keep).mean()))
        assert err <= 8.0 * disc, (name, err, 8.0 * disc)
    assert _same_bits(g2, g)  # out_dx is what f2n_hash_pos_grad takes
    dx3, g3, _ = _device_grad(grid, params, w, vol, c["x_h"])  # a second call: the same bits
    assert _same_bits(dx3, dx) and _same_bits(g3, g)
    assert _same_bits(_device_grad(grid, params, w, vol, c["x_h"], want_dx=False)[1], g)


def _restated_world_grad(st, grid, params, pts, anchors, dens, d_hidden=64, dx_of=None):
    """(ref64, ref32, S, keep) of the world-space gradient at the non-empty points: oc.warp on the located anchors, oracle features."""
    t = np.ascontiguousarray(anchors[:, 0])
    ref_w, jac = oc.warp(st["pers_trans"], t, pts)
    c = dr.field_chain(grid, params, ref_w, t, d_hidden=d_hidden)
    g32 = c["g32"] if dx_of is None else dr.df0_dw(c["cells"], dx_of(c), F32)[0]
    ref64, S = dr.grad_sigma(dens, jac, c["g"], F64, c["S_g"])
    ref32, _ = dr.grad_sigma(dens, jac, g32, F32)
    return ref64, ref32, S, ~c["ties"]


def test_query_density_grad_on_the_fox(fox_runner, fox_state):
    """runner.query_density_grad at 20000 points uniform in [-1.1, 1.1]^3 (empty and non-empty ones)."""
    runner, arrays = fox_runner
    n = 20000
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1.1, 1.1, (n, 3)).astype(F32)
    pd = torch.from_numpy(pts).cuda()
    dens, grad = (x.cpu().numpy() for x in runner.query_density_grad(pd))
    assert dens.shape == (n,) and grad.shape == (n, 3) and dens.dtype == F32 and grad.dtype == F32
    assert _same_bits(dens, runner.query_density(pd).cpu().numpy())  # the density of query_density, bit for bit
    a = runner.locate_points(pd)[1].cpu().numpy()
    empty = a[:, 0] < 0
    assert 0 < empty.sum() < n  # both kinds of points
    assert (dens[empty] == 0).all() and (grad[empty] == 0).all()
    ref64, ref32, S, keep = _restated_world_grad(fox_state, _grid_of(arrays), np.asarray(arrays[8], F32), pts[~empty], a[~empty], dens[~empty])
    assert (~keep).mean() <= 0.01
    disc, err = dr.rel_err(ref32, ref64, S, keep), dr.rel_err(grad[~empty], ref64, S, keep)
    print("%d non-empty points: restatement f32-vs-f64 %.3g, bar %.3g, device %.3g, left out %.5f" % ((~empty).sum(), disc, 8 * disc, err, (~keep).mean()))
    assert err <= 8.0 * disc, (err, 8.0 * disc)
    assert (np.ptp(grad, axis=0) > 0).all()  # a gradient field that varies
    d2, g2 = (x.cpu().numpy() for x in runner.query_density_grad(pd))  # a second call: the same bits
    assert _same_bits(d2, dens) and _same_bits(g2, grad)
    # field_normals: -grad / |grad|, zero where the gradient is
    nrm = runner.field_normals(pd).cpu().numpy()
    ln = np.sqrt((grad.astype(F64) ** 2).sum(1))
    assert (nrm[ln == 0] == 0).all() and (nrm[empty] == 0).all()
    mid = (ln > 1e-18) & (ln < 1e18)  # (outside, the float32 length under- or overflows: the kernel's to judge)
    assert mid.sum() > 1000 and np.abs(nrm[mid] + grad[mid] / ln[mid, None]).max() < 1e-5
    # all points empty, and no points
    d0, g0 = runner.query_density_grad(torch.full((7, 3), 1000.0, device="cuda"))
    assert tuple(d0.shape) == (7,) and (d0 == 0).all() and (g0 == 0).all()
    d0, g0 = runner.query_density_grad(torch.zeros((0, 3), device="cuda"))
    assert tuple(d0.shape) == (0,) and tuple(g0.shape) == (0, 3)
    assert tuple(runner.field_normals(torch.zeros((0, 3), device="cuda")).shape) == (0, 3)


def test_a_field_shape_without_the_fused_kernels(rt, fox_state):
    """field.mlp_hidden_dim=32: df0/dx comes from f2n_mlp_bwd (dy = e_0, loss scale 1), whose hidden gradients are h16.  Bar: 8 x the
    discrepancy between the restatement fed the oracle's mlp_bwd dx and the float64 restatement."""
    runner, cfg, arrays = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14", "field.mlp_hidden_dim=32"], seed=1, table_init=0.3)
    params = np.asarray(arrays[8], F32)
    assert len(params) == 32 * 32 + 16 * 32
    n = 5000
    rng = np.random.default_rng(8)
    pts = rng.uniform(-1.1, 1.1, (n, 3)).astype(F32)
    pd = torch.from_numpy(pts).cuda()
    dens, grad = (x.cpu().numpy() for x in runner.query_density_grad(pd))
    assert _same_bits(dens, runner.query_density(pd).cpu().numpy())
    a = runner.locate_points(pd)[1].cpu().numpy()
    empty = a[:, 0] < 0
    assert 0 < empty.sum() < n and (grad[empty] == 0).all()

    def oracle_dx(c):
        x = oc.h2f(c["x_h"])
        _, acts = oc.mlp_fwd(params, x, 32, 1, want_acts=True)
        dy = np.zeros((len(x), 16), F32)
        dy[:, 0] = 1
        return oc.mlp_bwd(params, x, acts, dy, 32, 1, 1.0)[1]

    ref64, ref32, S, keep = _restated_world_grad(fox_state, _grid_of(arrays), params, pts[~empty], a[~empty], dens[~empty], 32, oracle_dx)
    assert (~keep).mean() <= 0.01
    disc, err = dr.rel_err(ref32, ref64, S, keep), dr.rel_err(grad[~empty], ref64, S, keep)
    print("hidden width 32, %d non-empty points: oracle-dx restatement vs float64 %.3g, bar %.3g, device %.3g" % ((~empty).sum(), disc, 8 * disc, err))
    assert err <= 8.0 * disc, (err, 8.0 * disc)
    assert (np.ptp(grad, axis=0) > 0).all()


def _view_dirs(normals):
    flat = (normals == 0).all(1)
    return np.where(flat[:, None], np.array([0.0, 0.0, -1.0], F32), -normals).astype(F32)


def test_extract_mesh_attrs_with_field_normals(rt, fox_runner):
    runner, _ = fox_runner
    lo, hi = BOX
    res = 64
    g = runner.density_grid(lo, hi, res)
    gn = g.cpu().numpy()
    level = float(np.quantile(gn[gn > 0], 0.5))  # a level the scene crosses
    step = rt.host().grid_spec(lo, hi, res)[0]
    base = {k: v.cpu().numpy() for k, v in runner.extract_mesh_attrs(lo, hi, res, level).items()}
    grid_m = {k: v.cpu().numpy() for k, v in runner.extract_mesh_attrs(lo, hi, res, level, normal_source="grid").items()}
    assert sorted(base) == ["colors", "faces", "normals", "verts"]
    for k in base:  # the default is the grid source: what the export did before the option existed
        assert base[k].shape == grid_m[k].shape and (base[k].view(np.uint8) == grid_m[k].view(np.uint8)).all(), k
    vd = torch.from_numpy(base["verts"]).cuda()
    grid_n = rt.host().grid_normals(g, vd, lo, step).cpu().numpy()
    assert _same_bits(base["normals"], grid_n)
    assert _same_bits(base["colors"], runner.query_radiance(vd, torch.from_numpy(_view_dirs(grid_n)).cuda())[1].cpu().numpy())
    m = {k: v.cpu().numpy() for k, v in runner.extract_mesh_attrs(lo, hi, res, level, 0, True, True, "field").items()}
    assert len(m["faces"]) > 1000
    assert _same_bits(m["verts"], base["verts"]) and (m["faces"] == base["faces"]).all()
    fn = runner.field_normals(vd).cpu().numpy()
    zero = (fn == 0).all(1)
    assert _same_bits(m["normals"][~zero], fn[~zero]) and _same_bits(m["normals"][zero], grid_n[zero])
    ln = np.sqrt((m["normals"].astype(F64) ** 2).sum(1))
    assert ((np.abs(ln - 1) < 1e-5) | (ln == 0)).all() and (ln > 0).mean() > 0.99
    assert _same_bits(m["colors"], runner.query_radiance(vd, torch.from_numpy(_view_dirs(m["normals"])).cuda())[1].cpu().numpy())
    cos = (m["normals"].astype(F64) * grid_n).sum(1)
    print("fox %d^3: %d vertices, %d with a zero field normal, median cos(field normal, grid normal) = %.3f" % (res, len(fn), zero.sum(), np.median(cos)))
    assert sorted(runner.extract_mesh_attrs(lo, hi, res, level, 0, True, False, "field")) == ["faces", "normals", "verts"]
    with pytest.raises(RuntimeError):
        runner.extract_mesh_attrs(lo, hi, res, level, normal_source="mesh")


def test_density_grad_has_no_effect_on_training(rt, fox_state):
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 4096, rng)) for _ in range(6)]

    def run(query):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=15"], seed=3, table_init=0.3)
        runner.n_edge_pts = 512
        losses = []
        for k, b in enumerate(batches):
            if query and k == 3:
                p = torch.rand((1000, 3), device="cuda") * 2 - 1
                d, gr = runner.query_density_grad(p)
                assert (d > 0).any() and (gr != 0).any()
                g = runner.density_grid([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 48).cpu().numpy()
                level = float(np.quantile(g[g > 0], 0.5))  # a level the scene crosses
                m = runner.extract_mesh_attrs([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 48, level, min_component_faces=20, normal_source="field")
                assert len(m["faces"]) > 0 and m["normals"].shape == m["verts"].shape
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [t.detach().cpu().numpy().copy() for t in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))
