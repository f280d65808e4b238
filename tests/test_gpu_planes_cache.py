"""GPU (run with `-m gpu`): the gather's planes as the feature cache of a streaming train step.

The large-batch density pre-pass gathers the hash features as f16 planes [8][rows][4] and the plane-fed MLP used to write them a
second time as rows [n,32] for the field backward of the same step.  With ExpRunner.prepass_planes_cache (the default) the planes
themselves are kept, the row copy is not written (f2n_field_mlp_planes_ex with save_x_h = NULL) and the field backward reads the
planes (f2n_field_bwd_dyn_planes / f2n_field_bwd_step_tail_planes).  Only where the two 8-byte pieces of a row fragment are loaded
from differs, so everything here is bit for bit: there is no tolerance.

The planes of the kernel-level tests hold the f16 NaN pattern in every row that the call has no business reading, have more rows
than the call is told about samples (plane_rows = n + 13) and start 6 rows before the survivors' base: a wrong stride, a wrong
offset or a read of an unnamed row cannot give finite, equal results.  The gradient table is compared under the condition of
tests/test_gpu_feat_reuse.py (its module docstring): product numerics, and the owner-binned scatter or a single sample.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import capi as oc  # noqa: E402
from test_gpu_parity import DEV, F32, N, T, assert_same, grid_dev, make_grid, rand_params  # noqa: E402
from test_gpu_feat_reuse import checksums, h16, row_sets  # noqa: E402

SIZES = [1, 15, 16, 17, 50, 240, 1500]  # tile edges, a partial last tile, several tiles per wave, several blocks
PREPASS_SIZES = [1, 15, 16, 17, 240, 1500, 262227]  # the last: 2048 blocks x 4 waves x 16 samples = 131072 samples per round of the
#                                                     grid, so waves with three rounds, waves with two, and a partial last tile
LOG2 = 14
CAP = 32768  # F2N_BIN_MIN_N: capacities from here on take the owner-binned scatter
PAD, BASE = 13, 6  # plane_rows = n + PAD; the survivors' rows start at plane row BASE, the edge samples' at plane row 0
NAN16 = np.uint16(0x7e00)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import capi
    capi.lib()
    if "F2N_EXPECT_NUMERICS" in os.environ:  # (the child process of the reference-numerics test below: it must have got that library)
        assert capi.lib().f2n_numerics_mode() == int(os.environ["F2N_EXPECT_NUMERICS"])
    return capi


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    runtime.host()
    return runtime


@pytest.fixture(scope="module")
def field_net():
    return T(oc.f2h(rand_params(np.random.default_rng(71), 1)).view(np.float16))


def planes_with_nan(n, cache_np, rows, edge_np):
    """Flat f16 planes [8][n + PAD][4], NaN everywhere but: plane row BASE + r for every r in rows = cache row r, and (edge_np
    given) plane row s = edge row s.  Returns the device tensor and its row count."""
    pr = n + PAD
    pl = np.full((8, pr, 4), NAN16, np.uint16)
    pl[:, BASE + rows, :] = cache_np[rows].view(np.uint16).reshape(len(rows), 8, 4).transpose(1, 0, 2)
    if edge_np is not None and len(edge_np):
        assert len(edge_np) <= BASE
        pl[:, :len(edge_np), :] = edge_np.view(np.uint16).reshape(len(edge_np), 8, 4).transpose(1, 0, 2)
    return T(pl.view(np.float16).reshape(-1)), pr


def bwd_inputs(rng, g, cap):
    pick = rng.integers(0, len(g["march_pts"]), cap)
    return (T(g["march_pts"][pick]), T(np.ascontiguousarray(g["march_anchors"][pick, 0])),
            T((rng.standard_normal((cap, 16)) * 1e-3).astype(F32)))


def run_bwd(hip, gd, grid, cap, n_dev, n_off, pts, vol, ph, dfeat, x_edge, rows, cache=None, planes=None, plane_rows=0, edge_in_planes=False):
    dW = torch.zeros(3072, device=DEV)
    gtab = torch.zeros(grid.table_f32.size, dtype=torch.float16, device=DEV)
    hip.deferred_reset()
    head = (cap, n_dev, n_off, grid.n_volumes, gd["prim"], gd["lidx"], gd["lsize"], gd["bias"], gd["scale"], pts, vol, 1, ph)
    tail = (dfeat, 128.0, dW, gtab, 1 << LOG2, 1)
    if planes is None:
        hip.field_bwd_dyn_rows(*head, x_edge, cache, rows, *tail)
    else:
        hip.field_bwd_dyn_planes(*head, None if edge_in_planes else x_edge, planes if edge_in_planes else None, planes[4 * BASE:], plane_rows,
                                 rows, *tail)
    hip.reduce_deferred()
    torch.cuda.synchronize()
    return N(dW), h16(gtab)


@pytest.mark.parametrize("n", SIZES)
def test_field_backward_on_planes(hip, fox_state, fox_golden, field_net, n):
    """f2n_field_bwd_dyn_planes on (edge rows or edge plane rows, planes, src_rows) == f2n_field_bwd_dyn_rows on the row-major array
    of the same features: the weight gradients after f2n_reduce_deferred and the gradient table; finite although every plane row that
    is not named holds NaN."""
    g = fox_golden
    rng = np.random.default_rng(300 + n)
    grid = make_grid(fox_state, rng, LOG2, scale=0.5)
    gd = grid_dev(grid)
    cache_np = (rng.standard_normal((n, 32)) * 0.5).astype(np.float16)
    cache = T(cache_np)
    for name, rows in row_sets(rng, n):
        m = len(rows)
        for n_off in (0, 6):
            edge_np = (rng.standard_normal((n_off, 32)) * 0.5).astype(np.float16)
            x_edge = T(edge_np) if n_off else None
            for cap in (CAP, m + n_off + 3):
                pts, vol, dfeat = bwd_inputs(rng, g, cap)
                d_rows = T(np.concatenate([rows, np.zeros(cap - n_off - m, np.int32)]))
                n_dev = torch.tensor([m], dtype=torch.int32, device=DEV)
                want = run_bwd(hip, gd, grid, cap, n_dev, n_off, pts, vol, field_net, dfeat, x_edge, d_rows, cache=cache)
                assert np.abs(want[0]).max() > 0 and np.isfinite(want[0]).all()
                for edge_in_planes in ((False, True) if n_off else (False,)):
                    planes, pr = planes_with_nan(n, cache_np, rows, edge_np if edge_in_planes else None)
                    got = run_bwd(hip, gd, grid, cap, n_dev, n_off, pts, vol, field_net, dfeat, x_edge, d_rows, planes=planes, plane_rows=pr,
                                  edge_in_planes=edge_in_planes)
                    what = "n=%d rows=%s n_off=%d capacity=%d edge rows from %s: " % (n, name, n_off, cap, "planes" if edge_in_planes else "x_edge_h")
                    assert np.isfinite(got[0]).all(), what + "dW is not finite"
                    assert np.isfinite(got[1].view(np.float16).astype(F32)).all(), what + "the gradient table is not finite"
                    assert_same(got[0], want[0], what + "dW")
                    if hip.lib().f2n_numerics_mode() == 0 and (cap >= CAP or m + n_off == 1):
                        assert (want[1] != 0).any(), what
                        assert_same(got[1], want[1], what + "gradient table")


@pytest.mark.parametrize("n", [240, 1500])
def test_step_tail_on_planes(hip, fox_state, fox_golden, field_net, n):
    """f2n_field_bwd_step_tail_planes == f2n_field_bwd_step_tail_rows: every parameter, moment, f16 working copy and flag of the step's
    tail (the two small groups and the hash table), and the cleared gradient buffers."""
    g = fox_golden
    rng = np.random.default_rng(400 + n)
    grid = make_grid(fox_state, rng, LOG2, scale=0.5)
    gd = grid_dev(grid)
    cache_np = (rng.standard_normal((n, 32)) * 0.5).astype(np.float16)
    rows = row_sets(rng, n)[0][1]
    m, n_off = len(rows), 6
    edge_np = (rng.standard_normal((n_off, 32)) * 0.5).astype(np.float16)
    n_tab, n_full = 17 << LOG2, grid.table_f32.size
    sizes = (3072, 7168)
    base = [dict(p=rng.standard_normal(k).astype(F32), m=rng.standard_normal(k).astype(F32) * F32(0.1), v=rng.random(k, dtype=F32) * F32(0.01)) for k in sizes]
    g_pre = (rng.standard_normal(sizes[1]) * 0.1).astype(F32)
    tab = dict(p=(rng.standard_normal(n_full) * 1e-2).astype(F32), m=(rng.standard_normal(n_full) * 1e-3).astype(F32), v=rng.random(n_full, dtype=F32) * F32(1e-6))
    for cap in (CAP, m + n_off + 3):
        pts, vol, dfeat = bwd_inputs(rng, g, cap)
        d_rows = T(np.concatenate([rows, np.zeros(cap - n_off - m, np.int32)]))
        n_dev = torch.tensor([m], dtype=torch.int32, device=DEV)
        out = []
        for form in ("rows", "planes, edge rows from x_edge_h", "planes, edge rows from planes"):
            grp = [{k: T(v) for k, v in b.items()} for b in base]
            grads = [torch.zeros(sizes[0], device=DEV), T(g_pre)]
            hs = [torch.zeros(k, dtype=torch.float16, device=DEV) for k in sizes]
            tb = {k: T(v) for k, v in tab.items()}
            th = T(oc.f2h(tab["p"]).view(np.float16))
            gtab = torch.zeros(n_full, dtype=torch.float16, device=DEV)
            flags = torch.full((4,), -7, dtype=torch.int32, device=DEV)
            groups = [dict(param=grp[k]["p"], grad=grads[k], exp_avg=grp[k]["m"], exp_avg_sq=grp[k]["v"], param_h=hs[k], grad_scale=1.0 / 128,
                           weight_decay=1e-6, grad_round_h16=True) for k in range(2)]
            table = dict(param=tb["p"], exp_avg=tb["m"], exp_avg_sq=tb["v"], param_h=th, grad_scale=1.0 / 128, n=n_tab)
            head = (cap, n_dev, n_off, grid.n_volumes, gd["prim"], gd["lidx"], gd["lsize"], gd["bias"], gd["scale"], pts, vol, 1, field_net)
            mid = (dfeat, 128.0, grads[0], gtab, 1 << LOG2, grads[0], grads[1], flags, groups, table, 7, 3e-3, 0.9, 0.99, 1e-15)
            hip.deferred_reset()
            if form == "rows":
                by_owners = hip.field_bwd_step_tail(*head, T(edge_np), *mid, x_cache_h=T(cache_np), src_rows=d_rows)
            else:
                in_planes = form.endswith("from planes")
                planes, pr = planes_with_nan(n, cache_np, rows, edge_np if in_planes else None)
                by_owners = hip.field_bwd_step_tail(*head, None if in_planes else T(edge_np), *mid, x_cache_h=planes[4 * BASE:], src_rows=d_rows,
                                                    plane_rows=pr, x_edge_planes_h=planes if in_planes else None)
            torch.cuda.synchronize()
            out.append((form, by_owners, N(flags), [{k: N(v) for k, v in gk.items()} for gk in grp], [h16(h) for h in hs], [N(x) for x in grads],
                        {k: N(v) for k, v in tb.items()}, h16(th), h16(gtab)))
        want = out[0]
        assert int(want[2][2]) == 0  # the step was applied
        if hip.lib().f2n_numerics_mode() == 0:
            assert want[1] == (1 if cap >= CAP else 0)  # the owners of the binned scatter stepped the table
        assert any((want[3][0]["p"] != base[0]["p"]).ravel()) and (want[6]["p"] != tab["p"]).any()
        for got in out[1:]:
            what = "n=%d capacity=%d %s: " % (n, cap, got[0])
            assert got[1] == want[1], what + "table stepped by the owners"
            assert (got[2][:3] == want[2][:3]).all(), what + "flags"
            for k in range(2):
                for key in ("p", "m", "v"):
                    assert np.isfinite(got[3][k][key]).all(), what
                    assert_same(got[3][k][key], want[3][k][key], what + "group %d %s" % (k, key))
                assert_same(got[4][k], want[4][k], what + "group %d f16 copy" % k)
                assert (got[5][k] == 0).all() and (want[5][k] == 0).all(), what + "zero_grad"
            if hip.lib().f2n_numerics_mode() == 0 and cap >= CAP:
                for key in ("p", "m", "v"):
                    assert np.isfinite(got[6][key]).all(), what
                    assert_same(got[6][key], want[6][key], what + "table " + key)
                assert_same(got[7], want[7], what + "table f16 copy")
                assert (got[8] == 0).all() and (want[8] == 0).all(), what + "gradient table cleared"


@pytest.mark.parametrize("n", PREPASS_SIZES)
def test_prepass_mlp_without_the_row_copy(hip, field_net, n):
    """f2n_field_mlp_planes_ex with save_x_h = NULL == the same call with it (f0, out_feat_h), and both == f2n_field_fwd_cached on the
    rows (the route that did not change): out_feat_h is the f16 rounding of its fp32 rows, f0 its column 0; the saved rows are the
    planes' contents."""
    rng = np.random.default_rng(500 + n % 1000)
    x = (rng.standard_normal((n, 32)) * 0.5).astype(np.float16)
    planes = T(np.ascontiguousarray(x.reshape(n, 8, 4).transpose(1, 0, 2)))
    out = []
    for save in (True, False):
        cache = torch.zeros((n, 32), dtype=torch.float16, device=DEV) if save else None
        feat_h = torch.full((n, 16), -7.0, dtype=torch.float16, device=DEV)
        f0 = torch.full((n,), -7.0, device=DEV)
        hip.field_mlp_planes_ex(n, planes, field_net, None, f0, cache, feat_h)
        out.append((N(f0), h16(feat_h)))
        if save:
            assert_same(h16(cache), x.view(np.uint16), "n=%d: saved rows" % n)
    assert_same(out[1][0], out[0][0], "n=%d: f0 without / with save_x_h" % n)
    assert_same(out[1][1], out[0][1], "n=%d: out_feat_h without / with save_x_h" % n)
    feat = torch.zeros((n, 16), device=DEV)
    f0c = torch.zeros(n, device=DEV)
    hip.field_fwd_cached(n, n, None, T(x), field_net, feat, f0c, None)
    assert float(feat.abs().max()) > 0
    for f0, fh in out:
        assert_same(fh, h16(feat.to(torch.float16)), "n=%d: out_feat_h against field_fwd_cached" % n)
        assert_same(N(torch.from_numpy(fh.view(np.float16)).float()), N(feat), "n=%d: widened" % n)
        assert_same(f0, N(f0c), "n=%d: f0 against field_fwd_cached" % n)
    # the fp32 rows of the plane-fed call itself (out_feat_f32, which the pre-pass does not ask for)
    feat2 = torch.zeros((n, 16), device=DEV)
    hip.field_mlp_planes_ex(n, planes, field_net, feat2, None, None, None)
    assert_same(N(feat2), N(feat), "n=%d: out_feat_f32" % n)


KERNEL_TESTS = "field_backward_on_planes or step_tail_on_planes or prepass_mlp_without"
N_KERNEL_TESTS = len(SIZES) + 2 + len(PREPASS_SIZES)


def test_kernel_level_equalities_hold_in_the_reference_numerics_build():
    """Both library builds take the change: the kernel-level tests above again, in a child process that loads the
    reference-numerics library (a process has one numerics, chosen by the environment before the package is imported)."""
    env = dict(os.environ, F2N_REFERENCE_NUMERICS="1", F2N_EXPECT_NUMERICS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        KERNEL_TESTS], capture_output=True, text=True, env=env, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "%d passed" % N_KERNEL_TESTS in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("mode", ["default", "fused_tail"])
def test_train_steps_are_bit_identical_with_planes_and_with_rows(rt, fox_state, mode):
    """Two runners from one seed, ExpRunner.prepass_planes_cache on and off, three streaming steps at 512 rays: equal integer
    checksums of table and both MLPs, equal losses; every step took the reuse path in both."""
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 512, rng)) for _ in range(4)]
    outs = {}
    for planes in (True, False):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", [], seed=2022, device="cuda:0")
        torch.manual_seed(2022)
        assert runner.prepass_planes_cache is True and runner.prepass_feat_reuse is True  # the defaults
        runner.prepass_planes_cache = planes
        if mode == "fused_tail":
            runner.fused_tail = 1
        losses = []
        for i in range(3):
            b, nb = batches[i], batches[i + 1]
            s = runner.train_step(b[0], b[1], b[2], b[3], b[4], True, nb[0], nb[1], nb[2])
            assert s["n_samples"] >= 32768, s["n_samples"]  # (the planes route of the pre-pass, the owner-binned scatter)
            losses.append(float(s["loss"]))
        runner.flush()
        assert runner.prepass_reuse_steps == 3
        outs[planes] = (checksums(runner), losses)
        del runner
    assert outs[True][0] == outs[False][0], (mode, outs)
    assert outs[True][1] == outs[False][1] and all(x == x for x in outs[True][1]), (mode, outs)


def test_world_space_queries_leave_the_planes_cache(rt, fox_state):
    """A world-space query between a pre-pass that kept planes and its consumer (PrepassCacheGuard): the planes and the field outputs
    are the same arrays with the same contents afterwards, and no row cache has appeared."""
    runner, cfg, _ = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    world = torch.rand((4096, 3), device="cuda:0", generator=gen) * 2.0 - 1.0
    warped, anchors = runner.locate_points(world)
    inside = torch.nonzero(anchors[:, 0] >= 0).flatten()
    assert inside.numel() >= 64
    pick = inside[torch.arange(40000, device="cuda:0") % inside.numel()]  # (the planes route starts at 32768 points)
    w, a = warped[pick].contiguous(), anchors[pick, 0].contiguous()
    f0 = runner.density_prepass_planes(w, a)
    n = f0.shape[0]
    pl = runner.prepass_planes()
    x, fh = runner.prepass_caches()
    assert pl.shape == (8, n, 4) and x.numel() == 0 and fh.shape == (n, 16)
    assert torch.equal(fh[:, 0].float(), f0)
    f0_rows = runner.density_prepass(w, a, True)  # the unchanged binding: rows, no planes
    x_rows, _ = runner.prepass_caches()
    assert runner.prepass_planes().numel() == 0 and x_rows.shape == (n, 32) and torch.equal(f0_rows, f0)
    rows_of_planes = pl.permute(1, 0, 2).reshape(n, 32)
    assert torch.equal(rows_of_planes.view(torch.int16), x_rows.view(torch.int16))  # the planes hold what the rows hold
    del x_rows
    runner.density_prepass_planes(w, a)
    pl = runner.prepass_planes()
    _, fh = runner.prepass_caches()
    pl0, fh0 = pl.clone(), fh.clone()
    dirs = torch.nn.functional.normalize(torch.rand((4096, 3), device="cuda:0", generator=gen) - 0.5, dim=1)
    runner.query_density(world)
    runner.query_radiance(world, dirs)
    runner.query_density_grad(world)
    pl1 = runner.prepass_planes()
    x1, fh1 = runner.prepass_caches()
    assert pl1.data_ptr() == pl.data_ptr() and fh1.data_ptr() == fh.data_ptr() and pl1.shape == pl.shape and fh1.shape == fh.shape
    assert x1.numel() == 0
    assert torch.equal(pl1.view(torch.int16), pl0.view(torch.int16)) and torch.equal(fh1.view(torch.int16), fh0.view(torch.int16))
