"""GPU (run with `-m gpu`): a streaming train step reuses the field outputs of its own density pre-pass.

The pre-pass and the grad pass of one step evaluate the field network on the same h16 hash features with the same weights, so the
grad pass takes the pre-pass's 16 f16 outputs (f2n_field_*_ex: out_feat_h) instead of running the network again
(f2n_shade_fwd_feat against f2n_field_shade_fwd_extra), and the field backward reads its input rows from the pre-pass cache through
the survivors' row index instead of from a copy (f2n_field_bwd_dyn_rows / f2n_field_bwd_step_tail_rows against the compact calls).
Everything here is bit-for-bit: there is no arithmetic that differs, so there is no tolerance.

Where a check is indirect:
  * dL/dx planes and the non-zero mask words of the field backward live in the library's private workspace.  They are compared
    through the gradient table that the owner-binned scatter -- integer sums, order-free -- makes of them: the calls run with a
    capacity of 32768 rows (what selects that scatter) and the device-side count n, the way a streaming step calls them.
  * the small-capacity variant of the kernel scatters with f16 atomics in arrival order: two runs of ONE program differ in low-order
    bits of the table wherever two addends meet.  There the MLP weight gradients (a function of every input row) are compared
    exactly, and the table only at n = 1, where no two samples can meet.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import capi as oc  # noqa: E402
from test_gpu_parity import DEV, F32, N, T, assert_same, grid_dev, make_grid, rand_params  # noqa: E402

SIZES = [1, 15, 16, 17, 50, 240, 1500]  # tile edges, a partial last tile, several tiles per wave (240 = 15 tiles), several blocks
LOG2 = 14
CAP = 32768  # F2N_BIN_MIN_N: capacities from here on take the owner-binned scatter


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import capi
    capi.lib()
    import os
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


def h16(t):
    return N(t).view(np.uint16)


def row_sets(rng, n):
    """(name, strictly increasing int32 rows of [0, n)): about 2/3 of the rows, all of them, the last one alone."""
    k = max(1, (2 * n + 2) // 3)
    return [("two thirds", np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)),
            ("identity", np.arange(n, dtype=np.int32)), ("last row", np.array([n - 1], np.int32))]


@pytest.fixture(scope="module")
def nets():
    rng = np.random.default_rng(71)
    pf, pc = rand_params(rng, 1), rand_params(rng, 2)
    return T(oc.f2h(pf).view(np.float16)), T(oc.f2h(pc).view(np.float16))


def prepass_from_planes(hip, phf, x):
    """x: f16 features [n,32] (numpy) -> (cache [n,32] h16, feat_h [n,16] h16, f0 [n]) of f2n_field_mlp_planes_ex."""
    n = len(x)
    planes = T(np.ascontiguousarray(x.reshape(n, 8, 4).transpose(1, 0, 2)))  # plane p = features 4p..4p+3 of every sample
    cache = torch.zeros((n, 32), dtype=torch.float16, device=DEV)
    feat_h = torch.zeros((n, 16), dtype=torch.float16, device=DEV)
    f0 = torch.zeros(n, device=DEV)
    hip.field_mlp_planes_ex(n, planes, phf, None, f0, cache, feat_h)
    return cache, feat_h, f0


@pytest.mark.parametrize("n", SIZES)
def test_colour_path_from_cached_field_outputs(hip, nets, n):
    """f2n_shade_fwd_feat == f2n_field_shade_fwd_extra: f0, shade_x, rgb and the extra rows' fp32 features, memcmp-equal; rows at and
    beyond the device-side count keep their sentinel."""
    phf, phc = nets
    rng = np.random.default_rng(100 + n)
    x = (rng.standard_normal((n, 32)) * 0.5).astype(np.float16)
    cache, feat_h, _ = prepass_from_planes(hip, phf, x)
    assert_same(h16(cache), x.view(np.uint16), "saved pre-pass rows")
    emb_tab = T((rng.standard_normal((50, 16)) * 0.1).astype(F32))
    for name, rows in row_sets(rng, n):
        m = len(rows)
        n_max = m + 5  # capacity above the device-side count
        d_rows = T(np.concatenate([rows, np.zeros(n_max - m, np.int32)]))
        dirs = rng.standard_normal((n_max, 3)).astype(F32)
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        d_dirs, sidx = T(dirs), T(rng.integers(0, 50, n_max).astype(np.int32))
        n_dev = torch.tensor([m], dtype=torch.int32, device=DEV)
        for use_emb in (False, True):
            for n_extra in (0, 6):
                ex = rng.integers(0, n, n_extra)
                ex_x, ex_f = (cache[ex].contiguous(), feat_h[ex].contiguous()) if n_extra else (None, None)
                out = []
                for reuse in (False, True):
                    f0 = torch.full((n_max,), -7.0, device=DEV)
                    rgb = torch.full((n_max, 3), -7.0, device=DEV)
                    sx = torch.full((n_max, 32), -7.0, dtype=torch.float16, device=DEV)
                    fe = torch.full((max(n_extra, 1), 16), -7.0, device=DEV)
                    emb = emb_tab if use_emb else None
                    if reuse:
                        hip.shade_fwd_feat(n_max, d_rows, feat_h, d_dirs, emb, sidx if use_emb else None, phc, f0, sx, rgb, n_dev=n_dev,
                                           feat_extra_h=ex_f, feat_extra=fe if n_extra else None)
                    else:
                        fx = torch.zeros((n_max, 32), dtype=torch.float16, device=DEV)
                        hip.field_shade_fwd(n_max, d_rows, cache, phf, d_dirs, emb, sidx if use_emb else None, phc, f0, fx, sx, rgb, n_dev=n_dev,
                                            x_extra_h=ex_x, feat_extra=fe if n_extra else None)
                    out.append((N(f0), h16(sx), N(rgb), N(fe)))
                what = "n=%d rows=%s emb=%d extra=%d: " % (n, name, use_emb, n_extra)
                for a, b, k in zip(out[0], out[1], ("f0", "shade_x", "rgb", "feat_extra")):
                    assert_same(a, b, what + k)
                f0, sx, rgb, fe = out[1]
                assert (f0[m:] == -7.0).all() and (rgb[m:] == -7.0).all() and (sx[m:] == np.float16(-7.0).view(np.uint16)).all(), what
                assert (f0[:m] != -7.0).all() and (rgb[:m] != -7.0).all(), what
                assert (fe != -7.0).all() if n_extra else (fe == -7.0).all(), what


def run_field_bwd(hip, gd, grid, cap, n_dev, n_off, pts, vol, ph, dfeat, compact=None, x_edge=None, cache=None, rows=None):
    dW = torch.zeros(3072, device=DEV)
    gtab = torch.zeros(grid.table_f32.size, dtype=torch.float16, device=DEV)
    hip.deferred_reset()
    head = (cap, n_dev, n_off, grid.n_volumes, gd["prim"], gd["lidx"], gd["lsize"], gd["bias"], gd["scale"], pts, vol, 1, ph)
    tail = (dfeat, 128.0, dW, gtab, 1 << LOG2, 1)
    if compact is not None:
        hip.field_bwd_dyn(*head, compact, *tail)
    else:
        hip.field_bwd_dyn_rows(*head, x_edge, cache, rows, *tail)
    hip.reduce_deferred()
    torch.cuda.synchronize()
    return N(dW), h16(gtab)


@pytest.mark.parametrize("n", SIZES)
def test_field_backward_on_cache_rows(hip, fox_state, fox_golden, nets, n):
    """f2n_field_bwd_dyn_rows on (edge rows, cache, src_rows) == f2n_field_bwd_dyn on the gathered compact copy: the weight gradients
    after f2n_reduce_deferred and the gradient table (see the module docstring for the planes and the mask)."""
    phf, _ = nets
    g = fox_golden
    rng = np.random.default_rng(200 + n)
    grid = make_grid(fox_state, rng, LOG2, scale=0.5)
    gd = grid_dev(grid)
    cache_np = (rng.standard_normal((n, 32)) * 0.5).astype(np.float16)
    cache = T(cache_np)
    for name, rows in row_sets(rng, n):
        m = len(rows)
        for n_off in (0, 6):
            edge_np = (rng.standard_normal((n_off, 32)) * 0.5).astype(np.float16)
            for cap in (CAP, m + n_off + 3):
                tot = m + n_off
                pick = rng.integers(0, len(g["march_pts"]), cap)
                pts, vol = T(g["march_pts"][pick]), T(np.ascontiguousarray(g["march_anchors"][pick, 0]))
                dfeat = T((rng.standard_normal((cap, 16)) * 1e-3).astype(F32))
                compact_np = np.full((cap, 32), 3.0, np.float16)  # (rows beyond the count: never read)
                compact_np[:n_off] = edge_np
                compact_np[n_off:tot] = cache_np[rows]
                d_rows = T(np.concatenate([rows, np.zeros(cap - n_off - m, np.int32)]))
                n_dev = torch.tensor([m], dtype=torch.int32, device=DEV)
                want = run_field_bwd(hip, gd, grid, cap, n_dev, n_off, pts, vol, phf, dfeat, compact=T(compact_np))
                got = run_field_bwd(hip, gd, grid, cap, n_dev, n_off, pts, vol, phf, dfeat, x_edge=T(edge_np) if n_off else None,
                                    cache=cache, rows=d_rows)
                what = "n=%d rows=%s n_off=%d capacity=%d: " % (n, name, n_off, cap)
                assert np.abs(want[0]).max() > 0, what
                assert_same(got[0], want[0], what + "dW")
                # (the reference-numerics build scatters with per-addend atomics at every size: module docstring, second item)
                if hip.lib().f2n_numerics_mode() == 0 and (cap >= CAP or tot == 1):
                    assert (want[1] != 0).any(), what
                    assert_same(got[1], want[1], what + "gradient table")


def test_prepass_routes_keep_their_outputs(hip, fox_state, fox_golden, nets):
    """out_feat_h of the three pre-pass routes == the f16 rounding of f2n_field_fwd_cached's out_feat_f32 on the saved rows (exact:
    those values are f16 values widened); its column 0 widened == out_f0."""
    phf, _ = nets
    g = fox_golden
    rng = np.random.default_rng(7)
    grid = make_grid(fox_state, rng, LOG2, scale=0.5)
    gd = grid_dev(grid)

    def check(what, cache, feat_h, f0):
        n = cache.shape[0]
        feat = torch.zeros((n, 16), device=DEV)
        hip.field_fwd_cached(n, n, None, cache, phf, feat, None, None)
        assert_same(h16(feat_h), h16(feat.to(torch.float16)), what + ": out_feat_h")
        assert_same(N(feat_h.float()), N(feat), what + ": widened")
        assert_same(N(feat_h[:, 0].float()), N(f0), what + ": column 0 == out_f0")
        assert float(feat.abs().max()) > 0

    for n in (1500, 9000):  # f2n_field_fwd: one kernel below 8192 samples, partitioned gather + plane-fed MLP from there on
        pick = rng.integers(0, len(g["march_pts"]), n)  # (the golden march holds fewer samples than that)
        pts, anchors = T(g["march_pts"][pick]), T(g["march_anchors"][pick])
        assert pts.shape == (n, 3) and anchors.shape == (n, 3)
        for fused in (False, True):
            cache = torch.zeros((n, 32), dtype=torch.float16, device=DEV)
            feat_h = torch.zeros((n, 16), dtype=torch.float16, device=DEV)
            f0 = torch.zeros(n, device=DEV)
            hip.field_fwd_ex(n, grid.n_volumes, gd["table_h"], gd["prim"], gd["lidx"], gd["lsize"], gd["bias"], gd["scale"], pts, anchors, 3,
                             phf, None, f0, cache, feat_h, fused=fused)
            check("field_fwd%s n=%d" % ("_fused" if fused else "", n), cache, feat_h, f0)
    x = (rng.standard_normal((1500, 32)) * 0.5).astype(np.float16)
    check("field_mlp_planes", *prepass_from_planes(hip, phf, x))


def test_kernel_level_equalities_hold_in_the_reference_numerics_build():
    """Both library builds take the change: the kernel-level tests above again, in a child process that loads libf2n_hip_refnum.so
    (a process has one numerics, chosen by the environment before the package is imported)."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, F2N_REFERENCE_NUMERICS="1", F2N_EXPECT_NUMERICS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "colour_path or cache_rows or prepass_routes"], capture_output=True, text=True, env=env, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "15 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def checksums(runner):
    stt = runner.states()  # (as bench.py forms them: table, field MLP, colour MLP)
    return [int(stt[i].contiguous().view(torch.int32).to(torch.int64).sum().item()) for i in (4, 8, 9)]


@pytest.mark.parametrize("mode", ["default", "fused_tail", "synchronous"])
def test_train_steps_are_bit_identical_with_and_without_reuse(rt, fox_state, mode):
    """Two runners from one seed, ExpRunner.prepass_feat_reuse on and off, three streaming steps at 512 rays: equal integer checksums
    of table and both MLPs, equal losses.  With the step's tail forced into the field backward's call, and with async_counts = 0
    (every step synchronous: the knob must be inert -- no step takes the reuse path)."""
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 512, rng)) for _ in range(4)]
    outs = {}
    for reuse in (True, False):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", [], seed=2022, device="cuda:0")
        torch.manual_seed(2022)
        assert runner.prepass_feat_reuse is True  # the default
        runner.prepass_feat_reuse = reuse
        if mode == "fused_tail":
            runner.fused_tail = 1
        if mode == "synchronous":
            runner.async_counts = 0
        losses = []
        for i in range(3):
            b, nb = batches[i], batches[i + 1]
            s = runner.train_step(b[0], b[1], b[2], b[3], b[4], True, nb[0], nb[1], nb[2])
            assert s["n_samples"] >= 32768, s["n_samples"]  # (the owner-binned scatter: below it the table's atomics add in arrival order)
            losses.append(float(s["loss"]))
        runner.flush()
        assert runner.prepass_reuse_steps == (3 if reuse and mode != "synchronous" else 0)
        outs[reuse] = (checksums(runner), losses)
        del runner
    assert outs[True][0] == outs[False][0], (mode, outs)
    assert outs[True][1] == outs[False][1] and all(x == x for x in outs[True][1]), (mode, outs)


def test_world_space_queries_leave_both_prepass_caches(rt, fox_state):
    """A world-space query between a pre-pass and its consumer (PrepassCacheGuard): both caches -- hash features and field outputs --
    are the same arrays with the same contents afterwards."""
    runner, cfg, _ = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    world = torch.rand((4096, 3), device="cuda:0", generator=gen) * 2.0 - 1.0
    warped, anchors = runner.locate_points(world)
    inside = anchors[:, 0] >= 0
    assert int(inside.sum()) >= 64
    f0 = runner.density_prepass(warped[inside].contiguous(), anchors[inside, 0].contiguous(), True)
    x, fh = runner.prepass_caches()
    assert x.shape == (f0.shape[0], 32) and fh.shape == (f0.shape[0], 16)
    assert torch.equal(fh[:, 0].float(), f0)
    x0, fh0 = x.clone(), fh.clone()
    dirs = torch.nn.functional.normalize(torch.rand((4096, 3), device="cuda:0", generator=gen) - 0.5, dim=1)
    runner.query_density(world)
    runner.query_radiance(world, dirs)
    runner.query_density_grad(world)
    x1, fh1 = runner.prepass_caches()
    assert x1.data_ptr() == x.data_ptr() and fh1.data_ptr() == fh.data_ptr() and x1.shape == x.shape and fh1.shape == fh.shape
    assert torch.equal(x1, x0) and torch.equal(fh1, fh0)
    runner.density_prepass(warped[inside].contiguous(), anchors[inside, 0].contiguous(), False)  # a pre-pass nobody asked outputs of
    x2, fh2 = runner.prepass_caches()
    assert x2.shape == x.shape and fh2.numel() == 0
