"""GPU (run with `-m gpu`): the fused MLP kernels -- csrc/mlp_dev.h through f2n_mlp_fwd / f2n_mlp_bwd, f2n_shade_fwd / f2n_shade_bwd and
f2n_field_fwd_cached / f2n_field_bwd, csrc/mlp_generic.hip through f2n_mlp_fwd / f2n_mlp_bwd for the other shapes -- against an fp64
network, PER ELEMENT: every output, input gradient, weight gradient, appearance-embedding gradient and hash-table gradient within the
bound of its own rounding error (tests/mlp_bound_ref.py: hard tier, and the calibrated tier for sums over 33 samples and more), and
exactly zero where it has no term.  The inputs are built so that kernel and reference provably share their ReLU masks; what the
inputs must satisfy for that, and that the oracle's C MLP passes the same checks, is tests/test_mlp_bound_cpu.py.  C-ABI only.

Recorded head-room (largest |kernel - fp64| per entry point; hard tier in units of the bound, calibrated tier in u Q, where the
limit is C_Q = 5.0).  Information only, never a threshold -- a change that doubles one of them should be looked at.
MI355X, 2026-10-21 (the emulated wavefront gives the same figures to three digits):
  f2n_field binned dparams [hard]                0.004
  f2n_field binned dparams [u Q]                 0.527
  f2n_field binned f0 [hard]                     0.448
  f2n_field binned feat [hard]                   0.547
  f2n_field binned table [hard]                  0.455
  f2n_field dparams [hard]                       0.688
  f2n_field dparams [u Q]                        0.488
  f2n_field f0 [hard]                            0.363
  f2n_field feat [hard]                          0.524
  f2n_field table [hard]                         0.473
  f2n_mlp generic (2 calls) dparams [hard]       0.858
  f2n_mlp generic (2 calls) dparams [u Q]        0.824
  f2n_mlp generic dparams [hard]                 0.905
  f2n_mlp generic dparams [u Q]                  1.100
  f2n_mlp generic dx [hard]                      0.116
  f2n_mlp generic out [hard]                     0.179
  f2n_mlp shipped (2 calls) dparams [hard]       0.945
  f2n_mlp shipped (2 calls) dparams [u Q]        0.584
  f2n_mlp shipped dparams [hard]                 0.945
  f2n_mlp shipped dparams [u Q]                  0.584
  f2n_mlp shipped dx [hard]                      0.489
  f2n_mlp shipped out [hard]                     0.495
  f2n_shade demb [hard]                          0.057
  f2n_shade demb [u Q]                           0.060
  f2n_shade dfeat [hard]                         0.057
  f2n_shade dparams [hard]                       0.538
  f2n_shade dparams [u Q]                        0.750
  f2n_shade rgb [hard]                           0.132
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mlp_bound_ref as R  # noqa: E402
from oracle import capi as oc  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
FILL = 7.0          # what output buffers hold before a call
PAD = 37            # rows allocated past n
SENTINEL = 1000.0   # what input rows past n hold: large, finite, and an f16 value


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import capi
    capi.lib()
    return capi


@pytest.fixture(scope="module", autouse=True)
def headroom_report():
    """Prints (run with -s) the largest ratios the checks of this module saw: what the docstring above records."""
    yield
    for what in sorted(R.RATIOS):
        print("  %-46s %.3f" % (what, R.RATIOS[what]))


def T(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # (a copy: the cached input sets are read-only)


def N(t):
    return t.detach().cpu().numpy()


def H(a):
    """float32 / uint16 f16 values -> device f16 tensor."""
    a = np.asarray(a)
    return T(a.view(np.float16) if a.dtype == np.uint16 else oc.f2h(a).view(np.float16))


def padded(a, fill, pad=PAD):
    a = np.ascontiguousarray(a)
    return np.concatenate([a, np.full((pad,) + a.shape[1:], fill, a.dtype)])


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = a.view(np.uint8) != b.view(np.uint8)
    assert not bad.any(), "%s: %d bytes differ" % (what, int(bad.sum()))


def family(shape):
    return "f2n_mlp %s" % ("shipped" if shape in R.SHIPPED else "generic")


# ---------------------------------------------------------------------------------------------------
# f2n_mlp_fwd / f2n_mlp_bwd
# ---------------------------------------------------------------------------------------------------
def mlp_run(hip, shape, params, x, dy, n, loss_scale, calls=1, rows=None):
    """out [rows,16] f16 as float32, dx [rows,d_in], dparams (scaled) after `calls` calls; buffers hold FILL before."""
    d_in, d_hidden, n_hidden = shape
    rows = n if rows is None else rows
    ph = H(params)
    out = torch.full((rows, 16), FILL, dtype=torch.float16, device=DEV)
    dx = torch.full((rows, d_in), FILL, device=DEV)
    dparams = torch.zeros(params.size, device=DEV)
    xt, dyt = T(x), T(dy)
    hip.mlp_fwd(n, d_in, d_hidden, n_hidden, ph, xt, out)
    for _ in range(calls):
        hip.mlp_bwd(n, d_in, d_hidden, n_hidden, loss_scale, ph, xt, dyt, dparams, dx)
    return N(out).astype(F32), N(dx), N(dparams)


@pytest.mark.parametrize("shape,n", R.MLP_CASES)
@pytest.mark.parametrize("loss_scale", [1.0, 128.0])
def test_mlp_per_element(hip, shape, n, loss_scale):
    """Outputs, dx and dparams / loss_scale of every network at every batch size that reaches another mechanism (one lane, the 16-sample
    half, the 32-sample pair, a tail tile, several waves; 4099: several blocks, the partials reduction, a ragged last tile); a second
    call accumulates: twice the bound against twice the reference."""
    assert hip.lib().f2n_mlp_n_params(*shape) == R.n_params(*shape)
    inp = R.mlp_case(shape, n)
    f, b = R.reference(inp, loss_scale)
    out, dx, dp = mlp_run(hip, shape, inp.params, inp.x, inp.dy, n, loss_scale)
    R.check_mlp(out, dx, dp.astype(np.float64) / loss_scale, f, b, n, family(shape))
    _, dx2, dp2 = mlp_run(hip, shape, inp.params, inp.x, inp.dy, n, loss_scale, calls=2)
    same_bits(dx2, dx, "dx of the second call")
    R.check_dparams(dp2.astype(np.float64) / loss_scale, b, n, family(shape) + " (2 calls)", calls=2)


@pytest.mark.parametrize("shape", R.SHIPPED + R.GENERIC)
def test_mlp_zero_column_and_dead_unit_are_exact(hip, shape):
    """An all-zero input column leaves exactly zero in that column of the first layer's gradient.  A hidden unit with an all-zero weight
    row (pre-activation exactly 0) passes no gradient: its gradient row is exactly zero, its outgoing column's gradient is exactly
    zero -- and the rest is within its bounds."""
    n, col, unit = 33, 3, 5
    d_in, d_hidden, n_hidden = shape
    inp = R.make_inputs(*shape, n, zero_col=col, dead_unit=(0, unit))
    f, b = R.reference(inp, 128.0)
    out, dx, dp = mlp_run(hip, shape, inp.params, inp.x, inp.dy, n, 128.0)
    R.check_mlp(out, dx, dp.astype(np.float64) / 128.0, f, b, n, family(shape))  # (A = 0 there: compared exactly)
    w0 = dp[:d_hidden * d_in].reshape(d_hidden, d_in)
    rows1 = 16 if n_hidden == 1 else d_hidden
    w1 = dp[d_hidden * d_in:d_hidden * d_in + rows1 * d_hidden].reshape(rows1, d_hidden)
    assert (w0[:, col] == 0).all() and (w0[unit] == 0).all() and (w1[:, unit] == 0).all()
    assert (w0 != 0).any() and (w1 != 0).any()


@pytest.mark.parametrize("shape", R.SHIPPED + R.GENERIC)
def test_mlp_samples_without_dy_contribute_nothing(hip, shape):
    """Samples whose dy row is zero: with their x rows replaced by other finite values dparams is bit-identical, and so is dx on the
    other rows."""
    n = 33
    inp = R.mlp_case(shape, n)
    quiet = np.arange(n) % 3 == 1
    dy = inp.dy.copy()
    dy[quiet] = 0
    x2 = inp.x.copy()
    x2[quiet] = R.f16(inp.x[quiet] * 0.5 + 0.25)
    _, dx_a, dp_a = mlp_run(hip, shape, inp.params, inp.x, dy, n, 128.0)
    _, dx_b, dp_b = mlp_run(hip, shape, inp.params, x2, dy, n, 128.0)
    same_bits(dp_a, dp_b, "dparams")
    same_bits(dx_a[~quiet], dx_b[~quiet], "dx of the other rows")
    assert (dx_a[quiet] == 0).all() and (dx_b[quiet] == 0).all() and (dp_a != 0).any()


@pytest.mark.parametrize("shape", R.SHIPPED + R.GENERIC)
@pytest.mark.parametrize("n", [1, 17, 33])
def test_mlp_rows_past_n_are_neither_read_nor_written(hip, shape, n):
    """x, dy, out and dx allocated longer than n: a large finite sentinel or zeros in the input rows >= n give bit-identical results, and
    the output rows >= n keep what they held."""
    inp = R.mlp_case(shape, n)
    res = [mlp_run(hip, shape, inp.params, padded(inp.x, v), padded(inp.dy, v), n, 128.0, rows=n + PAD) for v in (SENTINEL, 0.0)]
    for a, b, what in zip(res[0], res[1], ("out", "dx", "dparams")):
        same_bits(a, b, what)
    out, dx, dp = res[0]
    assert (out[n:] == FILL).all() and (dx[n:] == FILL).all()
    f, b = R.reference(inp, 128.0)
    R.check_mlp(out[:n], dx[:n], dp.astype(np.float64) / 128.0, f, b, n, family(shape))


# ---------------------------------------------------------------------------------------------------
# f2n_shade_fwd / f2n_shade_bwd
# ---------------------------------------------------------------------------------------------------
def shade_run(hip, c, n_emb, drgb=None, df0=None, rows=None, pad_value=0.0, feat=None, dirs=None):
    """rgb, saved x rows (uint16), dfeat, dparams (scaled), demb -- buffers of `rows` rows, FILL before the call."""
    n = c.n
    rows = n if rows is None else rows
    use_emb = n_emb > 0
    grow = (lambda a, v: padded(a, v, rows - n)) if rows > n else (lambda a, v: a)
    feat, dirs = c.feat if feat is None else feat, c.dirs if dirs is None else dirs
    drgb = c.drgb if drgb is None else drgb
    ph = H(c.params)
    emb = T(c.emb) if use_emb else None
    # (an index past n is a VALID image -- the last one, which has no sample -- so that a stray read could only show as a wrong number)
    idx = T(grow(c.idx, np.int32(n_emb - 1))) if use_emb else None
    rgb = torch.full((rows, 3), FILL, device=DEV)
    sx = torch.full((rows, 32), FILL, dtype=torch.float16, device=DEV)
    hip.shade_fwd(n, T(grow(feat, pad_value)), T(grow(dirs, pad_value)), emb, idx, ph, rgb, sx)
    dfeat = torch.full((rows, 16), FILL, device=DEV)
    dparams = torch.zeros(c.params.size, device=DEV)
    demb = torch.zeros((n_emb, 16), device=DEV) if use_emb else None
    hip.shade_bwd(n, T(grow(drgb, pad_value)), idx, ph, sx, 128.0, dfeat, dparams, demb, df0=None if df0 is None else T(grow(df0, pad_value)))
    return N(rgb), N(sx).view(np.uint16), N(dfeat), N(dparams), N(demb) if use_emb else None


def shade_set(n, n_emb, pattern):
    c = R.shade_case(n, n_emb, pattern)
    s = R.shade_reference(c.params, R._h2f(c.x_h), c.drgb, 128.0, n_emb, c.idx)
    return c, s


@pytest.mark.parametrize("n,n_emb,pattern", R.SHADE_CASES)
def test_shade_per_element(hip, n, n_emb, pattern):
    """rgb, dfeat[:, 1:], dparams and the appearance-embedding gradient per element; dfeat column 0 untouched, or merged from df0 (with
    every other bit the same).  Images without a sample -- there is at least one -- have an exactly zero gradient row."""
    c, s = shade_set(n, n_emb, pattern)
    rgb, sx, dfeat, dp, demb = shade_run(hip, c, n_emb)
    same_bits(sx, c.x_h, "saved colour-network input rows")  # (the oracle's: what the reference was computed from)
    R.check_shade(s, rgb, dfeat, dp.astype(np.float64) / 128.0, demb, n, "f2n_shade", fill=FILL)
    if n_emb:
        assert (demb[s.count == 0] == 0).all() and (s.count == 0).any()
    df0 = np.random.default_rng(n).standard_normal(n).astype(F32)
    rgb2, _, dfeat2, dp2, demb2 = shade_run(hip, c, n_emb, df0=df0)
    R.check_shade(s, rgb2, dfeat2, dp2.astype(np.float64) / 128.0, demb2, n, "f2n_shade", df0=df0)
    same_bits(dfeat2[:, 1:], dfeat[:, 1:], "dfeat[:, 1:] with df0")
    same_bits(dp2, dp, "dparams with df0")


@pytest.mark.parametrize("n,pattern", [(17, "each"), (33, "rr"), (257, "rr"), (257, "one")])
def test_shade_lds_and_global_embedding_paths_agree(hip, n, pattern):
    """240 images: the per-block fixed-point LDS image; 241: global float atomics.  The same samples on the same images: the two
    gradients differ by no more than the sum of their bounds; everything else is the same bits."""
    c, s240 = shade_set(n, 240, pattern)
    c241, s241 = shade_set(n, 241, pattern)
    assert (c.x_h == c241.x_h).all() and (c.idx == c241.idx).all()
    a, b = shade_run(hip, c, 240), shade_run(hip, c241, 241)
    for i, what in ((0, "rgb"), (2, "dfeat"), (3, "dparams")):
        same_bits(a[i], b[i], what)
    assert (np.abs(a[4].astype(np.float64) - b[4][:240]) <= R.demb_tolerance(s240) + R.demb_tolerance(s241)[:240]).all()
    assert (b[4][240] == 0).all()


def test_shade_samples_without_drgb_contribute_nothing(hip):
    n, n_emb = 33, 3
    c, _ = shade_set(n, n_emb, "one")
    quiet = np.arange(n) % 3 == 1
    drgb = c.drgb.copy()
    drgb[quiet] = 0
    feat2 = c.feat.copy()
    feat2[quiet] = (c.feat[quiet] * F32(0.5) + F32(0.25)).astype(F32)
    a = shade_run(hip, c, n_emb, drgb=drgb)
    b = shade_run(hip, c, n_emb, drgb=drgb, feat=feat2)
    same_bits(a[3], b[3], "dparams")
    same_bits(a[4], b[4], "demb")
    same_bits(a[2][~quiet], b[2][~quiet], "dfeat of the other rows")
    assert (a[2][quiet][:, 1:] == 0).all() and (b[2][quiet][:, 1:] == 0).all() and (a[3] != 0).any()


@pytest.mark.parametrize("n,n_emb,pattern", [(1, 3, "one"), (17, 240, "each"), (33, 241, "rr"), (17, 0, None)])
def test_shade_rows_past_n_are_neither_read_nor_written(hip, n, n_emb, pattern):
    c, s = shade_set(n, n_emb, pattern)
    df0 = np.random.default_rng(n).standard_normal(n).astype(F32)
    res = [shade_run(hip, c, n_emb, df0=df0, rows=n + PAD, pad_value=F32(v)) for v in (SENTINEL, 0.0)]
    for a, b, what in zip(res[0], res[1], ("rgb", "saved x", "dfeat", "dparams", "demb")):
        if a is not None:
            same_bits(a, b, what)
    rgb, sx, dfeat, dp, demb = res[0]
    assert (rgb[n:] == FILL).all() and (dfeat[n:] == FILL).all() and (sx[n:].view(np.float16) == FILL).all()
    same_bits(sx[:n], c.x_h, "saved colour-network input rows")
    R.check_shade(s, rgb[:n], dfeat[:n], dp.astype(np.float64) / 128.0, demb, n, "f2n_shade", df0=df0)


# ---------------------------------------------------------------------------------------------------
# f2n_field_fwd_cached / f2n_field_bwd
# ---------------------------------------------------------------------------------------------------
def field_run(hip, c, level_entries, rows=None, pad_value=0.0, with_index=False):
    n, grid = c.n, c.grid
    rows = n if rows is None else rows
    grow = (lambda a, v: padded(a, v, rows - n)) if rows > n else (lambda a, v: a)
    ph = H(c.params)
    cache = H(grow(oc.h2f(c.x_h), pad_value))
    src = T(grow(np.arange(n, dtype=np.int32), np.int32(0 if pad_value == 0.0 else rows - 1))) if with_index else None  # (valid rows either way)
    feat = torch.full((rows, 16), FILL, device=DEV)
    f0 = torch.full((rows,), FILL, device=DEV)
    sx = torch.full((rows, 32), FILL, dtype=torch.float16, device=DEV)
    hip.field_fwd_cached(n, rows, src, cache, ph, feat, f0, sx)
    dparams = torch.zeros(c.params.size, device=DEV)
    gtab = torch.zeros(grid.table_f32.size, dtype=torch.float16, device=DEV)
    anchors = grow(c.anchors, np.int32(0))
    hip.field_bwd(n, grid.n_volumes, T(grid.prim_pool), T(grid.local_idx), T(grid.local_size), T(grid.bias_pool), T(grid.scales),
                  T(grow(c.pts, F32(0.3 if pad_value else 0.0))), T(anchors), 3, ph, sx, T(grow(c.dfeat, pad_value)), 128.0, dparams, gtab, level_entries)
    return N(feat), N(f0), N(sx).view(np.uint16), N(dparams), N(gtab).astype(F32)


@pytest.mark.parametrize("n", R.FIELD_CASES)
def test_field_per_element(hip, n):
    """feat, f0, dparams and the hash-table gradient over EVERY entry: touched ones within their bound (the scatter of w * dx over the
    eight corners and sixteen levels, addresses and weights the oracle's), untouched ones exactly 0.  Batches this small are scattered
    with direct packed-f16 atomics whatever level_entries says (field.hip: f2n_use_bins); test_field_binned_per_element is the other
    route."""
    c = R.field_case(n)
    f, b, t = R.field_reference(c, 128.0)
    feat, f0, sx, dp, gtab = field_run(hip, c, 1 << R.FIELD_LOG2)
    same_bits(sx, c.x_h, "saved field-network input rows")
    same_bits(f0, feat[:, 0].copy(), "f0 == feat[:, 0]")
    R.check_field(f, b, t, feat, f0, dp.astype(np.float64) / 128.0, gtab, n, "f2n_field")
    assert (gtab[t["A"] == 0] == 0).all() and (gtab != 0).any()


@pytest.mark.parametrize("rows_past_n", [False, True])
def test_field_binned_per_element(hip, rows_past_n):
    """The owner-binned scatter (32768 samples and more, level_entries = 2^14: queues of f16 records, exact fixed-point sums by the
    table slices' owners, one rounding into the table): the same checks with that route's rounding count, on rays of closely spaced
    samples (runs to combine) with a ragged tail.  Its sums do not depend on the order of arrival, so with rows allocated past n
    (rows_past_n) a sentinel or zeros there give the same bits in every output, the table gradient included."""
    n = R.FIELD_BINNED_N
    assert n >= 32768  # F2N_BIN_MIN_N: below it this would be the direct route again
    c = R.field_case(n)
    f, b, t = R.field_reference(c, 128.0, owner=True)
    if rows_past_n:
        res = [field_run(hip, c, 1 << R.FIELD_LOG2, rows=n + PAD, pad_value=v, with_index=True) for v in (SENTINEL, 0.0)]
        for a, b_, what in zip(res[0], res[1], ("feat", "f0", "saved x", "dparams", "table gradient")):
            same_bits(a, b_, what)
        feat, f0, sx, dp, gtab = res[0]
        assert (feat[n:] == FILL).all() and (f0[n:] == FILL).all() and (sx[n:].view(np.float16) == FILL).all()
        feat, f0, sx = feat[:n], f0[:n], sx[:n]
    else:
        feat, f0, sx, dp, gtab = field_run(hip, c, 1 << R.FIELD_LOG2)
    same_bits(sx, c.x_h, "saved field-network input rows")
    R.check_field(f, b, t, feat, f0, dp.astype(np.float64) / 128.0, gtab, n, "f2n_field binned")
    assert (gtab[t["A"] == 0] == 0).all() and (gtab != 0).any()


@pytest.mark.parametrize("n", R.FIELD_CASES)
def test_field_rows_past_n_are_neither_read_nor_written(hip, n):
    c = R.field_case(n)
    f, b, t = R.field_reference(c, 128.0)
    res = [field_run(hip, c, 0, rows=n + PAD, pad_value=v, with_index=True) for v in (SENTINEL, 0.0)]
    for a, b_, what in zip(res[0], res[1], ("feat", "f0", "saved x", "dparams")):
        same_bits(a, b_, what)
    # (batches this small sum the table gradient by packed-f16 atomics in the order the waves arrive: two runs need not give the same
    # bits, whatever the rows past n hold -- each is held to its bounds, untouched entries exactly 0; the owner-binned route is order-free
    # and is compared bit for bit in test_field_binned_per_element)
    for feat, f0, sx, dp, gtab in res:
        assert (feat[n:] == FILL).all() and (f0[n:] == FILL).all() and (sx[n:].view(np.float16) == FILL).all()
        R.check_field(f, b, t, feat[:n], f0[:n], dp.astype(np.float64) / 128.0, gtab, n, "f2n_field")
