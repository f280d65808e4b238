"""TEST INFRASTRUCTURE ONLY -- fp64 reference of the bias-free ReLU MLPs with a PER-ELEMENT error yardstick (plain numpy, no device).

The fused networks (csrc/mlp_dev.h from field.hip / shade.hip, csrc/mlp_generic.hip) cannot be pinned bit for bit (tiny-cuda-nn is
not in the reference tree), so they are held against an fp64 network.  The tolerance of an element is not a share of its tensor's
largest value but a bound on that element's own rounding error, computed next to it:

  A   the same pass with |W|, |x|, |dy| and the same ReLU masks: the sum of the absolute values of the element's terms.  Given the
      masks the computation is linear, so a chain of k roundings to f16 (u = 2^-11, each relative to a value <= A) and n_terms fp32
      additions (2^-24 each; a product of two f16 values is exact in fp32) stays within (k u + n_terms 2^-24) A of the fp64 value --
      the HARD tier, first order in u as every such bound.
  E   ("floor") what is not relative: 2^-25 per f16 rounding for results in the f16 subnormal range, 2^-39 per addend of the
      appearance-embedding gradient's 2^-38 fixed-point grid, and the colour path's d(sigmoid) being evaluated at the computed output
      (shade_reference).  Carried through the same |W| / masks.  The test inputs are of order 1 (activations) and 1e-2 .. 1
      (scaled gradients), where the subnormal and fixed-point parts of E are 1e-4 of the u A term or less: there for rigour, not as
      slack.  The colour path's sigmoid term is NOT small: |drgb| sup|sigmoid''| bound(o) is several u of dy, as much as the k u A
      term itself, and worst-case in a way roundings never are -- the kernels sit at 0.06 of the dfeat / demb bound.
  T   ("tight") the same first-order bound without the envelope |value| <= A: a rounding to f16 costs u |value rounded| (+ 2^-25),
      an fp32 sum of N products N 2^-24 sum|products|, and both travel on through |W| and the masks like E (with |value| + T for
      the computed value, so T is not first-order only).  T <= the A form up to the second-order terms that one neglects; it matters where A compounds |W| over many layers (five hidden layers: A is ~200 x the
      value, the A form alone could not see a zeroed answer in 10-30 % of the weight-gradient elements).  The hard tier applies
      both: the A form as stated, and T.
  Q   for quantities summed over SAMPLES (dW, the embedding gradient): the per-sample A combined in quadrature.  The worst case
      k u A is never met by a sum of n independent roundings; c u Q with a measured c (C_Q below) is the CALIBRATED tier used where
      n is large.

ReLU masks.  make_inputs / select_rows keep a sample only if every hidden pre-activation has |z| > 2 bound(z), bound(z) being z's own
hard bound: a correct kernel's fp32 pre-activation then has the sign of the fp64 one (and is not flushed by the f16 rounding), so
kernel, oracle and reference share their masks and every later comparison is between linear maps.  A unit whose terms are all zero
(A = 0: a zero weight row) is exactly 0 on every side and is kept.

Rounding table (k is the count along the longest path; read from the sources named).  nh = number of hidden layers, h_0 = x.
  quantity                          f16 roundings                                                             k
  x, weights                        f16-exact inputs (mlp_dev.h f2n_load_xfrag_*, mlp_generic.hip:128)         0
  hidden pre-activation z_l (fp32)  the l activations below it (mlp_dev.h f2n_pack<true>, mlp_generic f2n_cvt4) l   (l = 0 .. nh-1)
  hidden activation h_l             + its own rounding                                                          l   (l = 1 .. nh)
  network output                    nh activations + the f16 output (field.hip "(float)(half_t) o[r]",          nh + 1
                                    mlp_generic.hip:161, shade.hip:318)
  dy * loss_scale                   f16(f16(dy) * scale): exact for the inputs built here (f2n_field_bwd_body,   0
                                    mlpg_bwd_chain_kernel:182); the colour path rounds drgb * dsig once          (1, shade)
  hidden gradient at layer l        one rounding per layer passed, "in the precision they are consumed in"      nh - l + 1 (l = 1 .. nh)
                                    (mlp_dev.h f2n_pack<false> of gl / g0, mlp_generic.hip:195,213)
  dx                                W_0^T g_1 in fp32, / loss_scale (a power of two) exact                       nh
  dW_l = sum_s g_{l+1} h_l^T        roundings of g_{l+1} (nh - l) + of h_l (l); the identity-fragment            nh
                                    re-orientation is exact for f16 data; MFMA accumulation, per-wave flush
                                    (f2n_mlp_flush_dw), per-block partials and f2n_reduce_partials are all
                                    fp32 additions (n_terms), the output stays fp32 (no f16 rounding)
  dW_l, the oracle's C MLP          + f16(sum) (f2n_oracle.c:1043; the second rounding, f16(f16 / scale), is      nh + 1
                                    exact for a power-of-two scale above the subnormal range)
  colour: rgb                       output (nh + 1) through (1 + 2 eps) sigmoid(o) - eps in fp32                  nh + 1
  colour: dfeat, demb               dx with the rounded dy; demb = fp32 / fixed-point sums of dx rows            nh + 1
  field: table gradient, direct     dx (nh) -> f16 (field.hip f2n_pack<false>(dxT), Hash3DAnchored.cu:220),      nh + 1 + m
                                    w * g and run sums in fp32, -> f16, then one f16 rounding per packed-f16
                                    atomic after the first (f2n_scatter_frag): m = addends of the entry
  field: table gradient, owners     (n >= 32768: f2n_use_bins) dx -> f16, every record (run total) -> f16,       nh + 1 + min(m, 2)
                                    exact fixed-point sums, one rounding into the table
n_terms: the fp32 additions along the path -- the fan-ins of the matrices passed, plus the number of samples (and one per
accumulating call) for the sample sums; any summation order or tree of N numbers makes at most N - 1 rounded additions.
"""
import functools
import os

import numpy as np

U = 2.0 ** -11          # unit roundoff of binary16
EPS32 = 2.0 ** -24      # ... of binary32
SUB16 = 2.0 ** -25      # half the spacing of the f16 subnormals
EPS_RGB = 1e-3          # SHShader.cpp:27-28
MARGIN = 2.0            # |z| > MARGIN * bound(z)

# Calibrated tier: |got - ref| <= C_Q u Q for sample-summed quantities.  C_Q is 4 x the largest |oracle - fp64| / (u Q) over every input
# set of tests/test_gpu_mlp_bounds.py whose sums are held to this tier (the factor covers another summation order), rounded up to one
# decimal; tests/test_mlp_bound_cpu.py re-measures it on every run and asserts measured <= C_Q / 4.  Measured 2026-10-21: 1.2247 (the
# oracle's C MLP, dW of 80 -> 128 -> 128 -> 16 at n = 33; 1.14 on the colour path, 1.12 for 32 -> 64 -> 16 at n = 257, 0.81 on the field
# path): 4 x 1.2247 = 4.899 -> 5.0.
C_Q = 5.0


def f16(a):
    """Round to binary16, back as fp64."""
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def layer_dims(d_in, d_hidden, n_hidden):
    return [(d_hidden, d_in)] + [(d_hidden, d_hidden)] * (n_hidden - 1) + [(16, d_hidden)]


def n_params(d_in, d_hidden, n_hidden):
    return sum(r * c for r, c in layer_dims(d_in, d_hidden, n_hidden))


def split_params(params, d_in, d_hidden, n_hidden):
    """Flat parameter vector (the layout of oc.mlp_n_params: row-major [rows][cols], layers in order) -> list of fp64 matrices."""
    params = np.asarray(params, np.float64)
    assert params.size == n_params(d_in, d_hidden, n_hidden)
    out, off = [], 0
    for r, c in layer_dims(d_in, d_hidden, n_hidden):
        out.append(params[off:off + r * c].reshape(r, c))
        off += r * c
    return out


def rand_params(rng, d_in, d_hidden, n_hidden):
    """tests/test_gpu_mlp_shapes.py's initialisation, rounded to f16 (returned as float32)."""
    parts = []
    for rows, cols in layer_dims(d_in, d_hidden, n_hidden):
        s = np.sqrt(6.0 / (rows + cols))
        parts.append(rng.uniform(-s, s, rows * cols).astype(np.float32))
    return f16(np.concatenate(parts)).astype(np.float32)


class Fwd:
    """fp64 forward with its companions.  h[l], Ah[l], Eh[l]: input of matrix l (h[0] = x); z[l], Az[l], Ez[l], kz[l], nz[l]: hidden
    pre-activation l and its hard bound's ingredients; out / Aout / Eout with k_out, n_out; masks[l] = z[l] > 0.  Th[l], Tout: the
    tight bounds (module docstring, "T")."""

    def bound_z(self, l):
        return (self.kz[l] * U + self.nz[l] * EPS32) * self.Az[l] + self.Ez[l]

    def bound_out(self):
        return np.minimum((self.k_out * U + self.n_out * EPS32) * self.Aout + self.Eout, self.Tout)

    def margin_ok(self):
        """Per sample: every hidden pre-activation is MARGIN bounds away from zero (or has no term at all)."""
        ok = np.ones(self.h[0].shape[0], bool)
        for l in range(len(self.z)):
            ok &= ((np.abs(self.z[l]) > MARGIN * self.bound_z(l)) | (self.Az[l] == 0)).all(1)
        return ok


def forward(params, x, d_hidden, n_hidden, x_err=None):
    x = np.asarray(x, np.float64)
    assert x.ndim == 2 and (f16(x) == x).all(), "x must be f16-exact"
    W = split_params(params, x.shape[1], d_hidden, n_hidden)
    assert all((f16(w) == w).all() for w in W), "weights must be f16-exact"
    f = Fwd()
    f.W = W
    f.h, f.Ah, f.Eh = [x], [np.abs(x)], [np.zeros_like(x) if x_err is None else np.asarray(x_err, np.float64)]
    f.Th = [f.Eh[0]]
    f.kh, f.nh_terms = [0], [0]
    f.z, f.Az, f.Ez, f.kz, f.nz, f.masks = [], [], [], [], [], []
    for l in range(n_hidden):
        z, Az, Ez = f.h[l] @ W[l].T, f.Ah[l] @ np.abs(W[l]).T, f.Eh[l] @ np.abs(W[l]).T
        m = z > 0
        f.z.append(z); f.Az.append(Az); f.Ez.append(Ez); f.masks.append(m)
        f.kz.append(f.kh[l]); f.nz.append(f.nh_terms[l] + W[l].shape[1])
        f.h.append(np.where(m, z, 0.0)); f.Ah.append(np.where(m, Az, 0.0))
        f.Eh.append(np.where(m, Ez + SUB16, 0.0))  # (the rounding of this activation, should it be subnormal)
        Tz = f.Th[l] @ np.abs(W[l]).T + W[l].shape[1] * EPS32 * ((np.abs(f.h[l]) + f.Th[l]) @ np.abs(W[l]).T)
        f.Th.append(np.where(m, Tz + U * (np.abs(z) + Tz) + SUB16, 0.0))  # (the value rounded is the computed one: |z| + Tz at most)
        f.kh.append(f.kz[l] + 1); f.nh_terms.append(f.nz[l])
    Wo = W[n_hidden]
    f.out, f.Aout = f.h[-1] @ Wo.T, f.Ah[-1] @ np.abs(Wo).T
    f.Eout = np.where(f.Aout > 0, f.Eh[-1] @ np.abs(Wo).T + SUB16, 0.0)
    f.k_out, f.n_out = f.kh[-1] + 1, f.nh_terms[-1] + Wo.shape[1]
    To = f.Th[-1] @ np.abs(Wo).T + Wo.shape[1] * EPS32 * ((np.abs(f.h[-1]) + f.Th[-1]) @ np.abs(Wo).T)
    f.Tout = np.where(f.Aout > 0, To + U * (np.abs(f.out) + To) + SUB16, 0.0)
    return f


class Bwd:
    """dW[l] / A_dW[l] / Q_dW[l] / E_dW[l] / T_dW[l] per matrix with k_dW, n_dW[l]; dx / A_dx / E_dx / T_dx with k_dx, n_dx.  TRUE
    (unscaled) gradients."""


def backward(f, dy, loss_scale, k_dy=0, dy_err=None):
    """dy [n,16] fp64 with dy * loss_scale f16-exact (k_dy = 0), or the colour path's (k_dy = 1, dy_err = E of dy * loss_scale)."""
    n_hidden = len(f.z)
    g = np.asarray(dy, np.float64) * loss_scale
    if k_dy == 0:
        assert (f16(g) == g).all() and (f16(dy) == np.asarray(dy, np.float64)).all(), "dy and dy * loss_scale must be f16-exact"
    Ag = np.abs(g)
    Eg = np.zeros_like(g) if dy_err is None else np.asarray(dy_err, np.float64)
    Tg = Eg + k_dy * U * Ag
    kg, ng = k_dy, 0
    n = g.shape[0]
    b = Bwd()
    b.dW, b.A_dW, b.Q_dW, b.E_dW, b.T_dW, b.n_dW = ([None] * (n_hidden + 1) for _ in range(6))
    b.k_dW = k_dy + n_hidden
    inv = 1.0 / loss_scale
    for l in range(n_hidden, -1, -1):
        h, Ah, Eh = f.h[l], f.Ah[l], f.Eh[l]
        assert kg + f.kh[l] == b.k_dW
        b.dW[l] = g.T @ h * inv
        b.A_dW[l] = Ag.T @ Ah * inv
        b.Q_dW[l] = np.sqrt((Ag * Ag).T @ (Ah * Ah)) * inv
        b.E_dW[l] = (Eg.T @ Ah + Ag.T @ Eh) * inv
        b.n_dW[l] = ng + f.nh_terms[l] + n
        b.T_dW[l] = (Tg.T @ (np.abs(h) + f.Th[l]) + np.abs(g).T @ f.Th[l] + n * EPS32 * ((np.abs(g) + Tg).T @ (np.abs(h) + f.Th[l]))) * inv
        W = f.W[l]
        gp, Agp, Egp = g @ W, Ag @ np.abs(W), Eg @ np.abs(W)
        Tgp = Tg @ np.abs(W) + W.shape[0] * EPS32 * ((np.abs(g) + Tg) @ np.abs(W))
        ng += W.shape[0]
        if l > 0:
            m = f.masks[l - 1]
            g, Ag = np.where(m, gp, 0.0), np.where(m, Agp, 0.0)
            Eg = np.where(m & (Agp > 0), Egp + SUB16, 0.0)
            Tg = np.where(m & (Agp > 0), Tgp + U * (np.abs(gp) + Tgp) + SUB16, 0.0)
            kg += 1
        else:
            b.dx, b.A_dx, b.E_dx, b.T_dx, b.k_dx, b.n_dx = gp * inv, Agp * inv, Egp * inv, Tgp * inv, kg, ng
    return b


def flat(mats):
    return np.concatenate([np.asarray(m).reshape(-1) for m in mats])


# ---------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------
def tolerance(A, k, n_terms, floor=0.0):
    return (np.asarray(k) * U + np.asarray(n_terms) * EPS32) * np.asarray(A, np.float64) + floor


def hard_tolerance(A, k, n_terms, floor=0.0, tight=None):
    t = tolerance(A, k, n_terms, floor)
    return t if tight is None else np.minimum(t, tight)


def check(got, ref, A, Q, k, n_terms, what, floor=0.0, c=None, tight=None):
    """Per element, none skipped.  Hard tier (c is None): |got - ref| <= (k u + n_terms 2^-24) A + floor -- and <= tight (T), where
    given.  Calibrated tier: |got - ref| <= c u Q.  An element with A == 0 (dead unit, all-zero input column, image without samples) must be exactly 0.
    Returns the largest |got - ref| in units of the tolerance (hard tier) or of u Q (calibrated tier): information, not a threshold."""
    got, ref, A = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(A, np.float64)
    assert got.shape == ref.shape == A.shape, (what, got.shape, ref.shape, A.shape)
    assert np.isfinite(got).all(), "%s: non-finite values" % what
    zero = A == 0
    assert (ref[zero] == 0).all(), what
    bad0 = zero & (got != 0)
    assert not bad0.any(), "%s: %d elements without any term are not exactly 0 (first at %s: %r)" % (
        what, int(bad0.sum()), np.argwhere(bad0)[0].tolist(), got[tuple(np.argwhere(bad0)[0])])
    err = np.abs(got - ref)
    if c is None:
        unit = np.broadcast_to(hard_tolerance(A, k, n_terms, floor, tight), A.shape)
        tol = unit
    else:
        unit = U * np.broadcast_to(np.asarray(Q, np.float64), A.shape)
        tol = c * unit
    live = ~zero
    if not live.any():
        return 0.0
    ratio = np.zeros(A.shape)
    ratio[live] = err[live] / unit[live]
    bad = live & (err > tol)
    if bad.any():
        i = tuple(np.argwhere(bad)[np.argmax(ratio[bad])].tolist())
        raise AssertionError("%s (%s tier): %d / %d elements out of tolerance; worst at %s: got %.9g ref %.9g err %.3g tol %.3g" % (
            what, "hard" if c is None else "calibrated", int(bad.sum()), bad.size, list(i), got[i], ref[i], err[i], tol[i]))
    return float(ratio.max())


def blind_share(ref, tol, A):
    """Share of the live elements whose tolerance is at least |ref|: there the check could not see an answer of zero."""
    live = np.asarray(A) > 0
    return float((np.broadcast_to(tol, np.shape(ref))[live] >= np.abs(np.asarray(ref))[live]).mean()) if live.any() else 0.0


# ---------------------------------------------------------------------------------------------------
# inputs with provable masks
# ---------------------------------------------------------------------------------------------------
class Inputs:
    pass


# Input distribution per shape.  A compounds |W| through every layer while z does not, so |z| / A falls geometrically with depth and
# with the first layer's cancellation: with dense N(0,1) rows 1.6 % of the draws pass the margin for 80 -> 128 -> 128 -> 16 and none
# of 20 000 for 48 -> 16 (x5) -> 16 (measured 2026-10-21).  Rows with few non-zero entries have no cancellation in the first layer
# (|W_0| |x| = |W_0 x| for one entry), which is the part of the ratio the inputs can reach: 8 of 80 entries N(0,1), the others zero,
# keeps 25 %; 1 of 48 keeps 14 % (2 of 48: 8 %).  The margin itself is the same for every shape.
NONZEROS = {(48, 16, 5): 1, (80, 128, 2): 8}
# ... and dy.  Where the samples' terms cancel, |dW| is ~ sqrt(n) terms while its bound is ~ n: with zero-mean dy the five-hidden-layer
# shape has 5-30 % of its elements below their own tolerance at n = 257.  A mean of DY_MEAN standard deviations per output channel
# (random sign per channel) keeps the sums from cancelling.
DY_MEAN = {(48, 16, 5): 2.0}


@functools.lru_cache(maxsize=None)
def make_inputs(d_in, d_hidden, n_hidden, n, seed=0, dy_scale=1e-2, zero_col=None, dead_unit=None):
    """params (f16-exact float32), x [n, d_in] float32 f16-exact rows that pass the mask margin (N(0,1) draws; NONZEROS entries per
    row for the shapes listed there), dy [n,16] float32 f16-exact with dy * 128 f16-exact, and keep_rate = kept / drawn.  zero_col:
    that input column is zero in every row; dead_unit (layer, unit): that hidden unit's weight row is zero (pre-activation exactly
    0).  Cached: shared by the tests, do not modify."""
    rng = np.random.default_rng([seed, d_in, d_hidden, n_hidden, n])
    nonzeros = NONZEROS.get((d_in, d_hidden, n_hidden))
    params = rand_params(rng, d_in, d_hidden, n_hidden)
    if dead_unit is not None:
        W = split_params(params, d_in, d_hidden, n_hidden)
        W[dead_unit[0]][dead_unit[1], :] = 0.0
        params = flat(W).astype(np.float32)
    rows, drawn = [], 0
    while sum(len(r) for r in rows) < n:
        x = f16(rng.standard_normal((max(2048, 4 * n), d_in)))
        if nonzeros is not None:
            keep = np.zeros(x.shape, bool)
            np.put_along_axis(keep, np.argsort(rng.random(x.shape), 1)[:, :nonzeros], True, 1)
            x = x * keep
        if zero_col is not None:
            x[:, zero_col] = 0.0
        drawn += len(x)
        rows.append(x[forward(params, x, d_hidden, n_hidden).margin_ok()])
        assert drawn < 400 * n + 4096, "keep rate below any use"
    kept = sum(len(r) for r in rows)
    inp = Inputs()
    inp.d_in, inp.d_hidden, inp.n_hidden, inp.n = d_in, d_hidden, n_hidden, n
    inp.params = params
    inp.x = np.concatenate(rows)[:n].astype(np.float32)
    dy_mean = DY_MEAN.get((d_in, d_hidden, n_hidden), 0.0) * np.where(rng.random(16) < 0.5, -1.0, 1.0)
    inp.dy = f16((rng.standard_normal((n, 16)) + dy_mean) * dy_scale).astype(np.float32)
    inp.keep_rate = kept / drawn
    for a in (inp.params, inp.x, inp.dy):
        a.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def reference(inp, loss_scale):
    f = forward(inp.params, inp.x, inp.d_hidden, inp.n_hidden)
    assert f.margin_ok().all()
    return f, backward(f, inp.dy, loss_scale)


def select_rows(params, x_rows, d_hidden, n_hidden, n):
    """Indices of the first n rows of x_rows (f16-exact candidates, e.g. hash features of the golden march) that pass the margin, and
    the keep rate over the candidates looked at."""
    ok = forward(params, x_rows, d_hidden, n_hidden).margin_ok()
    idx = np.nonzero(ok)[0]
    assert len(idx) >= n, (len(idx), n)
    idx = idx[:n]
    return idx, n / float(idx[-1] + 1)


# ---------------------------------------------------------------------------------------------------
# colour network (shade.hip): sigmoid in front of the loss, appearance-embedding gradient behind dx
# ---------------------------------------------------------------------------------------------------
def _sig(o):
    return 1.0 / (1.0 + np.exp(-o))


def _dsig_sup(o, b):
    """sup of sigmoid' over [o - b, o + b] (sigmoid' is even and falls with |o|)."""
    s = _sig(np.maximum(np.abs(o) - b, 0.0))
    return s * (1.0 - s)


def _d2sig_sup(o, b):
    """sup of |sigmoid''| over [o - b, o + b]: sigmoid'' = sigmoid' (1 - 2 sigmoid), |1 - 2 sigmoid(t)| = tanh(|t| / 2) grows with |t|;
    0.0963 is its global maximum."""
    return np.minimum(0.0963, _dsig_sup(o, b) * np.tanh((np.abs(o) + b) / 2))


class Shade:
    pass


def shade_reference(params, x_h, drgb, loss_scale, n_emb=0, emb_idx=None, d_hidden=64, n_hidden=2):
    """x_h: the SAVED f16 input rows [n,32] (as float; the GPU test compares them bit for bit with the oracle's first).
    rgb = (1 + 2 eps) sigmoid(o) - eps; the oracle and the kernels take d(sigmoid) = 0 where exp(-o) overflows fp32 (o < -88.7,
    oracle/pipeline.py: shade_bwd) -- the fp64 derivative there is below 1e-38, and the inputs built here stay far from it (asserted).
    dy = drgb * dsig(o): the kernels evaluate dsig at their own f16 output, so dy carries, besides its one f16 rounding (k_dy = 1), the
    absolute term |drgb| sup|sigmoid''| bound(o) (_d2sig_sup) and the fp32 evaluation of exp and the
    quotient (8 x 2^-24 relative): both go into E and through the backward like every other E."""
    f = forward(params, x_h, d_hidden, n_hidden)
    o, bo = f.out[:, :3], f.bound_out()[:, :3]
    assert (np.abs(o) < 80).all()
    s = Shade()
    s.f = f
    s.rgb = (1 + 2 * EPS_RGB) * _sig(o) - EPS_RGB
    s.A_rgb = (1 + 2 * EPS_RGB) * _dsig_sup(o, bo) * f.Aout[:, :3]
    s.E_rgb = (1 + 2 * EPS_RGB) * _dsig_sup(o, bo) * f.Eout[:, :3] + 8 * EPS32
    s.T_rgb = (1 + 2 * EPS_RGB) * _dsig_sup(o, bo) * f.Tout[:, :3] + 8 * EPS32
    s.k_rgb, s.n_rgb = f.k_out, f.n_out
    drgb = np.asarray(drgb, np.float64)
    dsig = (1 + 2 * EPS_RGB) * _sig(o) * (1 - _sig(o))
    n = o.shape[0]
    dy = np.zeros((n, 16))
    dy[:, :3] = drgb * dsig
    dy_err = np.zeros((n, 16))
    dy_err[:, :3] = (np.abs(drgb) * (1 + 2 * EPS_RGB) * _d2sig_sup(o, bo) * bo + 8 * EPS32 * np.abs(dy[:, :3]) + SUB16) * loss_scale
    dy_err[dy == 0] = 0.0
    s.dy = dy
    b = backward(f, dy, loss_scale, k_dy=1, dy_err=dy_err)
    s.b = b
    s.dfeat, s.A_dfeat, s.E_dfeat, s.T_dfeat = b.dx[:, :16], b.A_dx[:, :16], b.E_dx[:, :16], b.T_dx[:, :16]
    if n_emb:
        idx = np.asarray(emb_idx)
        onehot = np.zeros((n_emb, n))
        inside = (idx >= 0) & (idx < n_emb)
        onehot[idx[inside], np.nonzero(inside)[0]] = 1.0
        s.count = onehot.sum(1)
        s.demb, s.A_demb = onehot @ s.dfeat, onehot @ s.A_dfeat
        s.Q_demb = np.sqrt(onehot @ (s.A_dfeat ** 2))
        # 2^-39 per addend of the 2^-38 fixed-point image of the LDS path (shade.hip F2N_EMB_FIXED_SCALE), one fp32 rounding of the image
        s.E_demb = onehot @ s.E_dfeat + (s.count * 2.0 ** -39)[:, None] * (s.A_demb > 0)
        s.T_demb = onehot @ s.T_dfeat + ((s.count + 2) * EPS32)[:, None] * (onehot @ np.abs(s.dfeat)) + (s.count * 2.0 ** -39)[:, None] * (s.A_demb > 0)
        s.n_demb = b.n_dx + n + 2
    return s


# ---------------------------------------------------------------------------------------------------
# field network (field.hip): the table gradient is the scatter of w * dx over eight corners and sixteen levels
# ---------------------------------------------------------------------------------------------------
def table_scatter(pool_halves, local_idx, pos, w, dx, A_dx, E_dx, T_dx, owner=False):
    """pos [n,16,8] entry of each corner inside its level, w [n,16,8] its fp32 interpolation weight -- both the ORACLE's
    (oc.hash_cell; pinned bit for bit by the hash tests) --, dx / A_dx / E_dx [n,32] (feature 2 l + ch of level l).  Returns the
    gradient in the table's addressing (level l starts at local_idx[l] halves, entry p at 2 p + ch), its A, E, T and the number of
    addends m of every half and the f16 roundings r behind dx: r = 1 + m on the direct route (dx -> f16, the run total -> f16, one per
    packed-f16 atomic after the first), r = 1 + min(m, 2) on the owner-binned one (owner=True: dx -> f16, every record -> f16, the
    records summed exactly in the owners' 2^-24 fixed-point image -- hash_bin_accumulate_kernel --, one rounding into the table)."""
    n = dx.shape[0]
    addr = (np.asarray(local_idx, np.int64)[None, :, None, None] + 2 * np.asarray(pos, np.int64)[:, :, :, None] + np.arange(2)[None, None, None, :])  # [n,16,8,2]
    w = np.asarray(w, np.float64)[:, :, :, None]
    assert (w >= 0).all()  # (trilinear weights)

    flat_addr = addr.reshape(-1)

    def put(v):
        return np.bincount(flat_addr, weights=(np.asarray(v, np.float64).reshape(n, 16, 1, 2) * w).reshape(-1), minlength=pool_halves)

    grad, A = put(dx), put(A_dx)
    m = np.bincount(flat_addr, weights=((np.asarray(A_dx, np.float64).reshape(n, 16, 1, 2) * w) > 0).reshape(-1).astype(np.float64),
                    minlength=pool_halves)
    r = 1 + (np.minimum(m, 2) if owner else m)
    E = put(E_dx) + (A > 0) * (m + 1) * SUB16  # dx -> f16, and every addend's / record's own rounding, should it be subnormal
    T = put(T_dx) + (r * U + (m + 1) * EPS32) * put(np.abs(dx) + np.asarray(T_dx)) + (A > 0) * (m + 1) * SUB16
    return grad, A, E, T, m, r


# ---------------------------------------------------------------------------------------------------
# the input sets of tests/test_gpu_mlp_bounds.py (tests/test_mlp_bound_cpu.py holds the oracle against every one of them)
# ---------------------------------------------------------------------------------------------------
SHIPPED = [(32, 64, 1), (32, 64, 2)]
GENERIC = [(17, 64, 2), (48, 16, 5), (80, 128, 2)]        # from tests/test_gpu_mlp_shapes.py SHAPES
SMALL_N = [1, 15, 16, 17, 31, 33, 257]                    # one lane, the 16-sample half, the 32-sample pair, a tail tile, several waves
BIG_N = 4099                                              # several blocks, the partials reduction, a ragged last tile (shipped shapes)
CALIBRATED_FROM = 33                                      # sample sums of at least this many samples are held to C_Q u Q as well
MLP_CASES = [(s, n) for s in SHIPPED + GENERIC for n in SMALL_N] + [(s, BIG_N) for s in SHIPPED]
KEEP_MIN, BLIND_MAX = 0.10, 0.05


def dw_vectors(b):
    """Flat (ref, A, Q, E, T, n_terms) of all layers' weight gradients in the parameter layout."""
    nt = np.concatenate([np.full(m.size, t, np.float64) for m, t in zip(b.dW, b.n_dW)])
    return flat(b.dW), flat(b.A_dW), flat(b.Q_dW), flat(b.E_dW), flat(b.T_dW), nt


def sum_tolerance(A, Q, k, n_terms, floor, tight, n):
    """The tolerance check_sum applies to a quantity summed over n samples."""
    tol = hard_tolerance(A, k, n_terms, floor, tight)
    return np.minimum(tol, C_Q * U * Q) if n >= CALIBRATED_FROM else tol


RATIOS = {}  # head-room seen by note(): {what: largest ratio}; information only (recorded in the GPU tests' docstring)


def note(what, r):
    RATIOS[what] = max(r, RATIOS.get(what, 0.0))
    return r


def check_sum(got, ref, A, Q, k, n_terms, what, floor, tight, n, tag=None):
    """Hard tier always; from CALIBRATED_FROM samples on the calibrated tier too."""
    tag = what if tag is None else tag
    note(tag + " [hard]", check(got, ref, A, Q, k, n_terms, what, floor=floor, tight=tight))
    if n >= CALIBRATED_FROM:
        note(tag + " [u Q]", check(got, ref, A, Q, k, n_terms, what, c=C_Q))


def blind_shares_dw(b, n):
    return [blind_share(m, sum_tolerance(a, q, b.k_dW, t, e, tt, n), a) for m, a, q, e, tt, t in zip(b.dW, b.A_dW, b.Q_dW, b.E_dW, b.T_dW, b.n_dW)]


def blind_share_dx(b):
    return blind_share(b.dx, hard_tolerance(b.A_dx, b.k_dx, b.n_dx, b.E_dx, b.T_dx), b.A_dx)


def conditions_hold(inp):
    """At least KEEP_MIN of the draws kept; at most BLIND_MAX of every layer's weight-gradient elements, and of dx, below their own
    tolerance.  Conditions on the inputs, computed from the reference alone."""
    return inp.keep_rate >= KEEP_MIN and all(max(blind_shares_dw(b, inp.n) + [blind_share_dx(b)]) <= BLIND_MAX
                                             for b in (reference(inp, 1.0)[1], reference(inp, 128.0)[1]))


def first_good_seed(shape, n):
    return next(seed for seed in range(16) if conditions_hold(make_inputs(*shape, n, seed=seed)))


# The seed of every (shape, n) whose seed 0 misses a condition (the network drawn keeps under 10 % of its samples, or a layer's blind
# share passes 5 %); tests/test_mlp_bound_cpu.py asserts that this is the whole list and that each entry is the first seed that holds.
SEEDS = {
    ((48, 16, 5), 15): 6,
    ((48, 16, 5), 16): 1,
    ((48, 16, 5), 17): 6,
    ((48, 16, 5), 31): 3,
    ((48, 16, 5), 33): 2,
}


@functools.lru_cache(maxsize=None)
def mlp_case(shape, n):
    """The input set of one (shape, n): seed 0, or the seed SEEDS names."""
    return make_inputs(*shape, n, seed=SEEDS.get((shape, n), 0))


# ---- colour path -----------------------------------------------------------------------------------
# (n, n_emb, pattern): "one" = every sample on image 1, "rr" = round-robin over all images but the last, "each" = sample i on image i.
# The last image never has a sample (its gradient row is exactly 0).  240 is the last size of the LDS fixed-point image, 241 takes the
# global atomics; the 240 / 241 sets of one (n, pattern) are the same samples on the same images.
SHADE_CASES = [(1, 0, None), (1, 3, "one"), (17, 0, None), (17, 3, "rr"), (17, 240, "each"), (17, 241, "each"), (33, 3, "one"), (33, 240, "rr"),
               (33, 241, "rr"), (257, 0, None), (257, 3, "rr"), (257, 240, "rr"), (257, 241, "rr"), (257, 240, "one"), (257, 241, "one")]


def _image_of(i, n_emb, pattern):
    m = min(n_emb, 240) - 1
    return 1 if pattern == "one" else i % m


@functools.lru_cache(maxsize=None)
def _golden(name):
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)))


# seeds of the colour-path sets, by (n, pattern) -- the 240 / 241 sets of a pair share theirs --: 0 unless listed, as SEEDS above
SHADE_SEEDS = {
    (17, None): 1,
    (257, 'rr'): 1,
}


def shade_conditions_hold(n, n_emb, pattern, seed):
    """Keep rate, and the blind shares of every layer's weight gradient, of dfeat and of the embedding gradient."""
    c = shade_case(n, n_emb, pattern, seed)
    s = shade_reference(c.params, _h2f(c.x_h), c.drgb, 128.0, n_emb, c.idx)
    shares = blind_shares_dw(s.b, n) + [blind_share(s.dfeat[:, 1:], hard_tolerance(s.A_dfeat[:, 1:], s.b.k_dx, s.b.n_dx, s.E_dfeat[:, 1:], s.T_dfeat[:, 1:]),
                                                    s.A_dfeat[:, 1:])]
    if n_emb:
        shares.append(blind_share(s.demb, demb_tolerance(s), s.A_demb))
    return c.keep_rate >= KEEP_MIN and max(shares) <= BLIND_MAX


def first_good_shade_seed(n, pattern):
    return next(seed for seed in range(16) if all(shade_conditions_hold(n, e, p, seed) for m, e, p in SHADE_CASES if (m, p) == (n, pattern)))


@functools.lru_cache(maxsize=None)
def shade_case(n, n_emb, pattern, seed=None):
    """feat [n,16], dirs [n,3] (golden march directions), emb [n_emb,16], idx [n], drgb [n,3], params, x_h [n,32] uint16 (the oracle's
    f16 input rows) -- every row passes the mask margin with the embedding row of its image -- and the keep rate."""
    from oracle import capi as oc
    from oracle import pipeline as op
    seed = SHADE_SEEDS.get((n, pattern), 0) if seed is None else seed
    rng = np.random.default_rng([31, n, 0 if pattern is None else len(pattern), seed])
    params = rand_params(rng, 32, 64, 2)
    pool_dirs = _golden("fox_golden.npz")["march_dirs"]
    order = rng.permutation(len(pool_dirs))
    pool_feat = rng.standard_normal((len(pool_dirs), 16)).astype(np.float32)
    emb_all = (rng.standard_normal((241, 16)) * 0.1).astype(np.float32)
    emb = emb_all[:n_emb] if n_emb else None
    rows, imgs, j, B = [], [], 0, 32
    for i in range(n):
        img = _image_of(i, n_emb, pattern) if n_emb else 0
        while True:
            cand = order[j:j + B]
            assert len(cand) == B, "candidate pool exhausted"
            x = op.shade_input(pool_feat[cand], pool_dirs[cand], emb, np.full(B, img, np.int32) if n_emb else None)
            ok = forward(params, oc.h2f(oc.f2h(x)), 64, 2).margin_ok()
            if ok.any():
                first = int(np.argmax(ok))
                rows.append(cand[first]); imgs.append(img)
                j += first + 1
                break
            j += B
    c = Inputs()
    rows = np.asarray(rows)
    c.n, c.n_emb, c.params, c.emb = n, n_emb, params, emb
    c.feat, c.dirs = np.ascontiguousarray(pool_feat[rows]), np.ascontiguousarray(pool_dirs[rows])
    c.idx = np.asarray(imgs, np.int32) if n_emb else None
    c.x_h = oc.f2h(op.shade_input(c.feat, c.dirs, emb, c.idx))
    c.drgb = (rng.standard_normal((n, 3)) * 1e-2).astype(np.float32)
    c.keep_rate = n / float(j)
    return c


# ---- field path ------------------------------------------------------------------------------------
FIELD_CASES = [17, 257]
FIELD_LOG2 = 14
# the owner-binned scatter is taken from 32768 samples on (field.hip F2N_BIN_MIN_N; level_entries a power of two >= 8192): below it
# f2n_field_bwd scatters with direct packed-f16 atomics whatever level_entries says
FIELD_BINNED_N = 32768 + 37


@functools.lru_cache(maxsize=None)
def field_case(n):
    """A random log2-14 table on the golden scene's hash state, the golden march's points whose hash features (the oracle's, f16) pass
    the mask margin of a 32 -> 64 -> 16 network, dfeat with dfeat * 128 f16-exact, and the oracle's cell addresses / weights."""
    from oracle import capi as oc
    from oracle import pipeline as op
    st, g = _golden("fox_state.npz"), _golden("fox_golden.npz")
    rng = np.random.default_rng([21, n])
    local = 1 << FIELD_LOG2
    grid = op.HashGrid((rng.standard_normal((16 * local, 2)) * 0.5).astype(np.float32), st["prim_pool"], st["bias_pool"], int(st["n_volumes"]), FIELD_LOG2)
    params = rand_params(rng, 32, 64, 1)
    if n < 32768:
        start = int(rng.integers(0, 2000))
        pts, anchors = g["march_pts"][start:], g["march_anchors"][start:]
    else:  # rays of 50 closely spaced samples (tests/test_gpu_parity.py: test_hash_backward_owner_binned): runs to combine, ragged tail
        m = n + 2048
        n_rays = m // 50 + 1
        o = rng.random((n_rays, 3), dtype=np.float32) * np.float32(.6) + np.float32(.2)
        dvec = rng.standard_normal((n_rays, 3)).astype(np.float32)
        dvec /= np.linalg.norm(dvec, axis=1, keepdims=True)
        ray = np.repeat(np.arange(n_rays), 50)[:m]
        q = np.clip(o[ray] + dvec[ray] * ((np.arange(m) % 50).astype(np.float32) * np.float32(0.004))[:, None], 0.01, 0.99).astype(np.float32)
        pts = (q * np.float32(2.) - np.float32(1.)).astype(np.float32)
        anchors = np.zeros((m, 3), np.int32)
        anchors[:, 0] = rng.integers(0, int(st["n_volumes"]), n_rays).astype(np.int32)[ray]
    q01 = ((pts + np.float32(1.)) * np.float32(.5)).astype(np.float32)
    x_h = oc.hash_fwd(grid.table_h, grid.prim_pool, grid.local_idx, grid.local_size, grid.bias_pool, q01, anchors[:, 0], grid.n_volumes, grid.scales)
    idx, keep = select_rows(params, oc.h2f(x_h), 64, 1, n)
    c = Inputs()
    c.n, c.grid, c.params, c.keep_rate = n, grid, params, keep
    c.pts, c.anchors, c.x_h = np.ascontiguousarray(pts[idx]), np.ascontiguousarray(anchors[idx]), np.ascontiguousarray(x_h[idx])
    c.dfeat = f16(rng.standard_normal((n, 16)) * 1e-2).astype(np.float32)
    q01 = np.ascontiguousarray(q01[idx])
    vol = c.anchors[:, 0]
    prim, bias = np.asarray(grid.prim_pool).reshape(-1, 3), np.asarray(grid.bias_pool).reshape(-1, 3)
    c.pos, c.w = np.zeros((n, 16, 8), np.int64), np.zeros((n, 16, 8))
    for l in range(16):
        tf = l * grid.n_volumes + vol
        pos, w = oc.hash_cell(q01, np.full(n, grid.scales[l], np.float32), prim[tf], bias[tf], np.full(n, grid.local_size[l], np.uint32))
        c.pos[:, l], c.w[:, l] = pos, w
    c.q01 = q01
    return c


def field_reference(c, loss_scale, owner=False):
    f = forward(c.params, _h2f(c.x_h), 64, 1)
    assert f.margin_ok().all()
    b = backward(f, c.dfeat, loss_scale)
    # the table gradient is delivered SCALED (f16): compare in that domain, where the f16 subnormal floor is what it is
    grad, A, E, T, m, r = table_scatter(c.grid.table_f32.size, c.grid.local_idx, c.pos, c.w, b.dx * loss_scale, b.A_dx * loss_scale,
                                        b.E_dx * loss_scale, b.T_dx * loss_scale, owner)
    return f, b, dict(grad=grad, A=A, E=E, T=T, m=m, k=b.k_dx + r, n_terms=b.n_dx + 1 + m)


def _h2f(h):
    return np.asarray(h, np.uint16).view(np.float16).astype(np.float64)


# ---------------------------------------------------------------------------------------------------
# the comparisons, shared by the oracle check (CPU) and the kernels' tests (GPU / emulator)
# ---------------------------------------------------------------------------------------------------
def check_dparams(got, b, n, tag, oracle=False, calls=1):
    """got: TRUE (unscaled) weight gradients in the parameter layout after `calls` accumulating calls.  oracle: one more f16 rounding
    (rounding table: the oracle's C MLP rounds the scaled sum to f16)."""
    ref, A, Q, E, T, nt = dw_vectors(b)
    extra = U * np.abs(ref) + (A > 0) * SUB16 if oracle else 0.0
    check_sum(got, calls * ref, calls * A, calls * Q, b.k_dW + (1 if oracle else 0), nt + (calls - 1),
              "dparams", calls * (E + extra), calls * (T + extra) + (calls - 1) * EPS32 * np.abs(calls * ref), n, tag + " dparams")


def check_mlp(out, dx, dparams, f, b, n, tag, oracle=False):
    """Outputs (f16 values), dx and dparams / loss_scale of f2n_mlp_fwd / f2n_mlp_bwd (or the oracle's), per element."""
    if out is not None:
        note(tag + " out [hard]", check(out, f.out, f.Aout, None, f.k_out, f.n_out, "outputs", floor=f.Eout, tight=f.Tout))
    if dx is not None:
        note(tag + " dx [hard]", check(dx, b.dx, b.A_dx, None, b.k_dx, b.n_dx, "dx", floor=b.E_dx, tight=b.T_dx))
    if dparams is not None:
        check_dparams(dparams, b, n, tag, oracle)


def check_shade(s, rgb, dfeat, dparams, demb, n, tag, oracle=False, df0=None, fill=None):
    """dfeat: the whole [n,16] array -- column 0 must be df0 (merged) or the fill value (untouched)."""
    b = s.b
    if rgb is not None:
        note(tag + " rgb [hard]", check(rgb, s.rgb, s.A_rgb, None, s.k_rgb, s.n_rgb, "rgb", floor=s.E_rgb, tight=s.T_rgb))
    if dfeat is not None:
        want0 = np.full(n, fill, np.float32) if df0 is None else np.asarray(df0, np.float32)
        assert (np.asarray(dfeat, np.float32)[:, 0].view(np.uint32) == want0.view(np.uint32)).all(), "dfeat column 0"
        note(tag + " dfeat [hard]", check(dfeat[:, 1:], s.dfeat[:, 1:], s.A_dfeat[:, 1:], None, b.k_dx, b.n_dx, "dfeat", floor=s.E_dfeat[:, 1:],
                                          tight=s.T_dfeat[:, 1:]))
    if dparams is not None:
        check_dparams(dparams, b, n, tag, oracle)
    if demb is not None:
        note(tag + " demb [hard]", check(demb, s.demb, s.A_demb, None, b.k_dx, s.n_demb, "demb", floor=s.E_demb, tight=s.T_demb))
        big = s.count >= CALIBRATED_FROM  # (rows summed over many samples: the calibrated tier too)
        if big.any():
            note(tag + " demb [u Q]", check(demb[big], s.demb[big], s.A_demb[big], s.Q_demb[big], b.k_dx, s.n_demb, "demb", c=C_Q))


def demb_tolerance(s):
    tol = hard_tolerance(s.A_demb, s.b.k_dx, s.n_demb, s.E_demb, s.T_demb)
    return np.where((s.count >= CALIBRATED_FROM)[:, None], np.minimum(tol, C_Q * U * s.Q_demb), tol)


def check_field(f, b, t, feat, f0, dparams, gtab_scaled, n, tag, oracle=False):
    """feat fp32 [n,16] (f16 values), f0 = feat[:,0], dparams / loss_scale, the table gradient as delivered (scaled, f16 values)."""
    if feat is not None:
        note(tag + " feat [hard]", check(feat, f.out, f.Aout, None, f.k_out, f.n_out, "feat", floor=f.Eout, tight=f.Tout))
    if f0 is not None:
        note(tag + " f0 [hard]", check(f0, f.out[:, 0], f.Aout[:, 0], None, f.k_out, f.n_out, "f0", floor=f.Eout[:, 0], tight=f.Tout[:, 0]))
    if dparams is not None:
        check_dparams(dparams, b, n, tag, oracle)
    if gtab_scaled is not None:  # every touched entry within its bound, every untouched entry (A = 0) exactly 0
        note(tag + " table [hard]", check(gtab_scaled, t["grad"], t["A"], None, t["k"], t["n_terms"], "table gradient", floor=t["E"], tight=t["T"]))
