"""numpy restatement of the analytic density gradient (include/f2n_abi.h: f2n_field_density_grad, f2n_hash_pos_grad,
f2n_density_grad_scatter), built from the oracle's pieces: oracle.capi.hash_cell for the corner positions, oracle.capi.hash_fwd for the
h16 features, oracle.capi.warp for the warp and its Jacobian, oracle.pipeline.HashGrid for the grid.

    w   = warp_t(p)
    q_l = ((w + 1) * 0.5) * scale_l + bias_{l,t}
    x   = h16 hash features [32]       (trilinear blend of 8 corners x 2 channels, 16 levels)
    f0  = (W2 relu(W1 x))[0]
    df0/dx = W1^T (m . W2[0,:]),  m_j = ((W1 x)_j > 0)
    df0/dw = sum_l (scale_l / 2) sum_c df0/dx_{l,c} sum_d d(weight_d)/d(a, b, c) v_{l,d,c}      (corner bit 2 = x, 1 = y, 0 = z)
    grad_p sigma = sigma J_t(p)^T df0/dw

Every input (table entries, weights, features x, the float32 points, the float32 Jacobian) is taken as exact.  Each quantity can be
evaluated in float64 (the reference) or in float32 in the kernels' operation order (to measure what float32 arithmetic costs: the
tests' bar is 8 x that discrepancy).  Next to every gradient component comes S, the sum of the absolute values of ALL its addends
(through the whole chain, in float64): errors are measured relative to S, which is insensitive to cancellation and summation order."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import capi as oc  # noqa: E402

F32, F64 = np.float32, np.float64
TIE = 2.0 ** -20


class Cells:
    """The 16 cells of every point: corner values v [n,16,8,2] (exact h16 values as float64), the float32 floor fl [n,16,3] that chose
    the cell, and the float32 level constants (scale [16], bias [n,16,3])."""

    def __init__(self, grid, w32, vol):
        w32 = np.ascontiguousarray(w32, F32).reshape(-1, 3)
        vol = np.ascontiguousarray(vol, np.int32).reshape(-1)
        n, V = len(w32), grid.n_volumes
        self.n, self.w32, self.vol, self.scale = n, w32, vol, np.asarray(grid.scales, F32)
        q01 = ((w32 + F32(1.)) * F32(.5)).astype(F32)
        prim = np.asarray(grid.prim_pool, np.int32).reshape(16, V, 3)
        bias = np.asarray(grid.bias_pool, F32).reshape(16, V, 3)
        table = oc.h2f(grid.table_h).astype(F64)  # flat halves, exact
        self.v = np.empty((n, 16, 8, 2), F64)
        self.fl = np.empty((n, 16, 3), F32)
        self.bias = np.ascontiguousarray(bias[:, vol].transpose(1, 0, 2))  # [n,16,3]
        for l in range(16):
            mul = np.full(n, self.scale[l], F32)
            pos, _ = oc.hash_cell(q01, mul, np.ascontiguousarray(prim[l, vol]), np.ascontiguousarray(bias[l, vol]),
                                  np.full(n, grid.local_size[l], np.uint32))
            base = int(grid.local_idx[l])
            for c in range(2):
                self.v[:, l, :, c] = table[base + pos.astype(np.int64) * 2 + c]
            q = (q01 * self.scale[l] + bias[l, vol]).astype(F32)  # mul, then add: f2n_hash_cell
            self.fl[:, l] = np.floor(q)

    def frac(self, w, dtype):
        """a, b, c [n,16,3] at the points w (default positions: self.w32), relative to the cells' own floor."""
        w = np.asarray(w, dtype).reshape(-1, 1, 3)
        q = ((w + dtype(1.)) * dtype(.5)) * self.scale.astype(dtype)[None, :, None] + self.bias.astype(dtype)
        return (q - self.fl.astype(dtype)).astype(dtype)

    def face_distance(self):
        """The distance of every point to the nearest cell face of any level, in cells of the FINEST level (float64)."""
        f = self.frac(self.w32, F64)
        rel = (self.scale[15].astype(F64) / self.scale.astype(F64))[None, :, None]
        return (np.minimum(f, 1.0 - f) * rel).min(axis=(1, 2))


def _weights(f):
    """The eight weights of f2n_hash_cell [.., 8] from fractions [.., 3]."""
    a, b, c = f[..., 0], f[..., 1], f[..., 2]
    one = f.dtype.type(1.)
    return np.stack([(one - a) * (one - b) * (one - c), (one - a) * (one - b) * c, (one - a) * b * (one - c), (one - a) * b * c,
                     a * (one - b) * (one - c), a * (one - b) * c, a * b * (one - c), a * b * c], -1)


def _weight_grads(f):
    """d(weight_d)/d(a, b, c): [.., 3, 8]."""
    a, b, c = f[..., 0], f[..., 1], f[..., 2]
    one = f.dtype.type(1.)
    wa, wb, wc = [one - a, a], [one - b, b], [one - c, c]
    sg = [-one, one]
    out = np.empty(f.shape[:-1] + (3, 8), f.dtype)
    for d in range(8):
        x, y, z = (d >> 2) & 1, (d >> 1) & 1, d & 1
        out[..., 0, d] = sg[x] * (wb[y] * wc[z])
        out[..., 1, d] = sg[y] * (wa[x] * wc[z])
        out[..., 2, d] = sg[z] * (wa[x] * wb[y])
    return out


def split_params(mlp_params, d_hidden=64):
    """(W1 [d_hidden,32], W2 row 0 [d_hidden]) as exact h16 values in float64 (one hidden layer)."""
    p = oc.h2f(oc.f2h(np.asarray(mlp_params, F32))).astype(F64)
    return p[:d_hidden * 32].reshape(d_hidden, 32), p[d_hidden * 32:d_hidden * 32 + d_hidden].copy()


def forward64(cells, W1, w2, w=None):
    """f0 in float64 without any activation rounding, at points w (default: the cells' own points; w must stay inside their cells)."""
    f = cells.frac(cells.w32 if w is None else w, F64)
    x = (_weights(f)[..., None] * cells.v).sum(2).reshape(cells.n, 32)  # [n,16,2] -> feature 2 l + c
    return np.maximum(x @ W1.T, 0.0) @ w2


def relu_ties(x, W1):
    """The exclusion: a point where some hidden unit has |(W1 x)_j| <= 2^-20 sum_k |W1[j,k] x_k| (float64)."""
    x = np.asarray(x, F64)
    return (np.abs(x @ W1.T) <= TIE * (np.abs(x) @ np.abs(W1).T)).any(1)


def df0_dx(x_h, W1, w2, dtype=F64):
    """df0/dx [n,32] from the h16 features x_h (uint16 bits) and its S [n,32].  float32: the kernel's order (the pre-activation summed
    over k in order, dx summed over the hidden units in order; a product of two h16 values is exact)."""
    x = oc.h2f(np.asarray(x_h, np.uint16)).astype(F64)
    mask64 = (x @ W1.T) > 0
    S = mask64.astype(F64) @ np.abs(W1 * w2[:, None])
    if dtype is F64:
        return (mask64 * w2[None, :]) @ W1, S
    x32, W32, g32 = x.astype(F32), W1.astype(F32), w2.astype(F32)
    dx = np.zeros((len(x), 32), F32)
    for j in range(W1.shape[0]):
        pre = W32[j, 0] * x32[:, 0]
        for k in range(1, 32):
            pre = pre + W32[j, k] * x32[:, k]
        gj = np.where(pre > 0, g32[j], F32(0.)).astype(F32)
        dx = dx + W32[j][None, :] * gj[:, None]
    return dx, S


def df0_dw(cells, dx, dtype=F64, S_dx=None):
    """df0/dw [n,3] from df0/dx [n,32], and its S [n,3].  S_dx (the S of dx) carries the chain's addends through; without it |dx| is
    used (dx taken as exact input).  float32: the kernel's order -- per level the corner-pair differences weighted by the other two
    axes' weights, the two channels, times scale / 2; levels added in pairs, pairs in order."""
    n = cells.n
    dx64 = np.asarray(dx, F64).reshape(n, 16, 2)
    adx = np.abs(dx64) if S_dx is None else np.asarray(S_dx, F64).reshape(n, 16, 2)
    f64 = cells.frac(cells.w32, F64)
    dW = _weight_grads(f64)  # [n,16,3,8]
    hs = (cells.scale.astype(F64) * 0.5)[None, :, None]
    S = (hs * np.einsum("nlc,nlkd,nldc->nlk", adx, np.abs(dW), np.abs(cells.v))).sum(1)
    if dtype is F64:
        return (hs * np.einsum("nlc,nlkd,nldc->nlk", dx64, dW, cells.v)).sum(1), S
    f = cells.frac(cells.w32, F32)
    v = cells.v.astype(F32)
    d = np.asarray(dx, F32).reshape(n, 16, 2)
    one = F32(1.)

    def blend_grad(vv, a, b, c):
        a0, b0, c0 = one - a, one - b, one - c
        return [(((b0 * c0) * (vv[:, 4] - vv[:, 0]) + (b0 * c) * (vv[:, 5] - vv[:, 1])) + (b * c0) * (vv[:, 6] - vv[:, 2])) + (b * c) * (vv[:, 7] - vv[:, 3]),
                (((a0 * c0) * (vv[:, 2] - vv[:, 0]) + (a0 * c) * (vv[:, 3] - vv[:, 1])) + (a * c0) * (vv[:, 6] - vv[:, 4])) + (a * c) * (vv[:, 7] - vv[:, 5]),
                (((a0 * b0) * (vv[:, 1] - vv[:, 0]) + (a0 * b) * (vv[:, 3] - vv[:, 2])) + (a * b0) * (vv[:, 5] - vv[:, 4])) + (a * b) * (vv[:, 7] - vv[:, 6])]

    t = np.empty((n, 16, 3), F32)
    for l in range(16):
        a, b, c = f[:, l, 0], f[:, l, 1], f[:, l, 2]
        d0, d1 = blend_grad(v[:, l, :, 0], a, b, c), blend_grad(v[:, l, :, 1], a, b, c)
        hs32 = cells.scale[l] * F32(.5)
        for k in range(3):
            t[:, l, k] = hs32 * (d[:, l, 0] * d0[k] + d[:, l, 1] * d1[k])
    pair = t[:, 0::2] + t[:, 1::2]
    out = pair[:, 0]
    for p in range(1, 8):
        out = out + pair[:, p]
    return out.astype(F32), S


def grad_sigma(sigma, jac, g, dtype=F64, S_g=None):
    """sigma J^T g [n,3] (sigma [n] and the Jacobian [n,3,3] as given: exact inputs) and its S.  float32: the kernel's order."""
    jac64, g64, s64 = np.asarray(jac, F64), np.asarray(g, F64), np.asarray(sigma, F64)
    ag = np.abs(g64) if S_g is None else np.asarray(S_g, F64)
    S = s64[:, None] * np.einsum("nrc,nr->nc", np.abs(jac64), ag)
    if dtype is F64:
        return s64[:, None] * np.einsum("nrc,nr->nc", jac64, g64), S
    j, gg, s = np.asarray(jac, F32), np.asarray(g, F32), np.asarray(sigma, F32)
    out = np.stack([s * (j[:, 0, c] * gg[:, 0] + (j[:, 1, c] * gg[:, 1] + j[:, 2, c] * gg[:, 2])) for c in range(3)], 1)
    return out.astype(F32), S


def rel_err(got, ref64, S, keep=None):
    """max_i |got_i - ref_i| / S_i over the kept points (components with S = 0 must agree exactly)."""
    got, ref64, S = np.asarray(got, F64), np.asarray(ref64, F64), np.asarray(S, F64)
    if keep is not None:
        got, ref64, S = got[keep], ref64[keep], S[keep]
    if got.size == 0:
        return 0.0
    diff = np.abs(got - ref64)
    assert (diff[S == 0] == 0).all()
    return float((diff[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0


def field_chain(grid, mlp_params, w32, vol, x_h=None, d_hidden=64):
    """The whole df0/dw chain of n warped points for a one-hidden-layer field: dict with the float64 reference (dx, g), the float32
    evaluation (dx32, g32), the S of both stages (S_dx, S_g), the tie exclusion `ties` and the cells."""
    cells = Cells(grid, w32, vol)
    W1, w2 = split_params(mlp_params, d_hidden)
    if x_h is None:
        q01 = ((cells.w32 + F32(1.)) * F32(.5)).astype(F32)
        x_h = oc.hash_fwd(grid.table_h, grid.prim_pool, grid.local_idx, grid.local_size, grid.bias_pool, q01, cells.vol, grid.n_volumes, grid.scales)
    dx, S_dx = df0_dx(x_h, W1, w2, F64)
    dx32, _ = df0_dx(x_h, W1, w2, F32)
    g, S_g = df0_dw(cells, dx, F64, S_dx)
    g32, _ = df0_dw(cells, dx32, F32, S_dx)
    return dict(cells=cells, W1=W1, w2=w2, x_h=x_h, dx=dx, dx32=dx32, S_dx=S_dx, g=g, g32=g32, S_g=S_g,
                ties=relu_ties(oc.h2f(x_h), W1))
