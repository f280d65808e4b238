"""numpy restatement of the mesh refinement of include/f2n_abi.h ("Mesh refinement"): the vertex one-ring, the Taubin smoothing pass,
the trust-region clamp, the level-set step and the face quality -- the tests' reference, written from the definitions in the header,
not from the kernels.  float32 arrays keep every operation at one float32 rounding, float64 arrays at one float64 rounding; numpy
contracts nothing into an FMA."""
import numpy as np

F32 = np.float32
EMPTY, CONVERGED, STEP_CLAMPED, MOVE_CLAMPED = 1, 2, 4, 8
QUALITY_K = 3.4641016151377544  # F2N_FACE_QUALITY_K: the double nearest 2 sqrt(3)
MOVE_CLAMP_ROUNDS = 16  # F2N_MOVE_CLAMP_ROUNDS


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def valid_faces(faces, n_verts):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < n_verts)).all(1)
    return ok & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def ring_keys(faces, n_verts):
    """keys [F,6] int64 (f2n_mesh_ring_keys)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, n_verts)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    V = np.int64(n_verts)
    k = np.stack([a * V + b, b * V + a, b * V + c, c * V + b, c * V + a, a * V + c], 1)
    return np.where(ok[:, None], k, -1).astype(np.int64)


def edges_of(keys):
    """(edge_keys [E], edge_uses [E]) int64: the caller's sort and run-length encoding"""
    k = np.sort(np.asarray(keys, np.int64).reshape(-1))
    k = k[k >= 0]
    uk, uses = np.unique(k, return_counts=True)
    return uk.astype(np.int64), uses.astype(np.int64)


def ring_fill(n_verts, edge_keys, edge_uses):
    """(ring_start_end [V,2] int32, ring [E] int32, pinned [V] uint8, edge_counts [2] int32) (f2n_mesh_ring_fill)"""
    V = np.int64(n_verts)
    v = np.arange(n_verts, dtype=np.int64)
    s, e = np.searchsorted(edge_keys, v * V, "left"), np.searchsorted(edge_keys, (v + 1) * V, "left")
    se = np.stack([s, e], 1).astype(np.int32).reshape(-1, 2)
    owner = edge_keys // V if n_verts > 0 else edge_keys
    ring = (edge_keys - owner * V).astype(np.int32)
    off = np.zeros(n_verts, np.int64)
    np.add.at(off, owner[edge_uses != 2], 1)
    pinned = ((s == e) | (off > 0)).astype(np.uint8)
    lower = ring > owner
    counts = np.array([(lower & (edge_uses == 1)).sum(), (lower & (edge_uses >= 3)).sum()], np.int32)
    return se, ring, pinned, counts


def ring(faces, n_verts):
    """(ring_start_end, ring, pinned, edge_counts) of a mesh"""
    return ring_fill(n_verts, *edges_of(ring_keys(faces, n_verts)))


def smooth_pass(verts, se, rg, pinned, factor):
    """one f2n_mesh_smooth pass: out [V,3] f32"""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    n = len(v)
    out = v.copy()
    if n == 0:
        return out
    s, e = se[:, 0].astype(np.int64), se[:, 1].astype(np.int64)
    cnt = e - s
    fin = np.isfinite(v).all(1)
    move = (pinned == 0) & (s >= 0) & (s < e) & (e <= len(rg)) & fin
    # the ring's sums in ring order, fp64, a round of the loop per position in the ring
    acc = np.zeros((n, 3), np.float64)
    live = move.copy()
    for j in range(int(cnt[move].max()) if move.any() else 0):
        at = live & (cnt > j)
        idx = np.flatnonzero(at)
        w = rg[s[idx] + j].astype(np.int64)
        good = (w >= 0) & (w < n)
        good[good] &= fin[w[good]]
        live[idx[~good]] = False
        idx, w = idx[good], w[good]
        acc[idx] = acc[idx] + v[w].astype(np.float64)
    idx = np.flatnonzero(live)
    with np.errstate(all="ignore"):
        m = acc[idx] / cnt[idx].astype(np.float64)[:, None]
        p = v[idx].astype(np.float64)
        d = m - p
        t = np.float64(factor) * d
        out[idx] = (p + t).astype(F32)
    return out


def move_clamp(p0, pts, max_move):
    """(pts clamped to the ball of radius max_move around p0, fp32; the mask of the points that moved) (f2n_mesh_move_clamp)"""
    p0, x = np.asarray(p0, F32).reshape(-1, 3), np.array(pts, F32).reshape(-1, 3)
    r = F32(max_move)
    with np.errstate(all="ignore"):
        u = x - p0
        l = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
        act = l > r
        k = r / l
        todo = act.copy()
        for _ in range(MOVE_CLAMP_ROUNDS):
            x[todo] = (p0 + u * k[:, None])[todo]
            w = x - p0
            lw = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
            todo = todo & (lw > r)
            if not todo.any():
                break
            k = np.where(todo, (k * (r / lw)) * F32(1.0 - 2.0 ** -21), k)
    return x, act


def smooth(verts, faces, passes, lam=0.5, mu=-0.53, max_move=float("inf")):
    """host.mesh_smooth: `passes` lambda|mu pairs, then the clamp against the input when max_move is finite"""
    v0 = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    se, rg, pinned, _ = ring(faces, len(v0))
    v = v0.copy()
    for _ in range(passes):
        v = smooth_pass(v, se, rg, pinned, lam)
        v = smooth_pass(v, se, rg, pinned, mu)
    if passes > 0 and np.isfinite(max_move):
        v, _ = move_clamp(v0, v, max_move)
    return v


def level_state(n):
    """the arrays f2n_level_step keeps between calls"""
    return {"cand": np.zeros((n, 3), F32), "best": np.zeros((n, 3), F32), "h_best": np.zeros(n, F32), "g_best": np.zeros((n, 3), F32),
            "scale": np.zeros(n, F32), "status": np.zeros(n, np.int32), "evals": np.zeros(n, np.int32)}


def _sumsq(a):
    return (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]


def level_step(first, propose, p0, sigma, grad, h, tol, max_step, max_move, st):
    """f2n_level_step on the state dict st (level_state), in place"""
    p0 = np.asarray(p0, F32).reshape(-1, 3)
    sigma, h, grad = np.asarray(sigma, F32), np.asarray(h, F32), np.asarray(grad, F32).reshape(-1, 3)
    tol, max_step, max_move = F32(tol), F32(max_step), F32(max_move)
    n = len(p0)
    status = np.zeros(n, np.int32) if first else st["status"].copy()
    done = (status & (EMPTY | CONVERGED)) != 0
    c = st["cand"].copy()
    with np.errstate(all="ignore"):
        g = grad / sigma[:, None]
        q = _sumsq(g)
        evaluable = (sigma > 0) & np.isfinite(sigma) & np.isfinite(h) & np.isfinite(g).all(1) & (q != 0)
        if first:
            evals = np.ones(n, np.int32)
            b, hb, a = c.copy(), h.copy(), np.ones(n, F32)
            gb = np.where(evaluable[:, None], g, F32(0)).astype(F32)
            status = np.where(evaluable, 0, EMPTY).astype(np.int32)
        else:
            evals = st["evals"] + 1
            accept = evaluable & (np.abs(h) <= np.abs(st["h_best"]))
            b = np.where(accept[:, None], c, st["best"])
            gb = np.where(accept[:, None], g, st["g_best"]).astype(F32)
            hb = np.where(accept, h, st["h_best"])
            a = np.where(accept, st["scale"], st["scale"] * F32(0.5))
        conv = ((status & EMPTY) == 0) & (np.abs(hb) <= tol)
        status = np.where(conv, status | CONVERGED, status)
        go = ((status & (EMPTY | CONVERGED)) == 0) & bool(propose)
        qb = _sumsq(gb)
        t = -((a * hb) / qb)
        d = t[:, None] * gb
        l = np.sqrt(_sumsq(d))
        long = l > max_step
        d = np.where(long[:, None], d * (max_step / l)[:, None], d)
        status = np.where(go & long, status | STEP_CLAMPED, status)
        nxt, moved = move_clamp(p0, b + d, max_move)
        status = np.where(go & moved, status | MOVE_CLAMPED, status)
        nxt = np.where(np.isfinite(nxt).all(1)[:, None], nxt, b)
        nxt = np.where(go[:, None], nxt, b)
    new = {"cand": nxt, "best": b, "h_best": hb, "g_best": gb, "scale": a, "status": status, "evals": evals}
    for key, val in new.items():
        old = st[key]
        if first:
            st[key] = np.ascontiguousarray(val, old.dtype)
        elif key == "cand":
            st[key] = np.ascontiguousarray(np.where(done[:, None], st["best"], val), old.dtype)
        else:
            keep = done[:, None] if val.ndim == 2 else done
            st[key] = np.ascontiguousarray(np.where(keep, old, val), old.dtype)
    return st


def face_quality(verts, faces):
    """quality [F] fp64 (f2n_mesh_face_quality)"""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    out = np.zeros(len(f), np.float64)
    ok = valid_faces(f, len(v))
    if not ok.any():
        return out
    A, B, C = (v[f[ok, k]].astype(np.float64) for k in range(3))
    fin = np.isfinite(A).all(1) & np.isfinite(B).all(1) & np.isfinite(C).all(1)
    with np.errstate(all="ignore"):
        p, q, r = B - A, C - A, C - B
        nx = p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1]
        ny = p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2]
        nz = p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]
        area2 = np.sqrt((nx * nx + ny * ny) + nz * nz)
        L = (_sumsq(p) + _sumsq(q)) + _sumsq(r)
        val = np.where(L > 0, (QUALITY_K * area2) / L, 0.0)
    out[ok] = np.where(fin, val, np.nan)
    return out


def face_normals(verts, faces):
    """unnormalised face normals [F,3] fp64 (for the flipped-face count; zeros for invalid faces)"""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, len(v))
    n = np.zeros((len(f), 3))
    n[ok] = np.cross(v[f[ok, 1]] - v[f[ok, 0]], v[f[ok, 2]] - v[f[ok, 0]])
    return n
