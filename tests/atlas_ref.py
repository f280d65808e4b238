"""The texture atlas restated in numpy (include/f2n_abi.h, "Texture atlas of a triangle mesh"): classify, order, offsets, place, the
texel map with both clamps, and the bilinear lookup, rounding by rounding.  Test infrastructure only: the product never imports it."""
import numpy as np

F32, F64 = np.float32, np.float64
DEGENERATE = 4
MAX_LOG_CAP = 13


def _pow2(size):
    return size >= 1 and (size & (size - 1)) == 0


def classify(verts, faces, density, max_log=7):
    """(log_s [F] int32, rot [F] int32); rot == 4 flags a degenerate face"""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    d = float(F32(density))
    if not (d > 0 and d < float("inf")) or not 2 <= max_log <= MAX_LOG_CAP:
        raise ValueError("density must be positive and finite, max_log in [2, 13]")
    nf = len(f)
    log_s, rot = np.full(nf, 2, np.int32), np.full(nf, DEGENERATE, np.int32)
    if nf == 0:
        return log_s, rot
    ok = ((f >= 0) & (f < len(v))).all(1)
    fi = np.where(ok[:, None], f, 0)
    if len(v) == 0:
        return log_s, rot
    P = v[fi].astype(F64)  # [F,3,3]
    ok &= np.isfinite(P).all((1, 2))
    with np.errstate(all="ignore"):
        p, q, e = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], P[:, 2] - P[:, 1]
        sq = lambda x: (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]  # noqa: E731
        l_ab, l_bc, l_ca = sq(p), sq(e), sq(q)
        n = np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)
        n2 = sq(n)
        ok &= n2 > 0
        need = np.maximum(4.0, np.ceil(np.sqrt(np.sqrt(n2)) * d) + 3.0)
    ls = np.full(nf, 2, np.int32)
    for k in range(2, max_log):
        ls = np.where((ls == k) & (float(1 << k) < need), k + 1, ls)
    r = np.zeros(nf, np.int32)
    longest = l_bc.copy()
    r = np.where(l_ca > longest, 1, r)
    longest = np.where(l_ca > longest, l_ca, longest)
    r = np.where(l_ab > longest, 2, r)
    return np.where(ok, ls, 2).astype(np.int32), np.where(ok, r, DEGENERATE).astype(np.int32)


def morton_decode(m):
    m = np.asarray(m, np.int64)
    x, y = np.zeros(m.shape, np.int64), np.zeros(m.shape, np.int64)
    for k in range(MAX_LOG_CAP):
        x |= ((m >> (2 * k)) & 1) << k
        y |= ((m >> (2 * k + 1)) & 1) << k
    return x, y


def morton_encode(x, y):
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    m = np.zeros(x.shape, np.int64)
    for k in range(MAX_LOG_CAP):
        m |= (((x >> k) & 1) << (2 * k)) | (((y >> k) & 1) << (2 * k + 1))
    return m


def layout(log_s, max_log=7):
    """order, blocks and offsets: dict of slot [F], block_log [B], block_faces [B,2], offsets [B+1] int64, size"""
    log_s = np.asarray(log_s, np.int32)
    nf = len(log_s)
    keys = np.sort((max_log - log_s.astype(np.int64)) * max(nf, 1) + np.arange(nf, dtype=np.int64))
    order, cls = keys % max(nf, 1), keys // max(nf, 1)
    ncls = max_log - 1
    n_c = np.bincount(cls, minlength=ncls).astype(np.int64)
    nb_c = (n_c + 1) // 2
    c0, b0 = np.cumsum(n_c) - n_c, np.cumsum(nb_c) - nb_c
    q = np.arange(nf, dtype=np.int64) - c0[cls]
    sl = (b0[cls] + q // 2) * 2 + (q & 1)
    B = int(nb_c.sum())
    slot = np.zeros(nf, np.int32)
    slot[order] = sl
    block_faces = np.full(B * 2, -1, np.int32)
    block_faces[sl] = order
    block_log = (max_log - np.repeat(np.arange(ncls), nb_c)).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.int64(1) << (2 * block_log.astype(np.int64)))]).astype(np.int64)
    size = 4
    while size * size < int(offsets[-1]):
        size *= 2
    return {"slot": slot, "block_log": block_log, "block_faces": block_faces.reshape(-1, 2), "offsets": offsets, "size": size}


def place(log_s, rot, lay):
    """uv [F,3,2] float32"""
    nf = len(log_s)
    uv = np.zeros((nf, 3, 2), F32)
    if nf == 0:
        return uv
    sl = lay["slot"].astype(np.int64)
    x0, y0 = morton_decode(lay["offsets"][sl >> 1])
    up = (sl & 1) != 0
    s = (1 << np.asarray(log_s, np.int64)).astype(F32)
    S = F32(lay["size"])
    half, far = F32(0.5), F32(2.5)
    c0 = np.where(up, s - half, half).astype(F32)
    c1 = np.where(up, far, s - far).astype(F32)
    cx = np.stack([c0, c1, c0], 1)  # chart corners 0, 1, 2
    cy = np.stack([c0, c0, c1], 1)
    r = np.asarray(rot, np.int64) & 3
    for j in range(3):
        k = (j - r + 3) % 3
        rows = np.arange(nf)
        uv[:, j, 0] = (x0.astype(F32) + cx[rows, k]) / S
        uv[:, j, 1] = (y0.astype(F32) + cy[rows, k]) / S
    return uv


def texels(verts, faces, rot, lay, clamp):
    """(tex_face [S,S] int32, tex_bary [S,S,3], tex_pos [S,S,3])"""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    S, offsets = lay["size"], lay["offsets"]
    B = len(lay["block_log"])
    y, x = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    m = morton_encode(x, y)
    tex_face = np.full((S, S), -1, np.int32)
    bary, pos = np.zeros((S, S, 3), F32), np.zeros((S, S, 3), F32)
    if B == 0 or len(f) == 0:
        return tex_face, bary, pos
    has = m < offsets[B]
    b = np.clip(np.searchsorted(offsets, m, side="right") - 1, 0, B - 1)
    x0, y0 = morton_decode(offsets[b])
    s = np.int64(1) << lay["block_log"][b].astype(np.int64)
    i, j = x - x0, y - y0
    up = i + j > s - 1
    face = lay["block_faces"][b, up.astype(np.int64)]
    rot = np.asarray(rot, np.int32)
    ok = has & (face >= 0) & (face < len(f))
    fc = np.where(ok, face, 0)
    ok &= (rot[fc] & DEGENERATE) == 0
    ok &= ((f[fc] >= 0) & (f[fc] < len(v))).all(-1)
    leg = (s - 3).astype(F32)
    with np.errstate(all="ignore"):
        u = np.where(up, s - 1 - i, i).astype(F32) / leg
        w = np.where(up, s - 1 - j, j).astype(F32) / leg
        w0 = (F32(1.0) - u) - w
        chart = np.stack([w0, u, w], -1).astype(F32)
        r = (rot[fc] & 3).astype(np.int64)
        bb = np.stack([np.take_along_axis(chart, ((k - r + 3) % 3)[..., None], -1)[..., 0] for k in range(3)], -1)
        if clamp:
            neg = (bb < 0).any(-1)
            c = np.maximum(bb, F32(0.0))
            tot = (c[..., 0] + c[..., 1]) + c[..., 2]
            bb = np.where(neg[..., None], c / tot[..., None], bb).astype(F32)
        P = v[np.where(ok[..., None], f[fc], 0)] if len(v) else np.zeros((S, S, 3, 3), F32)  # [S,S,3 corners,3]
        pp = (bb[..., 0, None] * P[..., 0, :] + bb[..., 1, None] * P[..., 1, :]) + bb[..., 2, None] * P[..., 2, :]
    tex_face[ok] = face[ok]
    bary[ok] = bb[ok]
    pos[ok] = pp[ok].astype(F32)
    return tex_face, bary, pos


def sample(tex, uv):
    """[N,C] float32: the bilinear lookup of tex [S,S,C] at uv [N,2]"""
    tex = np.ascontiguousarray(tex, F32)
    S, C = tex.shape[0], tex.shape[2]
    uv = np.ascontiguousarray(uv, F32).reshape(-1, 2)
    fin = np.isfinite(uv).all(1)
    with np.errstate(all="ignore"):
        u, w = np.where(fin, uv[:, 0], F32(0)), np.where(fin, uv[:, 1], F32(0))
        top, Sf, half, one = F32(S - 1), F32(S), F32(0.5), F32(1.0)
        fx = np.minimum(np.maximum(u * Sf - half, F32(0)), top)
        fy = np.minimum(np.maximum(w * Sf - half, F32(0)), top)
        gx, gy = np.floor(fx), np.floor(fy)
        ax, ay = fx - gx, fy - gy
        cx, cy = one - ax, one - ay
        x0, y0 = gx.astype(np.int64), gy.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, S - 1), np.minimum(y0 + 1, S - 1)
        n = lambda a: a[:, None]  # noqa: E731
        out = ((tex[y0, x0] * n(cx * cy) + tex[y0, x1] * n(ax * cy)) + tex[y1, x0] * n(cx * ay)) + tex[y1, x1] * n(ax * ay)
    return np.where(fin[:, None], out, F32(0)).astype(F32).reshape(-1, C)


def min_layout_size(n_faces):
    size = 4
    while size * size < 16 * ((n_faces + 1) // 2):
        size *= 2
    return size


def atlas(verts, faces, density, max_size=8192, max_log=7, classify_fn=classify, place_fn=place):
    """The fit loop of host.mesh_atlas: (uv, size, layout dict with log_s and rot added, density_used).  classify_fn / place_fn let a
    library stand in for the restatement's kernels."""
    if not _pow2(int(max_size)) or max_size < 4:
        raise ValueError("max_size must be a power of two, at least 4")
    nf = len(np.asarray(faces).reshape(-1, 3))
    if min_layout_size(nf) > max_size:
        raise ValueError("the mesh does not fit the atlas even at the smallest block size")
    d = float(F32(density))
    for _ in range(33):
        log_s, rot = classify_fn(verts, faces, d, max_log)
        lay = layout(log_s, max_log)
        if lay["size"] <= max_size:
            lay["log_s"], lay["rot"] = log_s, rot
            return place_fn(log_s, rot, lay), lay["size"], lay, d
        d = float(F32(d * 0.5))
    raise ValueError("the mesh does not fit the atlas after 32 halvings of the density")
