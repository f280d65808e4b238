"""float32 numpy restatement of the TSDF entry points of include/f2n_abi.h (f2n_tsdf_integrate, f2n_tsdf_finalize,
f2n_mesh_count_masked + f2n_mesh_emit): the tests' reference, written from the definitions in the header, not from the kernels.  Every
operation is one float32 rounding in the header's order (numpy never contracts a product and a sum), so the device must give its bits."""
import numpy as np

import mesh_ref as mr

F32 = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all()


def distort(k, u, v):
    """Step 5 of f2n_tsdf_integrate: the distortion of the camera model at (u, v), float32 in the header's order."""
    k1, k2, p1, p2 = (F32(x) for x in k)
    u2, uv, v2 = u * u, u * v, v * v
    r2 = u2 + v2
    radial = k1 * r2 + (k2 * r2) * r2
    du = (u * radial + (F32(2) * p1) * uv) + p2 * (r2 + F32(2) * u2)
    dv = (v * radial + (F32(2) * p2) * uv) + p1 * (r2 + F32(2) * v2)
    return du, dv


def voxel_points(lo, step, nx, ny, nz):
    cx, cy, cz = mr.grid_points(lo, step, (nx, ny, nz))
    idx = np.arange(nx * ny * nz)
    return cx[idx % nx], cy[(idx // nx) % ny], cz[idx // (nx * ny)]


def integrate(S, W, lo, step, nx, ny, nz, poses, intri, dist, depth, conf, trunc, stats=None):
    """(S, W) after the views of depth [V,h,w] were added in index order; the inputs are not modified.  stats (a dict, optional)
    receives how many (voxel, view) pairs took each exit of the header's twelve steps."""
    S = np.array(S, F32).reshape(-1).copy()
    W = np.array(W, F32).reshape(-1).copy()
    poses, intri, dist = np.asarray(poses, F32).reshape(-1, 3, 4), np.asarray(intri, F32).reshape(-1, 3, 3), np.asarray(dist, F32).reshape(-1, 4)
    depth = np.asarray(depth, F32)
    V, h, w = depth.shape
    trunc = F32(trunc)
    px, py, pz = voxel_points(lo, step, nx, ny, nz)
    st = dict(behind=0, outside=0, no_depth=0, no_conf=0, far_behind=0, at_minus_trunc=0, clamped=0, used=0)
    with np.errstate(all="ignore"):
        for v in range(V):
            P, K = poses[v], intri[v]
            q = [px - P[0, 3], py - P[1, 3], pz - P[2, 3]]
            c = [P[0, j] * q[0] + (P[1, j] * q[1] + P[2, j] * q[2]) for j in range(3)]
            s = -c[2]
            front = s > 0
            u, vv = c[0] / s, (-c[1]) / s
            du, dv = distort(dist[v], u, vv)
            x = K[0, 0] * (u + du) + K[0, 2]
            y = K[1, 1] * (vv + dv) + K[1, 2]
            fb, fa = np.floor(x), np.floor(y)
            inside = front & (fa >= 0) & (fa < F32(h)) & (fb >= 0) & (fb < F32(w))
            ia, ib = np.where(inside, fa, 0).astype(np.int64), np.where(inside, fb, 0).astype(np.int64)
            D = depth[v, ia, ib]
            has = inside & (D > 0)
            wgt = np.asarray(conf, F32)[v, ia, ib] if conf is not None else np.ones_like(D)
            weighted = has & (wgt > 0)
            sdf = D - np.sqrt(q[0] * q[0] + (q[1] * q[1] + q[2] * q[2]))
            ok = weighted & ~(sdf < -trunc)
            d = sdf / trunc
            d = np.where(d < 1, d, F32(1))
            S = np.where(ok, S + wgt * d, S).astype(F32)
            W = np.where(ok, W + wgt, W).astype(F32)
            st["behind"] += int((~front).sum()); st["outside"] += int((front & ~inside).sum()); st["no_depth"] += int((inside & ~has).sum())
            st["no_conf"] += int((has & ~weighted).sum()); st["far_behind"] += int((weighted & ~ok).sum())
            st["at_minus_trunc"] += int((ok & (sdf == -trunc)).sum()); st["clamped"] += int((ok & (sdf >= trunc)).sum()); st["used"] += int(ok.sum())
    if stats is not None:
        stats.update(st)
    return S.reshape(nz, ny, nx), W.reshape(nz, ny, nx)


def project(lo, step, nx, ny, nz, pose, K, k, h, w):
    """Per voxel of one view: (visible, a, b, |q|) by the header's steps 1-7 and 10 (what the case builder plants exact values with)."""
    px, py, pz = voxel_points(lo, step, nx, ny, nz)
    P, K = np.asarray(pose, F32), np.asarray(K, F32)
    with np.errstate(all="ignore"):
        q = [px - P[0, 3], py - P[1, 3], pz - P[2, 3]]
        c = [P[0, j] * q[0] + (P[1, j] * q[1] + P[2, j] * q[2]) for j in range(3)]
        s = -c[2]
        u, vv = c[0] / s, (-c[1]) / s
        du, dv = distort(k, u, vv)
        fb, fa = np.floor(K[0, 0] * (u + du) + K[0, 2]), np.floor(K[1, 1] * (vv + dv) + K[1, 2])
        vis = (s > 0) & (fa >= 0) & (fa < F32(h)) & (fb >= 0) & (fb < F32(w))
        r = np.sqrt(q[0] * q[0] + (q[1] * q[1] + q[2] * q[2]))
    return vis, np.where(vis, fa, 0).astype(np.int64), np.where(vis, fb, 0).astype(np.int64), r


def finalize(S, W, min_weight):
    S, W = np.asarray(S, F32), np.asarray(W, F32)
    with np.errstate(all="ignore"):
        valid = (W >= F32(min_weight)) & (W > 0)
        g = np.where(valid, (-S) / W, F32(0)).astype(F32)
    return g, valid.astype(np.uint8)


# ---- the masked mesher -------------------------------------------------------------------------------------------------------------
def observed_cells(valid):
    """[nz-1, ny-1, nx-1] bool: all eight corners of the cell are valid."""
    v = np.asarray(valid) != 0
    out = np.ones(tuple(n - 1 for n in v.shape), bool)
    for o in range(8):
        dx, dy, dz = o & 1, (o >> 1) & 1, (o >> 2) & 1
        out &= v[dz:v.shape[0] - 1 + dz, dy:v.shape[1] - 1 + dy, dx:v.shape[2] - 1 + dx]
    return out


def marching_tets_masked(g, level, valid, lo=(0.0, 0.0, 0.0), step=1.0):
    """The rules of f2n_mesh_count_masked + f2n_mesh_emit: (verts, faces, vert_keys [(owner corner, edge type)], face_cells [cell index
    (x fastest over the (nx-1)(ny-1)(nz-1) cells)], edge_mask [N] uint8).  The unmasked rules are those of mesh_ref.marching_tets."""
    g = np.asarray(g, F32)
    nz, ny, nx = g.shape
    level = F32(level)
    inside = g > level
    obs = observed_cells(valid)
    cx, cy, cz = mr.grid_points(lo, step, (nx, ny, nz))
    flat_in, flat_g = inside.reshape(-1), g.reshape(-1)

    def cell_ok(x, y, z):
        return 0 <= x < nx - 1 and 0 <= y < ny - 1 and 0 <= z < nz - 1 and bool(obs[z, y, x])

    cand = []
    edge_mask = np.zeros(nx * ny * nz, np.uint8)
    for c in range(nx * ny * nz):
        x, y, z = c % nx, (c // nx) % ny, c // (nx * ny)
        for t, o in enumerate(mr.EDGE_OFFSETS):
            dx, dy, dz = o & 1, (o >> 1) & 1, (o >> 2) & 1
            if x + dx >= nx or y + dy >= ny or z + dz >= nz:
                continue
            b = c + dx + dy * nx + dz * nx * ny
            if flat_in[c] == flat_in[b]:
                continue
            # the cells whose Kuhn tetrahedra use the edge: c - d, d over the subsets of the axes the edge does not run along
            if not any(cell_ok(x - (d & 1), y - ((d >> 1) & 1), z - ((d >> 2) & 1)) for d in range(8) if not d & o):
                continue
            cand.append((c, t, b))
            edge_mask[c] |= 1 << t
    cand.sort()
    vid, verts = {}, []
    for c, t, b in cand:
        ga, gb = flat_g[c], flat_g[b]
        s = F32((level - ga) / (gb - ga))
        pa = np.array([cx[c % nx], cy[(c // nx) % ny], cz[c // (nx * ny)]], F32)
        pb = np.array([cx[b % nx], cy[(b // nx) % ny], cz[b // (nx * ny)]], F32)
        vid[(c, t)] = len(verts)
        verts.append((pa + s * (pb - pa)).astype(F32))
    faces, face_cells = [], []
    for z in range(nz - 1):
        for y in range(ny - 1):
            for x in range(nx - 1):
                if not obs[z, y, x]:
                    continue
                cm = [bool(inside[z + ((o >> 2) & 1), y + ((o >> 1) & 1), x + (o & 1)]) for o in range(8)]
                if all(cm) or not any(cm):
                    continue
                for axes in mr.TET_AXES:
                    tv = [0, axes[0], axes[0] | axes[1], 7]
                    ins = [cm[o] for o in tv]
                    k = sum(ins)
                    if k == 0 or k == 4:
                        continue

                    def vert_of(oa, ob):
                        lo_o = oa if (oa & ob) == oa else ob
                        t = mr.EDGE_OFFSETS.index(oa ^ ob)
                        c = (z + ((lo_o >> 2) & 1)) * nx * ny + (y + ((lo_o >> 1) & 1)) * nx + (x + (lo_o & 1))
                        return vid[(c, t)]

                    I = [tv[i] for i in range(4) if ins[i]]
                    O = [tv[i] for i in range(4) if not ins[i]]
                    if k == 1 or k == 3:
                        lone = I[0] if k == 1 else O[0]
                        tris = [[vert_of(lone, o) for o in tv if o != lone]]
                    else:
                        (i, j), (kk, ll) = I, O
                        tris = [[vert_of(i, kk), vert_of(i, ll), vert_of(j, ll)], [vert_of(i, kk), vert_of(j, ll), vert_of(j, kk)]]
                    faces.extend(tris)
                    face_cells.extend([(z * (ny - 1) + y) * (nx - 1) + x] * len(tris))
                    mr._fix_winding(faces, len(tris), I, O, np.mean([mr._off(o) for o in I], 0), np.mean([mr._off(o) for o in O], 0), vert_of)
    return (np.array(verts, F32).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3), [(c, t) for c, t, _ in cand],
            np.array(face_cells, np.int64), edge_mask)


def check_masked_mesh(verts, faces, g, level, valid, lo, step):
    """The properties the header promises of a masked mesh (verts / faces: the device's or the restatement's): every vertex is used by a
    face, every face lies in a cell with eight valid corners -- found from the face's own vertex positions, not from any bookkeeping."""
    verts, faces = np.asarray(verts), np.asarray(faces)
    assert faces.min(initial=0) >= 0 and faces.max(initial=-1) < len(verts)
    assert len(np.unique(faces)) == len(verts)  # every vertex is used by a face
    if not len(faces):
        return
    obs = observed_cells(valid)
    tri = verts[faces].astype(np.float64)  # [F,3,3]: a face lies inside one cell; its centroid is strictly inside that cell
    cell = np.floor((tri.mean(1) - np.asarray(lo, np.float64)[None]) / float(step)).astype(np.int64)
    nz, ny, nx = np.asarray(g).shape
    assert (cell >= 0).all() and (cell[:, 0] < nx - 1).all() and (cell[:, 1] < ny - 1).all() and (cell[:, 2] < nz - 1).all()
    assert obs[cell[:, 2], cell[:, 1], cell[:, 0]].all()  # no face survives in a cell with an invalid corner


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def scaled_intrinsics(intri, image_hw, h, w):
    """intri [V,3,3] of images image_hw, in units of the pixels of an h x w depth map (x by w / W, y by h / H)."""
    k = np.array(intri, F32, copy=True)
    H, Wd = (float(v) for v in image_hw)
    k[:, 0, 0] *= F32(w / Wd); k[:, 0, 2] *= F32(w / Wd)
    k[:, 1, 1] *= F32(h / H); k[:, 1, 2] *= F32(h / H)
    return k


def axes_focus(poses):
    """The point closest (least squares) to the optical axes of the cameras poses [V,3,4] (direction -R[:, 2] from o)."""
    P = np.asarray(poses, np.float64)
    A, b = np.zeros((3, 3)), np.zeros(3)
    for p in P:
        d = -p[:, 2] / np.linalg.norm(p[:, 2])
        M = np.eye(3) - np.outer(d, d)
        A += M
        b += M @ p[:, 3]
    return np.linalg.solve(A, b)


def synthetic_case(st, dims=(37, 21, 19), n_views=5, hw=(61, 45), seed=3, with_conf=True, pow2=False):
    """A grid of dims = (nx, ny, nz) points between the fox cameras and the point they look at, long enough to reach behind some of them
    and wide enough to leave every image; depth maps around the distance of the grid's centre with zeros, negatives, NaN and +inf
    sprinkled in, conf with zeros; a few pixels planted so that sdf == -trunc exactly and others so that sdf >= trunc.  pow2: step is
    rounded to a power of two and lo to a multiple of it before the maps are made -- the grid can then be translated by whole steps
    without a rounding (a window of a larger grid)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    h, w = hw
    cams = np.asarray(st["train_set"])[np.linspace(0, len(st["train_set"]) - 1, n_views).astype(int)]
    poses = np.ascontiguousarray(st["poses"][cams], F32)
    intri = scaled_intrinsics(st["intri"][cams], st["image_hw"], h, w)
    dist = np.ascontiguousarray(st["dist_params"][cams], F32)
    focus = axes_focus(st["poses"][np.asarray(st["train_set"])])
    eye = poses[:, :, 3].astype(np.float64).mean(0)
    # the box is centred between the cameras and their focus and reaches past both: voxels behind cameras, voxels outside the images
    centre = 0.5 * (focus + eye)
    extent = 1.6 * np.linalg.norm(focus - eye)
    step = F32(extent / (nx - 1))
    if pow2:
        step = F32(2.0 ** np.round(np.log2(float(step))))
    lo = (centre - 0.5 * float(step) * (np.array(dims) - 1)).astype(F32)
    if pow2:
        lo = (np.round(lo.astype(np.float64) / float(step)) * float(step)).astype(F32)
    trunc = F32(0.0625)
    r_mid = np.linalg.norm(poses[:, :, 3].astype(np.float64) - focus[None], axis=1)
    depth = (r_mid[:, None, None] * rng.uniform(0.6, 1.1, (n_views, h, w))).astype(F32)
    kind = rng.integers(0, 40, depth.shape)
    depth[kind == 0] = 0.0
    depth[kind == 1] = -rng.uniform(0.1, 2.0, int((kind == 1).sum())).astype(F32)
    depth[kind == 2] = np.nan
    depth[kind == 3] = np.inf
    conf = rng.uniform(0.05, 1.0, depth.shape).astype(F32)
    conf[rng.integers(0, 9, depth.shape) == 0] = 0.0
    # planted pixels: D = |q| - trunc (exact: trunc is a power of two far above the spacing of |q|) and D = |q| + 2 trunc
    for v in range(n_views):
        vis, ia, ib, r = project(lo, step, nx, ny, nz, poses[v], intri[v], dist[v], h, w)
        pick = np.flatnonzero(vis & (r > 4 * trunc))
        pick = pick[rng.permutation(len(pick))[:12]]
        for n, i in enumerate(pick):
            depth[v, ia[i], ib[i]] = F32(r[i] - trunc) if n % 2 == 0 else F32(r[i] + F32(2) * trunc)
            conf[v, ia[i], ib[i]] = F32(0.75)
    return dict(lo=lo, step=step, nx=nx, ny=ny, nz=nz, poses=poses, intri=intri, dist=dist, depth=depth, conf=conf if with_conf else None,
                trunc=trunc, h=h, w=w)


def sphere_depth_maps(poses, intri, dist, h, w, centre, radius, min_cos=0.5):
    """Analytic depth maps of a sphere: per pixel (a, b) the ray through the pixel's centre (b + 0.5, a + 0.5) -- undistorted by fixed
    point iteration, float64 -- meets the sphere at distance D along the unit ray; conf = 1 where it does at a cosine >= min_cos between
    the ray and the inward normal, else 0 (and D = 0 where it misses)."""
    V = len(poses)
    depth, conf = np.zeros((V, h, w), F32), np.zeros((V, h, w), F32)
    a, b = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    for v in range(V):
        P, K, k = np.asarray(poses[v], np.float64), np.asarray(intri[v], np.float64), np.asarray(dist[v], np.float64)
        xd, yd = (b + 0.5 - K[0, 2]) / K[0, 0], (a + 0.5 - K[1, 2]) / K[1, 1]
        u, vv = xd.copy(), yd.copy()
        for _ in range(50):
            r2 = u * u + vv * vv
            radial = k[0] * r2 + k[1] * r2 * r2
            du = u * radial + 2 * k[2] * u * vv + k[3] * (r2 + 2 * u * u)
            dv = vv * radial + 2 * k[3] * u * vv + k[2] * (r2 + 2 * vv * vv)
            u, vv = xd - du, yd - dv
        d_cam = np.stack([u, -vv, -np.ones_like(u)], -1)
        d = d_cam @ P[:, :3].T
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        oc = P[:, 3] - np.asarray(centre, np.float64)
        bq = (d * oc).sum(-1)
        disc = bq * bq - ((oc * oc).sum() - radius * radius)
        hit = disc > 0
        t = -bq - np.sqrt(np.where(hit, disc, 0))
        hit &= t > 0
        n = (oc[None, None] + t[..., None] * d) / radius
        cos = -(n * d).sum(-1)
        depth[v] = np.where(hit, t, 0).astype(F32)
        conf[v] = (hit & (cos >= min_cos)).astype(F32)
    return depth, conf
