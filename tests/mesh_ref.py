"""numpy restatement of the marching-tetrahedra iso-surface of include/f2n_abi.h (f2n_mesh_count / f2n_mesh_emit) and of the octree
point location (f2n_oct_locate_warp): the tests' reference, written from the definitions in the header, not from the kernels."""
import numpy as np

F32 = np.float32
# Kuhn split: tetrahedron t of a cell = corners (0, a, a|b, 7) for the axis order (a, b, c) of row t (x = 1, y = 2, z = 4)
TET_AXES = [(1, 2, 4), (1, 4, 2), (2, 1, 4), (2, 4, 1), (4, 1, 2), (4, 2, 1)]
EDGE_OFFSETS = [1, 2, 4, 3, 5, 6, 7]  # edge types +x, +y, +z, +xy, +xz, +yz, +xyz


def _off(o):
    return np.array([o & 1, (o >> 1) & 1, (o >> 2) & 1])


def _parity_even(axes):
    perm = [{1: 0, 2: 1, 4: 2}[a] for a in axes]
    inv = sum(1 for i in range(3) for j in range(i + 1, 3) if perm[i] > perm[j])
    return inv % 2 == 0


def _orient(p0, p1, p2, p3):
    return np.linalg.det(np.stack([p1 - p0, p2 - p0, p3 - p0]).astype(np.float64))


def grid_points(lo, step, n):
    """lo + step * i per axis, float32 with two roundings (no FMA)."""
    return [F32(lo[k]) + F32(step) * np.arange(n[k], dtype=F32) for k in range(3)]


def marching_tets(g, level, lo=(0.0, 0.0, 0.0), step=1.0):
    """g [nz, ny, nx] float32 -> (verts [V,3] f32, faces [F,3] int32) by the rules of include/f2n_abi.h.  Windings are derived from
    geometry here (the normal of each triangle must point from the tet's inside corners to its outside ones), independently of the
    kernel's case table."""
    g = np.asarray(g, F32)
    nz, ny, nx = g.shape
    level = F32(level)
    inside = g > level
    cx, cy, cz = grid_points(lo, step, (nx, ny, nz))
    # vertices: owner corner (x-fastest index) then edge type
    vid = {}
    verts = []
    flat_in = inside.reshape(-1)
    flat_g = g.reshape(-1)
    idx = np.arange(nx * ny * nz)
    xs, ys, zs = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    cand = []
    for t, o in enumerate(EDGE_OFFSETS):
        d = _off(o)
        ok = (xs + d[0] < nx) & (ys + d[1] < ny) & (zs + d[2] < nz)
        b = np.where(ok, idx + d[0] + d[1] * nx + d[2] * nx * ny, 0)
        cross = ok & (flat_in != flat_in[b])
        for c in idx[cross]:
            cand.append((int(c), t, int(b[c])))
    cand.sort()
    for c, t, b in cand:
        ga, gb = flat_g[c], flat_g[b]
        s = F32((level - ga) / (gb - ga))
        pa = np.array([cx[c % nx], cy[(c // nx) % ny], cz[c // (nx * ny)]], F32)
        pb = np.array([cx[b % nx], cy[(b // nx) % ny], cz[b // (nx * ny)]], F32)
        vid[(c, t)] = len(verts)
        verts.append((pa + s * (pb - pa)).astype(F32))
    faces = []
    for z in range(nz - 1):
        for y in range(ny - 1):
            for x in range(nx - 1):
                cm = [bool(inside[z + ((o >> 2) & 1), y + ((o >> 1) & 1), x + (o & 1)]) for o in range(8)]
                if all(cm) or not any(cm):
                    continue
                for axes in TET_AXES:
                    tv = [0, axes[0], axes[0] | axes[1], 7]
                    ins = [cm[o] for o in tv]
                    k = sum(ins)
                    if k == 0 or k == 4:
                        continue

                    def vert_of(oa, ob):
                        lo_o = oa if (oa & ob) == oa else ob
                        t = EDGE_OFFSETS.index(oa ^ ob)
                        c = (z + ((lo_o >> 2) & 1)) * nx * ny + (y + ((lo_o >> 1) & 1)) * nx + (x + (lo_o & 1))
                        return vid[(c, t)]

                    I = [tv[i] for i in range(4) if ins[i]]
                    O = [tv[i] for i in range(4) if not ins[i]]
                    if k == 1 or k == 3:
                        lone = I[0] if k == 1 else O[0]
                        others = [o for o in tv if o != lone]
                        tris = [[vert_of(lone, o) for o in others]]
                    else:
                        i, j = I
                        kk, ll = O
                        tris = [[vert_of(i, kk), vert_of(i, ll), vert_of(j, ll)], [vert_of(i, kk), vert_of(j, ll), vert_of(j, kk)]]
                    # wind by geometry on the unit cube: normal from the inside corners' centroid to the outside ones'
                    cin = np.mean([_off(o) for o in I], 0)
                    cout = np.mean([_off(o) for o in O], 0)
                    faces.extend(tris)
                    _fix_winding(faces, len(tris), I, O, cin, cout, vert_of)
    return (np.array(verts, F32).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3))


def _fix_winding(faces, n_new, I, O, cin, cout, vert_of):
    """Orient the last n_new triangles: each lies on edges of the tet between inside and outside corners; with the edge midpoints as
    positions, the normal must have a positive component along cout - cin."""
    inv = {}
    for a in I:
        for b in O:
            inv[vert_of(a, b)] = (_off(a) + _off(b)) / 2.0
    for q in range(len(faces) - n_new, len(faces)):
        a, b, c = faces[q]
        n = np.cross(inv[b] - inv[a], inv[c] - inv[a])
        if np.dot(n, cout - cin) < 0:
            faces[q] = [a, c, b]


def euler_characteristic(verts, faces):
    e = set()
    for f in faces:
        for i in range(3):
            a, b = int(f[i]), int(f[(i + 1) % 3])
            e.add((min(a, b), max(a, b)))
    used = len(np.unique(np.asarray(faces).reshape(-1))) if len(faces) else 0
    return used - len(e) + len(faces)


def edge_face_counts(faces):
    cnt = {}
    for f in faces:
        for i in range(3):
            a, b = int(f[i]), int(f[(i + 1) % 3])
            k = (min(a, b), max(a, b))
            cnt[k] = cnt.get(k, 0) + 1
    return cnt


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def sphere_grid(n, r):
    c = (n - 1) / 2.0
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    return (r - np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)).astype(F32)  # > 0 inside


def torus_grid(n, R, r):
    c = (n - 1) / 2.0
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    q = np.sqrt((x - c) ** 2 + (y - c) ** 2) - R
    return (r - np.sqrt(q ** 2 + (z - c) ** 2)).astype(F32)


# ---- octree point location (f2n_oct_locate_warp), restated on the TreeNode bytes -------------------------------------------------
def parse_nodes(tree_nodes_bytes):
    b = np.frombuffer(np.asarray(tree_nodes_bytes, np.uint8).tobytes(), np.uint8).reshape(-1, 64)
    f = b.view(np.float32)
    i = b.view(np.int32)
    return {"center": f[:, 0:3].copy(), "side": f[:, 3].copy(), "childs": i[:, 5:13].copy(), "trans": i[:, 14].copy()}


def locate(nodes, p):
    """(trans_idx, leaf) of world point p (float32 [3]), (-1, -1) when empty."""
    p = np.asarray(p, F32)
    h = F32(nodes["side"][0] * F32(0.5))
    c0 = nodes["center"][0]
    if not all((p[k] >= F32(c0[k] - h)) and (p[k] <= F32(c0[k] + h)) for k in range(3)):
        return -1, -1
    u = 0
    for _ in range(32):
        ch = nodes["childs"][u]
        if (ch < 0).all():
            t = int(nodes["trans"][u])
            return (t, u) if t >= 0 else (-1, -1)
        c = nodes["center"][u]
        st = 4 * int(p[0] >= c[0]) + 2 * int(p[1] >= c[1]) + int(p[2] >= c[2])
        if ch[st] < 0:
            return -1, -1
        u = int(ch[st])
    return -1, -1
