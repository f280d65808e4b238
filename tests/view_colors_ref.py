"""float32 numpy restatement of the view-colour entry points of include/f2n_abi.h (f2n_view_colors_accumulate, f2n_view_colors_finalize):
the tests' reference, written from the definitions in the header, not from the kernels.  Every operation is one float32 rounding in
the header's order (numpy never contracts a product and a sum), so the device must give its bits.  Also the cases the CPU and the
device tests share."""
import numpy as np

import tsdf_ref as tr

F32 = np.float32
TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))
EXITS = ("behind", "facing", "no_tap", "tap_outside", "no_depth", "depth_low", "depth_high", "conf0", "zero_weight", "used_1", "used_2",
         "used_3", "used_4", "at_minus_tol", "at_plus_tol")


def has_normal(normals, n):
    """[n] bool: the row is a normal (not all zero, every component finite); None: no row is."""
    if normals is None:
        return np.zeros(n, bool)
    nr = np.asarray(normals, F32).reshape(-1, 3)
    return np.isfinite(nr).all(1) & (nr != 0).any(1)


def project(points, pose, K, k):
    """Steps 1-6 of f2n_tsdf_integrate for points [n,3] and one view: (front, q [3][n], x, y, r)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    P, K = np.asarray(pose, F32), np.asarray(K, F32)
    with np.errstate(all="ignore"):
        q = [p[:, j] - P[j, 3] for j in range(3)]
        c = [P[0, j] * q[0] + (P[1, j] * q[1] + P[2, j] * q[2]) for j in range(3)]
        s = -c[2]
        u, vv = c[0] / s, (-c[1]) / s
        du, dv = tr.distort(k, u, vv)
        x = K[0, 0] * (u + du) + K[0, 2]
        y = K[1, 1] * (vv + dv) + K[1, 2]
        r = np.sqrt(q[0] * q[0] + (q[1] * q[1] + q[2] * q[2]))
    return s > 0, q, x, y, r


def accumulate(acc, wsum, count, points, normals, poses, intri, dist, depth, conf, image, tol, cos_min, stats=None):
    """(acc [n,C], wsum [n], count [n] int32) after the views were added in index order; the inputs are not modified.  stats (a dict,
    optional) receives how many (point, view) pairs -- for the tap exits: (point, view, tap) triples -- took each exit (EXITS)."""
    acc = np.array(acc, F32, copy=True)
    wsum = np.array(wsum, F32, copy=True).reshape(-1)
    count = np.array(count, np.int32, copy=True).reshape(-1)
    p = np.asarray(points, F32).reshape(-1, 3)
    n, C = acc.shape
    has = has_normal(normals, n)
    nr = np.asarray(normals, F32).reshape(-1, 3) if normals is not None else np.zeros((n, 3), F32)
    poses, intri, dist = np.asarray(poses, F32).reshape(-1, 3, 4), np.asarray(intri, F32).reshape(-1, 3, 3), np.asarray(dist, F32).reshape(-1, 4)
    depth, image = np.asarray(depth, F32), np.asarray(image, F32)
    V, h, w = depth.shape
    assert image.shape == (V, h, w, C)
    tol, cos_min, half, one = F32(tol), F32(cos_min), F32(0.5), F32(1)
    st = dict.fromkeys(EXITS, 0)
    with np.errstate(all="ignore"):
        for v in range(V):
            front, q, x, y, r = project(p, poses[v], intri[v], dist[v])
            cosv = (nr[:, 0] * (-q[0]) + (nr[:, 1] * (-q[1]) + nr[:, 2] * (-q[2]))) / r
            faces = ~has | (cosv > cos_min)
            facing = np.where(has, cosv, one).astype(F32)
            live = front & faces
            xs, ys = x - half, y - half
            b0, a0 = np.floor(xs), np.floor(ys)
            fx, fy = xs - b0, ys - a0
            om, col, nvalid, nexist = np.zeros(n, F32), np.zeros((n, C), F32), np.zeros(n, np.int64), np.zeros(n, np.int64)
            tap_stats = []
            for i, j in TAPS:
                ta, tb = a0 + F32(i), b0 + F32(j)
                ex = live & (ta >= 0) & (ta < F32(h)) & (tb >= 0) & (tb < F32(w))
                ia, ib = np.where(ex, ta, 0).astype(np.int64), np.where(ex, tb, 0).astype(np.int64)
                D = depth[v, ia, ib]
                cf = np.asarray(conf, F32)[v, ia, ib] if conf is not None else np.ones(n, F32)
                d = D - r
                has_d = ex & (D > 0)
                has_c = has_d & (cf > 0)
                valid = has_c & ~(d < -tol) & ~(d > tol)
                ok = ((fy if i else one - fy) * (fx if j else one - fx)) * cf
                om = np.where(valid, om + ok, om).astype(F32)
                for c in range(C):
                    col[:, c] = np.where(valid, col[:, c] + ok * image[v, ia, ib, c], col[:, c])
                nvalid += valid
                nexist += ex
                tap_stats.append((ex, has_d, has_c, d, valid))
            use = live & (om > 0)
            for c in range(C):
                acc[:, c] = np.where(use, acc[:, c] + facing * col[:, c], acc[:, c])
            wsum = np.where(use, wsum + facing * om, wsum).astype(F32)
            count = (count + use).astype(np.int32)
            some = live & (nexist > 0)
            st["behind"] += int((~front).sum()); st["facing"] += int((front & ~faces).sum()); st["no_tap"] += int((live & (nexist == 0)).sum())
            for ex, has_d, has_c, d, valid in tap_stats:
                st["tap_outside"] += int((some & ~ex).sum()); st["no_depth"] += int((ex & ~has_d).sum()); st["conf0"] += int((has_d & ~has_c).sum())
                st["depth_low"] += int((has_c & (d < -tol)).sum()); st["depth_high"] += int((has_c & (d > tol)).sum())
                st["at_minus_tol"] += int((valid & (d == -tol)).sum()); st["at_plus_tol"] += int((valid & (d == tol)).sum())
            st["zero_weight"] += int((live & (nvalid > 0) & ~use).sum())
            for m in range(1, 5):
                st["used_%d" % m] += int((use & (nvalid == m)).sum())
    if stats is not None:
        stats.update(st)
    return acc, wsum, count


def finalize(acc, wsum, count, min_views):
    acc, wsum, count = np.asarray(acc, F32), np.asarray(wsum, F32).reshape(-1), np.asarray(count, np.int32).reshape(-1)
    with np.errstate(all="ignore"):
        known = (count >= int(min_views)) & (wsum > 0)
        rgb = np.where(known[:, None], acc / wsum[:, None], F32(0)).astype(F32)
    return rgb, known.astype(np.uint8)


def fuse(points, normals, case, C=3, tol=None, cos_min=None, min_views=1, views=None):
    """zero sums -> accumulate over the case's views (or the listed ones) -> finalize: (rgb, known, wsum, count)"""
    n = len(points)
    sel = slice(None) if views is None else list(views)
    conf = None if case.get("conf") is None else case["conf"][sel]
    a, ws, cn = accumulate(np.zeros((n, C), F32), np.zeros(n, F32), np.zeros(n, np.int32), points, normals, case["poses"][sel], case["intri"][sel],
                           case["dist"][sel], case["depth"][sel], conf, case["image"][sel], case["tol"] if tol is None else tol,
                           case["cos_min"] if cos_min is None else cos_min)
    return finalize(a, ws, cn, min_views) + (ws, cn)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def grid_case(st, seed=11):
    """The bit-for-bit case: the views of tr.synthetic_case(dims=(37,21,19), n_views=5, hw=(61,45)) -- depth with zeros, negatives, NaN and
    +inf, conf with zeros -- its 14 763 grid points as the points (no multiple of 256), random unit normals with zero rows and NaN
    rows, tol = 0.0625 and cos_min = 0.1.  Planted per view, around picked points that face the view (tap (0,0) at (a0, b0)): D = r + tol
    and D = r - tol exactly (checked: the sum is exact and the difference gives tol back), all four taps at D = r, and three taps at D = r
    with the fourth 2 tol in front.  Images are drawn by image_for(case, C)."""
    c = tr.synthetic_case(st, dims=(37, 21, 19), n_views=5, hw=(61, 45))
    rng = np.random.default_rng(seed)
    px, py, pz = tr.voxel_points(c["lo"], c["step"], c["nx"], c["ny"], c["nz"])
    points = np.ascontiguousarray(np.stack([px, py, pz], 1), F32)
    n = len(points)
    normals = rng.standard_normal((n, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F32)
    kind = rng.integers(0, 12, n)
    normals[kind == 0] = 0.0
    normals[kind == 1, rng.integers(0, 3, int((kind == 1).sum()))] = np.nan
    normals[kind == 2, 0] = np.inf
    tol, cos_min = F32(0.0625), F32(0.1)
    depth, conf = c["depth"].copy(), c["conf"].copy()
    has = has_normal(normals, n)
    h, w = c["h"], c["w"]
    for v in range(len(depth)):
        front, q, x, y, r = project(points, c["poses"][v], c["intri"][v], c["dist"][v])
        with np.errstate(all="ignore"):
            cosv = (normals[:, 0] * (-q[0]) + (normals[:, 1] * (-q[1]) + normals[:, 2] * (-q[2]))) / r
            a0, b0 = np.floor(y - F32(0.5)), np.floor(x - F32(0.5))
            exact = (F32(r + tol) - r == tol) & (F32(r - tol) - r == -tol)
        ok = front & (~has | (cosv > cos_min)) & (a0 >= 0) & (a0 < h - 1) & (b0 >= 0) & (b0 < w - 1) & (r > 4 * tol) & exact
        pick = np.flatnonzero(ok)
        pick = pick[rng.permutation(len(pick))[:24]]
        taken = np.zeros((h, w), bool)
        m = 0
        for i in pick:
            a, b = int(a0[i]), int(b0[i])
            if taken[a:a + 2, b:b + 2].any():
                continue
            taken[a:a + 2, b:b + 2] = True
            conf[v, a:a + 2, b:b + 2] = F32(0.75)
            if m % 4 == 0:
                depth[v, a, b] = F32(r[i] + tol)
            elif m % 4 == 1:
                depth[v, a, b] = F32(r[i] - tol)
            else:
                depth[v, a:a + 2, b:b + 2] = r[i]
                if m % 4 == 3:
                    depth[v, a + 1, b + 1] = F32(r[i] - F32(2) * tol)
            m += 1
    return dict(points=points, normals=normals, poses=c["poses"], intri=c["intri"], dist=c["dist"], depth=depth, conf=conf, h=h, w=w, tol=tol,
                cos_min=cos_min)


def image_for(case, C, seed=5):
    """a random image [V,h,w,C] in [0, 1) with a few negative and large entries (the kernel does not clip)"""
    rng = np.random.default_rng(seed + C)
    im = rng.uniform(0, 1, case["depth"].shape + (C,)).astype(F32)
    im[rng.integers(0, 50, im.shape) == 0] = F32(-0.25)
    im[rng.integers(0, 50, im.shape) == 0] = F32(3.5)
    return im


def big_case(st, n=200003, seed=17):
    """n random points in the grid case's box against 9 views of 120 x 67 built the same way, C = 3: a grid-stride or 64-bit indexing
    mistake shows at this size and not at 14 763."""
    c = tr.synthetic_case(st, dims=(37, 21, 19), n_views=9, hw=(120, 67), seed=7)
    rng = np.random.default_rng(seed)
    lo = np.asarray(c["lo"], np.float64)
    hi = lo + float(c["step"]) * (np.array([c["nx"], c["ny"], c["nz"]]) - 1)
    points = rng.uniform(lo, hi, (n, 3)).astype(F32)
    normals = rng.standard_normal((n, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F32)
    normals[rng.integers(0, 10, n) == 0] = 0.0
    case = dict(points=points, normals=normals, poses=c["poses"], intri=c["intri"], dist=c["dist"], depth=c["depth"], conf=c["conf"], h=c["h"],
                w=c["w"], tol=F32(0.0625), cos_min=F32(0.1))
    case["image"] = image_for(case, 3)
    return case


def pixel_rays(pose, K, k, h, w):
    """Unit world directions [h,w,3] (float64) of the rays through the pixel centres (b + 0.5, a + 0.5), undistorted by the fixed-point
    iteration of tr.sphere_depth_maps."""
    P, K, k = np.asarray(pose, np.float64), np.asarray(K, np.float64), np.asarray(k, np.float64)
    a, b = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    xd, yd = (b + 0.5 - K[0, 2]) / K[0, 0], (a + 0.5 - K[1, 2]) / K[1, 1]
    u, vv = xd.copy(), yd.copy()
    for _ in range(50):
        r2 = u * u + vv * vv
        radial = k[0] * r2 + k[1] * r2 * r2
        du = u * radial + 2 * k[2] * u * vv + k[3] * (r2 + 2 * u * u)
        dv = vv * radial + 2 * k[3] * u * vv + k[2] * (r2 + 2 * vv * vv)
        u, vv = xd - du, yd - dv
    d = np.stack([u, -vv, -np.ones_like(u)], -1) @ P[:, :3].T
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


SPHERE_R = 0.15
SPHERE_COS_MIN = 0.5


def sphere_rig(st, intrinsics, n_points=4000, n_views=6, s=2):
    """The known-answer rig: n_views fox training cameras (evenly picked), maps at 1/s of the resolution with intrinsics(intri, s)
    (mesh.view_intrinsics), tr.sphere_depth_maps of a sphere of radius SPHERE_R around the cameras' focus (conf 1 wherever a ray meets
    it), an image that paints every pixel 0.5 + 0.5 n of its hit point (float64, analytic; 0 where the ray misses), and n_points points
    of a Fibonacci spiral on the sphere with their normals.  tol = rho / cos_min with rho = sqrt(2) (r_max + R) / f_min, the lateral
    reach of a tap (see bound()); cos_min = SPHERE_COS_MIN.  Also per (view, point), analytic in float64: cos (the facing cosine), xy (the
    projection in map pixels, by the forward model)."""
    ts = np.asarray(st["train_set"])
    cams = ts[np.linspace(0, len(ts) - 1, n_views).astype(int)]
    centre = tr.axes_focus(st["poses"][ts])
    H, Wd = (int(v) for v in st["image_hw"])
    h, w = H // s, Wd // s
    poses = np.ascontiguousarray(st["poses"][cams], F32)
    intri = np.ascontiguousarray(intrinsics(st["intri"][cams], s), F32)
    dist = np.ascontiguousarray(st["dist_params"][cams], F32)
    depth, conf = tr.sphere_depth_maps(poses, intri, dist, h, w, centre, SPHERE_R, -2.0)
    image = np.zeros((n_views, h, w, 3), F32)
    for v in range(n_views):
        d = pixel_rays(poses[v], intri[v], dist[v], h, w)
        hit = poses[v][:, 3].astype(np.float64)[None, None] + depth[v].astype(np.float64)[..., None] * d
        nrm = (hit - centre[None, None]) / SPHERE_R
        image[v] = np.where((depth[v] > 0)[..., None], 0.5 + 0.5 * nrm, 0.0).astype(F32)
    k = np.arange(n_points) + 0.5
    z = 1.0 - 2.0 * k / n_points
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    nrm = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    pts = centre[None] + SPHERE_R * nrm
    cos, xy = np.zeros((n_views, n_points)), np.zeros((n_views, n_points, 2))
    r_max = 0.0
    for v in range(n_views):
        P, K, kd = poses[v].astype(np.float64), intri[v].astype(np.float64), dist[v].astype(np.float64)
        q = pts - P[:, 3][None]
        r = np.linalg.norm(q, axis=1)
        r_max = max(r_max, float(r.max()))
        cos[v] = -(nrm * q).sum(1) / r
        c = q @ P[:, :3]
        u, vv = c[:, 0] / -c[:, 2], -c[:, 1] / -c[:, 2]
        r2 = u * u + vv * vv
        radial = kd[0] * r2 + kd[1] * r2 * r2
        du = u * radial + 2 * kd[2] * u * vv + kd[3] * (r2 + 2 * u * u)
        dv = vv * radial + 2 * kd[3] * u * vv + kd[2] * (r2 + 2 * vv * vv)
        xy[v, :, 0], xy[v, :, 1] = K[0, 0] * (u + du) + K[0, 2], K[1, 1] * (vv + dv) + K[1, 2]
        assert (c[:, 2] < 0).all()  # the whole sphere lies in front of every camera
    f_min = float(min(intri[:, 0, 0].min(), intri[:, 1, 1].min()))
    rho = np.sqrt(2.0) * (r_max + SPHERE_R) / f_min
    return dict(points=pts.astype(F32), normals=nrm.astype(F32), truth=0.5 + 0.5 * nrm, poses=poses, intri=intri, dist=dist, depth=depth,
                conf=conf, image=image, h=h, w=w, centre=centre, cos=cos, xy=xy, rho=rho, tol=F32(rho / SPHERE_COS_MIN), cos_min=F32(SPHERE_COS_MIN))


def sphere_bound(rig):
    """The colour bound of the sphere rig.  A fused colour is a convex combination (weights >= 0) of the image at its valid taps, so
    its error is at most the largest |image_k - truth(p)| over them.  A tap's pixel centre lies within one pixel of the point's
    projection along each axis: an angle of at most sqrt(2) / f between the tap's ray and the point's, so its hit point h_k (at most
    r_max + R from the camera) is at most rho = sqrt(2) (r_max + R) / f_min to the side of p; along the ray a valid tap is within tol
    of p by definition, and tol = rho / cos_min -- the pixel footprint at the grazing limit: across a footprint seen at the cosine
    cos_min the range changes by rho tan(theta) < rho / cos_min, so the taps of a point the view faces by the margin stay valid.
    Hence |h_k - p| <= sqrt(rho^2 + tol^2), and the colour 0.5 + 0.5 (h - centre) / R changes by 0.5 / R per unit length in every
    component: bound = 0.5 / R * rho * sqrt(1 + 1 / cos_min^2), plus 1e-5 for the float32 roundings of maps, image and sums."""
    return 0.5 / SPHERE_R * rig["rho"] * np.sqrt(1.0 + 1.0 / SPHERE_COS_MIN ** 2) + 1e-5


def sphere_classes(rig):
    """(seen [n], unseen [n]) bool: some view faces the point at a cosine >= cos_min + 0.1 with its projection >= 2 pixels inside the
    image; every view faces it at a cosine <= cos_min - 0.1 or has its projection >= 2 pixels outside.  The rest is not asserted."""
    x, y = rig["xy"][..., 0], rig["xy"][..., 1]
    inside = (x >= 2) & (x <= rig["w"] - 2) & (y >= 2) & (y <= rig["h"] - 2)
    outside = (x <= -2) | (x >= rig["w"] + 2) | (y <= -2) | (y >= rig["h"] + 2)
    seen = ((rig["cos"] >= SPHERE_COS_MIN + 0.1) & inside).any(0)
    unseen = ((rig["cos"] <= SPHERE_COS_MIN - 0.1) | outside).all(0)
    return seen, unseen


def check_sphere(rig, fuse_fn):
    """The known answer for fuse_fn(points, normals, rig) -> (rgb, known, ...): returns (largest colour error over the seen points,
    share of points not asserted)."""
    rgb, known = fuse_fn(rig["points"], rig["normals"], rig)[:2]
    rgb, known = np.asarray(rgb), np.asarray(known) != 0
    seen, unseen = sphere_classes(rig)
    other = 1.0 - (seen | unseen).mean()
    err = np.abs(rgb[seen].astype(np.float64) - rig["truth"][seen]).max()
    print("sphere: %d seen, %d unseen, %.1f %% not asserted, %d known; colour error max %.4g (bound %.4g)" % (
        seen.sum(), unseen.sum(), 100 * other, known.sum(), err, sphere_bound(rig)))
    assert seen.sum() > 500 and unseen.sum() > 500 and other <= 0.15, (seen.sum(), unseen.sum(), other)
    assert known[seen].all(), int((~known[seen]).sum())
    assert not known[unseen].any(), int(known[unseen].sum())
    assert (rgb[~known] == 0).all()
    assert err <= sphere_bound(rig), (err, sphere_bound(rig))
    return err, other


def occlusion_case(rig):
    """Views 0 and 1 of the sphere rig, view 0's image pure (1, 0, 0) and view 1's pure (0, 1, 0), and a disc of 8 pixels radius in FRONT
    of the sphere in view 0's depth map only (0.2 closer, around the sphere's centre pixel).  Returns (case, hidden [n] bool): the points
    whose projection in view 0 lies >= 2 pixels inside the disc (all four taps on it) and that view 1 sees by the margin of
    sphere_classes."""
    c = {k: (rig[k][:2].copy() if k in ("poses", "intri", "dist", "depth", "conf", "image") else rig[k]) for k in rig}
    h, w = rig["h"], rig["w"]
    a, b = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    mid = rig["xy"][0][np.argmax(rig["cos"][0])]  # the projection of the point that faces view 0 most: the sphere's centre pixel
    disc = (b - mid[0]) ** 2 + (a - mid[1]) ** 2 <= 8.0 ** 2
    assert (c["depth"][0][disc] > 0.3).all()
    c["depth"][0][disc] -= F32(0.2)
    c["image"][0] = np.array([1, 0, 0], F32)
    c["image"][1] = np.array([0, 1, 0], F32)
    x0, y0 = rig["xy"][0][:, 0], rig["xy"][0][:, 1]
    x1, y1 = rig["xy"][1][:, 0], rig["xy"][1][:, 1]
    behind_disc = (rig["cos"][0] > 0) & ((x0 - mid[0]) ** 2 + (y0 - mid[1]) ** 2 <= 6.0 ** 2)
    seen1 = (rig["cos"][1] >= SPHERE_COS_MIN + 0.1) & (x1 >= 2) & (x1 <= w - 2) & (y1 >= 2) & (y1 <= h - 2)
    return c, behind_disc & seen1


def check_occlusion(rig, fuse_fn):
    c, hidden = occlusion_case(rig)
    rgb, known, _, count = fuse_fn(rig["points"], rig["normals"], c)
    rgb, known, count = np.asarray(rgb), np.asarray(known) != 0, np.asarray(count)
    assert hidden.sum() >= 10, hidden.sum()
    assert known[hidden].all() and (count[hidden] == 1).all()
    assert np.abs(rgb[hidden] - np.array([0, 1, 0], F32)[None]).max() <= 1e-6
    seen0 = known & (rgb[:, 0] > 0.5)  # the case is not trivial: elsewhere view 0 is seen, and blends with view 1
    assert seen0.sum() > 100 and (count[seen0] >= 1).all() and (count == 2).any()
