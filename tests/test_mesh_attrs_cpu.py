"""Mesh attributes without a GPU: the normals, connected-components and component-filter kernels of csrc/octree.hip run under the
wavefront emulator (tests/wave_emul) against their numpy restatements (tests/mesh_attr_ref.py), and the PLY writer / launcher options
of f2_nerf_amd/mesh.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import mesh_attr_ref as ar  # noqa: E402
import mesh_ref as mr  # noqa: E402


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def emul_normals(L, g, pts, lo, step):
    g = np.ascontiguousarray(g, np.float32)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    nz, ny, nx = g.shape
    out = np.full((len(pts), 3), np.nan, np.float32)
    lo3 = (ctypes.c_float * 3)(*[float(v) for v in lo])
    assert L.f2n_grid_normals(None, len(pts), _vp(pts), _vp(g), nx, ny, nz, lo3, ctypes.c_float(step), _vp(out)) == 0
    return out


def emul_components(L, faces, n_verts):
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    labels = np.full(n_verts, -7, np.int32)
    changed = np.zeros(1, np.int32)
    rounds = ctypes.c_int(-1)
    assert L.f2n_mesh_components(None, n_verts, len(faces), _vp(faces), _vp(labels), _vp(changed), ctypes.byref(rounds)) == 0
    return labels, rounds.value


def emul_filter(L, verts, faces, min_faces):
    """f2n_mesh_components -> f2n_mesh_filter_count -> f2n_mesh_filter_emit, as MeshFilterComponents of csrc/host/RendererQuery.cpp."""
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nv, nf = len(verts), len(faces)
    labels, _ = emul_components(L, faces, nv)
    i32 = lambda *s: np.full(s, -7, np.int32)  # noqa: E731
    comp, vkeep, vse, fkeep, fse, totals = i32(nv), i32(nv), i32(nv, 2), i32(nf), i32(nf, 2), i32(2)
    assert L.f2n_mesh_filter_count(None, nv, nf, _vp(faces), _vp(labels), min_faces, _vp(comp), _vp(vkeep), _vp(vse), _vp(fkeep), _vp(fse),
                                   _vp(totals)) == 0
    kv, kf = int(totals[0]), int(totals[1])
    ov, src, of = np.full((kv, 3), np.nan, np.float32), i32(kv), i32(kf, 3)
    assert L.f2n_mesh_filter_emit(None, nv, nf, _vp(verts), _vp(faces), _vp(vkeep), _vp(vse), _vp(fkeep), _vp(fse), _vp(ov), _vp(src),
                                  _vp(of)) == 0
    return ov, of, src


def normal_cases():
    rng = np.random.default_rng(4)
    return [("sphere24", mr.sphere_grid(24, 8.3), 0.0, (0.0, 0.0, 0.0), 1.0),
            ("torus28", mr.torus_grid(28, 8.0, 3.4), 0.0, (-1.0, 0.5, 2.0), 0.25),
            ("random9x7x11", rng.standard_normal((9, 7, 11)).astype(np.float32), 0.1, (0.3, -0.2, 0.1), 0.125)]


def test_normals_on_the_emulator_match_the_restatement(emul):
    """The kernel's unit normals against the float64 restatement, as an error of the blend g(p) relative to max|G| (mesh_attr_ref.
    normal_error), at the vertices the marching-tetrahedra restatement gives.

    The bar is 8 x the float32-vs-float64 discrepancy of the RESTATEMENT ITSELF on the same grid and vertices (x 8: freedom in operation
    order and division rounding), computed here on the CPU.  Measured: discrepancy 1.24e-7 (sphere 24^3), 2.24e-7 (torus 28^3), 6.86e-7
    (random 9x7x11) -> bars 9.9e-7, 1.79e-6, 5.49e-6; the emulated kernel's error: 1.23e-7, 2.76e-7, 5.29e-7.  No vertex of the three grids
    falls under the exclusion |g_ref| < 1e-3 max|G| (at most 1 % may)."""
    for name, g, level, lo, step in normal_cases():
        v, _ = mr.marching_tets(g, level, lo, step)
        assert len(v) > 100
        disc = ar.blend_discrepancy(g, v, lo, step)
        bar = 8.0 * disc
        n = emul_normals(emul, g, v, lo, step)
        err, left_out = ar.normal_error(n, g, v, lo, step)
        print("%s: %d vertices, restatement f32-vs-f64 %.3g, bar %.3g, kernel error %.3g, left out %.4f" % (name, len(v), disc, bar, err, left_out))
        assert 0 < disc < 1e-5
        assert left_out <= 0.01
        assert err <= bar, (name, err, bar)
        ln = np.sqrt((n.astype(np.float64) ** 2).sum(1))
        assert (np.abs(ln - 1) < 1e-6).all()  # unit vectors (no gradient of these grids vanishes at a vertex)


def test_normals_point_outwards_in_xyz_order(emul):
    """On a sphere the normal is the radial direction: a sign and axis-order check, not a precision bar (the float64 restatement gives
    0.999994 on this 24^3 grid; the kernel must reach 0.9999)."""
    n_grid = 24
    g = mr.sphere_grid(n_grid, 8.3)
    v, _ = mr.marching_tets(g, 0.0)
    radial = v.astype(np.float64) - (n_grid - 1) / 2.0
    radial /= np.sqrt((radial ** 2).sum(1))[:, None]
    ref = ar.normals_of(ar.gradient_blend(g, v, dtype=np.float64)[0])
    assert (ref * radial).sum(1).min() >= 0.99999
    n = emul_normals(emul, g, v, (0.0, 0.0, 0.0), 1.0)
    dots = (n.astype(np.float64) * radial).sum(1)
    print("min dot(normal, radial) = %.7f" % dots.min())
    assert dots.min() >= 0.9999
    # an anisotropic field: the axes are not interchangeable
    nz, ny, nx = 10, 12, 14
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ramp = (1.0 * x + 10.0 * y + 100.0 * z).astype(np.float32)
    pts = np.array([[3.3, 4.4, 5.5], [0.0, 0.0, 0.0], [13.0, 11.0, 9.0], [-5.0, 40.0, 2.0]], np.float32)  # inside, corners, outside (clamped)
    n = emul_normals(emul, ramp, pts, (0.0, 0.0, 0.0), 1.0)
    want = -np.array([1.0, 10.0, 100.0]) / np.sqrt(10101.0)
    assert np.abs(n - want).max() < 1e-6
    # a flat grid and a NaN point: exactly zero
    assert (emul_normals(emul, np.ones((4, 5, 6), np.float32), pts, (0.0, 0.0, 0.0), 1.0) == 0).all()
    bad = emul_normals(emul, np.full((4, 5, 6), np.inf, np.float32), pts, (0.0, 0.0, 0.0), 1.0)
    assert (bad == 0).all()


def two_spheres():
    """Two well separated spheres of different size in one grid, and the large one alone."""
    shape = (20, 20, 34)
    big = ar.sphere_field(shape, (10.2, 9.6, 9.9), 6.3)
    small = ar.sphere_field(shape, (27.1, 10.3, 9.4), 2.7)
    return np.maximum(big, small), big


def random_blobs():
    rng = np.random.default_rng(11)
    return rng.standard_normal((10, 9, 11)).astype(np.float32), 0.8


def _check_mesh(L, v, f, thresholds):
    labels, rounds = emul_components(L, f, len(v))
    assert (labels == ar.components(f, len(v))).all()
    assert rounds >= (1 if len(f) else 0)
    for t in thresholds:
        ov, of, src = emul_filter(L, v, f, t)
        rv, rf, rsrc = ar.filter_components(v, f, t)
        assert ov.shape == rv.shape and (ov.view(np.uint32) == rv.view(np.uint32)).all(), t
        assert of.shape == rf.shape and (of == rf).all(), t
        assert (src == rsrc).all(), t
    return labels, rounds


def test_components_and_filter_two_spheres(emul):
    g, big = two_spheres()
    v, f = mr.marching_tets(g, 0.0)
    sizes = sorted(ar.component_face_counts(f, len(v)).values())
    assert len(sizes) == 2 and sizes[0] < sizes[1]
    labels, rounds = _check_mesh(emul, v, f, [2, sizes[0], sizes[0] + 1, sizes[1], sizes[1] + 1])
    print("two spheres: %d vertices, %d faces, components %s, %d labelling rounds" % (len(v), len(f), sizes, rounds))
    assert len(np.unique(labels)) == 2
    # a threshold between the two face counts leaves the large sphere: closed, genus 0, and the mesh of its own grid
    ov, of, src = emul_filter(emul, v, f, (sizes[0] + sizes[1]) // 2)
    assert mr.euler_characteristic(ov, of) == 2 and set(mr.edge_face_counts(of).values()) == {2}
    bv, bf = mr.marching_tets(big, 0.0)
    assert ov.shape == bv.shape and (ov.view(np.uint32) == bv.view(np.uint32)).all() and (of == bf).all()
    assert (v[src].view(np.uint32) == ov.view(np.uint32)).all()
    # everything is a floater above the larger count
    ov, of, src = emul_filter(emul, v, f, sizes[1] + 1)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and src.shape == (0,)


def test_components_and_filter_random_blobs(emul):
    g, level = random_blobs()
    v, f = mr.marching_tets(g, level)
    sizes = sorted(ar.component_face_counts(f, len(v)).values())
    assert len(sizes) >= 8 and sizes[0] < sizes[-1]  # many components of different sizes ...
    assert 1 in set(mr.edge_face_counts(f).values())  # ... some of them open (cut by the grid's faces)
    labels, rounds = _check_mesh(emul, v, f, sorted({2, 5, sizes[len(sizes) // 2], sizes[-1], sizes[-1] + 1}))
    print("random blobs: %d vertices, %d faces, %d components (%d..%d faces), %d labelling rounds"
          % (len(v), len(f), len(sizes), sizes[0], sizes[-1], rounds))
    # faces in a scrambled order and with rotated corners: the labels are the same (a unique fixpoint)
    rng = np.random.default_rng(5)
    f2 = np.roll(f[rng.permutation(len(f))], 1, axis=1)
    assert (emul_components(emul, f2, len(v))[0] == labels).all()


def test_components_and_filter_empty_and_unused(emul):
    # (c) an empty mesh
    labels, rounds = emul_components(emul, np.zeros((0, 3), np.int32), 0)
    assert labels.shape == (0,) and rounds == 0
    ov, of, src = emul_filter(emul, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 3)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and src.shape == (0,)
    # vertices without any face: every one its own component, none survives a filter
    pts = np.arange(15, dtype=np.float32).reshape(5, 3)
    labels, rounds = emul_components(emul, np.zeros((0, 3), np.int32), 5)
    assert (labels == np.arange(5)).all() and rounds == 0
    ov, of, src = emul_filter(emul, pts, np.zeros((0, 3), np.int32), 2)
    assert ov.shape == (0, 3) and of.shape == (0, 3)
    # (d) a vertex array with unused vertices between the used ones
    g, level = random_blobs()
    v, f = mr.marching_tets(g, level)
    rng = np.random.default_rng(6)
    spread = np.sort(rng.choice(len(v) + 40, len(v), replace=False)).astype(np.int32)  # new index of every old vertex
    v2 = rng.standard_normal((len(v) + 40, 3)).astype(np.float32)
    v2[spread] = v
    f2 = spread[f]
    labels, _ = _check_mesh(emul, v2, f2, [2, 7])
    unused = np.setdiff1d(np.arange(len(v2)), spread)
    assert (labels[unused] == unused).all()
    ov, of, src = emul_filter(emul, v2, f2, 2)  # every component has >= 2 faces here?  the restatement decides; unused vertices go
    assert not np.isin(src, unused).any()
    # a face that names a vertex outside the array connects nothing and is dropped
    tri = np.array([[0, 1, 2], [2, 3, 9], [3, 4, 5], [4, 5, 3]], np.int32)
    labels, _ = emul_components(emul, tri, 6)
    assert (labels == [0, 0, 0, 3, 3, 3]).all()
    ov, of, src = emul_filter(emul, np.arange(18, dtype=np.float32).reshape(6, 3), tri, 2)
    assert (src == [3, 4, 5]).all() and (of == [[0, 1, 2], [1, 2, 0]]).all()


# ---- the PLY writer and the launcher's options ---------------------------------------------------------------------------------------
def _ply_of_the_plain_writer(verts, faces):
    """The bytes mesh.write_ply(path, verts, faces) has written since mode=extract_mesh exists."""
    v = np.ascontiguousarray(verts, dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype="<i4").reshape(-1, 3)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
    rec = np.empty(len(f), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"] = 3
    rec["idx"] = f
    return header.encode("ascii") + v.tobytes() + rec.tobytes()


def read_ply_attrs(path):
    """Reader for the PLY files of mesh.write_ply with any of its vertex attributes: {"verts", "faces", "normals"?, "colors"?}."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0"
    iv = [i for i, h in enumerate(header) if h.startswith("element vertex")][0]
    jf = [i for i, h in enumerate(header) if h.startswith("element face")][0]
    nv, nf = int(header[iv].split()[-1]), int(header[jf].split()[-1])
    props = [h.split()[1:] for h in header[iv + 1:jf]]
    assert all(len(p) == 2 for p in props)
    names = [p[1] for p in props]
    assert names[:3] == ["x", "y", "z"]
    dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[kind]) for kind, name in props])
    assert header[jf + 1:] == ["property list uchar int vertex_indices", "end_header"]
    vrec = np.frombuffer(data, dt, nv, end)
    frec = np.frombuffer(data, [("n", "u1"), ("idx", "<i4", (3,))], nf, end + nv * dt.itemsize)
    assert (frec["n"] == 3).all() and len(data) == end + nv * dt.itemsize + nf * 13
    out = {"verts": np.stack([vrec[k] for k in "xyz"], 1).reshape(nv, 3), "faces": frec["idx"], "names": names}
    if "nx" in names:
        out["normals"] = np.stack([vrec[k] for k in ("nx", "ny", "nz")], 1).reshape(nv, 3)
    if "red" in names:
        out["colors"] = np.stack([vrec[k] for k in ("red", "green", "blue")], 1).reshape(nv, 3)
    return out


def test_ply_attributes(tmp_path):
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    rng = np.random.default_rng(0)
    v = rng.standard_normal((37, 3)).astype(np.float32)
    f = rng.integers(0, 37, (53, 3)).astype(np.int32)
    n = rng.standard_normal((37, 3)).astype(np.float32)
    c = rng.uniform(-0.2, 1.2, (37, 3)).astype(np.float32)
    c[:4] = [[0.0, 1.0, 0.5], [254.999 / 255, 1.5 / 255, 0.9999 / 255], [-1e-3, 1 + 1e-3, 0.25], [np.float32(128) / np.float32(255), 0.1, 0.7]]
    # without attributes: the bytes of the plain writer, whether the arguments are left out or passed as None
    for kw in ({}, {"normals": None, "colors": None}):
        p = mesh.write_ply(str(tmp_path / "plain.ply"), v, f, **kw)
        assert open(p, "rb").read() == _ply_of_the_plain_writer(v, f)
    p = mesh.write_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None, None)
    assert open(p, "rb").read() == _ply_of_the_plain_writer(np.zeros((0, 3)), np.zeros((0, 3)))
    quant = (np.clip(c, 0, 1) * np.float32(255)).astype(np.uint8)  # the project's image quantisation: truncation
    assert (quant[:3] == [[0, 255, 127], [254, 1, 0], [0, 255, 63]]).all()
    for normals, colors, names in ((n, c, ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]), (n, None, ["x", "y", "z", "nx", "ny", "nz"]),
                                   (None, c, ["x", "y", "z", "red", "green", "blue"])):
        m = read_ply_attrs(mesh.write_ply(str(tmp_path / "a" / "attrs.ply"), v, f, normals=normals, colors=colors))
        assert m["names"] == names
        assert (m["verts"].view(np.uint32) == v.view(np.uint32)).all() and (m["faces"] == f).all()
        assert ("normals" in m) == (normals is not None) and ("colors" in m) == (colors is not None)
        if normals is not None:
            assert (m["normals"].view(np.uint32) == n.view(np.uint32)).all()
        if colors is not None:
            assert m["colors"].dtype == np.uint8 and (m["colors"] == quant).all()
    m = read_ply_attrs(mesh.write_ply(str(tmp_path / "e.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32),
                                      np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)))
    assert m["verts"].shape == (0, 3) and m["normals"].shape == (0, 3) and m["colors"].shape == (0, 3)
    assert read_ply_attrs(str(tmp_path / "plain.ply"))["names"] == ["x", "y", "z"]


def test_attribute_options_parse_and_default():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    o = mesh.options(config.preset("wanjinyou", []))
    assert o["normals"] is False and o["colors"] is False and o["min_component_faces"] == 0
    assert o["resolution"] == 256 and o["level"] == mesh.DEFAULT_LEVEL
    o = mesh.options(config.preset("wanjinyou", ["mesh.normals=true", "mesh.colors=true", "mesh.min_component_faces=150", "mesh.level=5.5"]))
    assert o["normals"] is True and o["colors"] is True and o["min_component_faces"] == 150 and o["level"] == 5.5
    o = mesh.options(config.preset("wanjinyou", ["mesh.normals=false", "mesh.colors=true"]))
    assert o["normals"] is False and o["colors"] is True and o["min_component_faces"] == 0
    assert "mesh" not in config.GROUP_DEFAULTS
