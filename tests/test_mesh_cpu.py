"""Mesh export without a GPU: the PLY writer of f2_nerf_amd/mesh.py and the numpy restatement of the marching-tetrahedra rules of
include/f2n_abi.h (tests/mesh_ref.py), which the GPU tests hold the kernels to."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_ref as mr  # noqa: E402


def read_ply(path):
    """A small reader for the binary little-endian PLY files mesh.write_ply produces."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0"
    nv = int([h for h in header if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in header if h.startswith("element face")][0].split()[-1])
    assert "property list uchar int vertex_indices" in header
    v = np.frombuffer(data, "<f4", nv * 3, end).reshape(nv, 3)
    rec = np.frombuffer(data, [("n", "u1"), ("idx", "<i4", (3,))], nf, end + nv * 12)
    assert (rec["n"] == 3).all() and len(data) == end + nv * 12 + nf * 13
    return v, rec["idx"]


def test_ply_round_trip(tmp_path):
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    rng = np.random.default_rng(0)
    v = rng.standard_normal((37, 3)).astype(np.float32)
    f = rng.integers(0, 37, (53, 3)).astype(np.int32)
    p = mesh.write_ply(str(tmp_path / "m" / "a.ply"), v, f)
    v2, f2 = read_ply(p)
    assert (v2.view(np.uint32) == v.view(np.uint32)).all() and (f2 == f).all()
    v3, f3 = read_ply(mesh.write_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)))
    assert v3.shape == (0, 3) and f3.shape == (0, 3)


def test_world_frame_and_options():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config, mesh
    v = mesh.to_world(np.array([[0.0, 0.0, 0.0], [1.0, -1.0, 0.5]], np.float32), np.array([1.0, 2.0, 3.0], np.float32), 2.0)
    assert np.allclose(v, [[1, 2, 3], [3, 0, 4]])
    cfg = config.preset("wanjinyou", ["mesh.resolution=97", "mesh.level=5.5"])
    o = mesh.options(cfg)
    assert o["resolution"] == 97 and o["level"] == 5.5
    assert o["bbox_min"] == [-1.0, -1.0, -1.0] and o["bbox_max"] == [1.0, 1.0, 1.0]  # the pts_sampler box, not the 512-wide root
    assert mesh.options(config.preset("wanjinyou", []))["resolution"] == 256
    assert "mesh" not in config.GROUP_DEFAULTS


def _closed_checks(v, f, chi):
    assert len(f) > 0
    cnt = mr.edge_face_counts(f)
    assert set(cnt.values()) == {2}  # closed: every undirected edge in exactly two faces
    assert mr.euler_characteristic(v, f) == chi
    assert len(np.unique(f)) == len(v)  # every vertex is used


def test_restatement_sphere_is_closed_genus_0_and_outward():
    r = 5.3
    v, f = mr.marching_tets(mr.sphere_grid(16, r), 0.0)
    _closed_checks(v, f, 2)
    vol = mr.signed_volume(v, f)
    assert vol > 0 and abs(vol - 4.0 / 3.0 * np.pi * r ** 3) < 0.05 * 4.0 / 3.0 * np.pi * r ** 3


def test_restatement_torus_has_euler_characteristic_0():
    v, f = mr.marching_tets(mr.torus_grid(20, 5.0, 2.2), 0.0)
    _closed_checks(v, f, 0)
    assert mr.signed_volume(v, f) > 0


def test_restatement_open_and_empty_cases():
    v, f = mr.marching_tets(np.full((5, 6, 7), -1.0, np.float32), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    g = mr.sphere_grid(12, 7.0)  # the sphere is cut by the grid's faces: an open surface
    v, f = mr.marching_tets(g, 0.0)
    assert len(f) > 0 and 1 in set(mr.edge_face_counts(f).values())
