"""Mesh export of a trained scene: `python -m f2_nerf_amd.run ... mode=extract_mesh is_continue=true`.

The density grid and the iso-surface are computed on the device (ExpRunner.extract_mesh: f2n_oct_locate_warp_grid -> field
forward -> f2n_mesh_count / f2n_mesh_emit); this module only picks the options, maps the vertices back to the data set's world
frame and writes the PLY file.

Options (hydra-style overrides, no `mesh` group in the configs):
  mesh.resolution  cells along the longest side of the box (default 256)
  mesh.level       density iso-level (default DEFAULT_LEVEL)
  mesh.bbox_min / mesh.bbox_max  the box in the NORMALISED scene frame (default: pts_sampler.bbox_min / bbox_max, [-1, 1]^3,
                   which holds the normalised cameras; the octree's root cube is 512 wide and mostly empty)
"""
import os

import numpy as np

# The density iso-level of the default export.  A march step of sample_l = 1/256 (warped units) at fineness 1 is half opaque where
# 1 - exp(-sigma / 256) = 1/2, i.e. sigma = 256 ln 2 ~ 177: a level of that order puts the surface where a ray's transmittance
# drops within a step or two.  DESIGN.md section 3 ("Mesh extraction") records how this default was chosen.
DEFAULT_LEVEL = 177.0


def options(cfg):
    m = cfg.get("mesh") or {}
    ps = cfg.get("pts_sampler") or {}
    lo = [float(v) for v in m.get("bbox_min", ps.get("bbox_min", [-1.0, -1.0, -1.0]))]
    hi = [float(v) for v in m.get("bbox_max", ps.get("bbox_max", [1.0, 1.0, 1.0]))]
    return {"resolution": int(m.get("resolution", 256)), "level": float(m.get("level", DEFAULT_LEVEL)), "bbox_min": lo,
            "bbox_max": hi}


def to_world(verts, center, radius):
    """Normalised scene frame -> the data set's original frame (rigs.prepare_scene: p_norm = (p - center) / radius)."""
    v = np.asarray(verts, np.float32)
    return (v * np.float32(radius) + np.asarray(center, np.float32)[None]).astype(np.float32)


def write_ply(path, verts, faces):
    """Binary little-endian PLY: float x, y, z per vertex; `list uchar int vertex_indices` per face."""
    v = np.ascontiguousarray(verts, dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype="<i4").reshape(-1, 3)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
    rec = np.empty(len(f), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"] = 3
    rec["idx"] = f
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())
    return path


def extract(runner, cfg, scene, exp_dir):
    """Density grid -> iso-surface -> <exp_dir>/meshes/<iter>_<res>.ply, vertices in the data set's world frame."""
    o = options(cfg)
    verts, faces = runner.extract_mesh(o["bbox_min"], o["bbox_max"], o["resolution"], o["level"])
    v = to_world(verts.cpu().numpy(), scene["center"], scene["radius"])
    path = os.path.join(exp_dir, "meshes", "%d_%d.ply" % (runner.iter_step, o["resolution"]))
    write_ply(path, v, faces.cpu().numpy())
    print("Mesh: %d vertices, %d faces at level %g -> %s" % (len(v), len(faces), o["level"], path))
    return path
