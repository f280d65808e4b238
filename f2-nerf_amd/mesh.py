"""Mesh export of a trained scene: `python -m f2_nerf_amd.run ... mode=extract_mesh is_continue=true`.

The density grid and the iso-surface are computed on the device (ExpRunner.extract_mesh: f2n_oct_locate_warp_grid -> field
forward -> f2n_mesh_count / f2n_mesh_emit); this module only picks the options, maps the vertices back to the data set's world
frame and writes the PLY file.

Options (hydra-style overrides, no `mesh` group in the configs):
  mesh.resolution  cells along the longest side of the box (default 256)
  mesh.level       density iso-level (default DEFAULT_LEVEL)
  mesh.bbox_min / mesh.bbox_max  the box in the NORMALISED scene frame (default: pts_sampler.bbox_min / bbox_max, [-1, 1]^3,
                   which holds the normalised cameras; the octree's root cube is 512 wide and mostly empty)
  mesh.normals     true: per-vertex normals from the density grid's gradient (float nx, ny, nz; default false)
  mesh.normal_source  grid | field (default grid): where the normals of mesh.normals (and the view directions of mesh.colors) come
                   from -- the density grid's central differences, or the field's own analytic gradient at every vertex
                   (runner.query_density_grad; a vertex where that vanishes keeps its grid normal)
  mesh.colors      true: per-vertex colours (uchar red, green, blue; default false): the radiance AT the vertex seen along the
                   inward normal -- a single-point query, not a volume-rendered pixel
  mesh.min_component_faces  N > 1: connected components of fewer than N faces ("floaters") are dropped (default 0: none)
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
            "bbox_max": hi, "normals": _flag(m.get("normals", False)), "colors": _flag(m.get("colors", False)),
            "min_component_faces": int(m.get("min_component_faces", 0)), "normal_source": _normal_source(m.get("normal_source", "grid"))}


NORMAL_SOURCES = ("grid", "field")


def _normal_source(v):
    s = str(v).strip().lower()
    if s not in NORMAL_SOURCES:
        raise ValueError("mesh.normal_source must be one of %s, got %r" % (" | ".join(NORMAL_SOURCES), v))
    return s


def _flag(v):
    return v.strip().lower() in ("1", "true", "yes", "on") if isinstance(v, str) else bool(v)


def to_world(verts, center, radius):
    """Normalised scene frame -> the data set's original frame (rigs.prepare_scene: p_norm = (p - center) / radius)."""
    v = np.asarray(verts, np.float32)
    return (v * np.float32(radius) + np.asarray(center, np.float32)[None]).astype(np.float32)


def quantize_colors(colors):
    """float colours -> uint8 as the project quantises images for PSNR: (clip(c, 0, 1) * 255) truncated."""
    return (np.clip(np.asarray(colors, np.float32), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)


def write_ply(path, verts, faces, normals=None, colors=None):
    """Binary little-endian PLY: float x, y, z per vertex, then float nx, ny, nz (normals [V,3]) and / or uchar red, green, blue
    (colors [V,3] floats, quantize_colors) when given; `list uchar int vertex_indices` per face."""
    v = np.ascontiguousarray(verts, dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype="<i4").reshape(-1, 3)
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None or colors is not None:
        fields = [("xyz", "<f4", (3,))]
        if normals is not None:
            props += "property float nx\nproperty float ny\nproperty float nz\n"
            fields.append(("n", "<f4", (3,)))
        if colors is not None:
            props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            fields.append(("rgb", "u1", (3,)))
        vrec = np.empty(len(v), dtype=fields)
        vrec["xyz"] = v
        if normals is not None:
            vrec["n"] = np.asarray(normals, "<f4").reshape(len(v), 3)
        if colors is not None:
            vrec["rgb"] = quantize_colors(colors).reshape(len(v), 3)
        v = vrec
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v) + props +
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f))
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
    path = os.path.join(exp_dir, "meshes", "%d_%d.ply" % (runner.iter_step, o["resolution"]))
    if not (o["normals"] or o["colors"] or o["min_component_faces"] > 1):
        verts, faces = runner.extract_mesh(o["bbox_min"], o["bbox_max"], o["resolution"], o["level"])
        v = to_world(verts.cpu().numpy(), scene["center"], scene["radius"])
        write_ply(path, v, faces.cpu().numpy())
    else:
        m = runner.extract_mesh_attrs(o["bbox_min"], o["bbox_max"], o["resolution"], o["level"], o["min_component_faces"], o["normals"],
                                      o["colors"], o["normal_source"])
        verts, faces = m["verts"], m["faces"]
        v = to_world(verts.cpu().numpy(), scene["center"], scene["radius"])
        # (the world frame is a uniform scale and a shift of the normalised one: normals are the same in both)
        write_ply(path, v, faces.cpu().numpy(), m["normals"].cpu().numpy() if o["normals"] else None,
                  m["colors"].cpu().numpy() if o["colors"] else None)
    print("Mesh: %d vertices, %d faces at level %g -> %s" % (len(v), len(faces), o["level"], path))
    return path
