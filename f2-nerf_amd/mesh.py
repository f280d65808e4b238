"""Mesh export of a trained scene: `python -m f2_nerf_amd.run ... mode=extract_mesh is_continue=true`.

The density grid and the iso-surface are computed on the device (ExpRunner.extract_mesh: f2n_oct_locate_warp_grid -> field
forward -> f2n_mesh_count / f2n_mesh_emit); this module only picks the options, maps the vertices back to the data set's world
frame and writes the PLY file.

Options (hydra-style overrides, no `mesh` group in the configs):
  mesh.resolution  cells along the longest side of the box (default 256; at most 1024, with mesh.sparse or tsdf.sparse at most 8192)
  mesh.level       density iso-level (default DEFAULT_LEVEL)
  mesh.bbox_min / mesh.bbox_max  the box in the NORMALISED scene frame (default: pts_sampler.bbox_min / bbox_max, [-1, 1]^3,
                   which holds the normalised cameras; the octree's root cube is 512 wide and mostly empty)
  mesh.normals     true: per-vertex normals from the density grid's gradient (float nx, ny, nz; default false)
  mesh.normal_source  grid | field (default grid): where the normals of mesh.normals (and the view directions of mesh.colors) come
                   from -- the density grid's central differences, or the field's own analytic gradient at every vertex
                   (runner.query_density_grad; a vertex where that vanishes keeps its grid normal)
  mesh.colors      true: per-vertex colours (uchar red, green, blue; default false): the radiance AT the vertex seen along the
                   inward normal -- a single-point query, not a volume-rendered pixel
  mesh.color_source  radiance | views (default radiance: nothing changes): with views the colours of mesh.colors are the colours the
                   training views OBSERVED at the vertex, blended (fuse_view_colors, below); a vertex no view sees keeps its
                   radiance colour, so the file is fully coloured, and one line is printed: Colors: <known> of <n> vertices from
                   <V> views (1/<res_level>, tol <t>).  It works with either mesh.source, with mesh.sparse / tsdf.sparse,
                   mesh.simplify and mesh.refine (the final vertices, and the refined ones for _r.ply); mesh.colors raises when it
                   raised before
  mesh.min_component_faces  N > 1: connected components of fewer than N faces ("floaters") are dropped (default 0: none)
  mesh.simplify    k >= 2: the mesh is simplified by vertex clustering on cells of k grid steps with quadric-error placement
                   (host.mesh_simplify; default 0: off) after the floater removal and before normals and colours, which are computed
                   at the new vertices -> <iter>_<res>_s<k>.ply (<iter>_<res>_tsdf_s<k>.ply).  One vertex per occupied cell: features
                   thinner than a cell become two-sided sheets or non-manifold edges, never holes
  mesh.check       true: after the .ply is written the mesh is compared with the field it came from, seen from the training cameras
                   (check_mesh: the field's surface distance per ray against a ray cast at the mesh, host.mesh_raycast) ->
                   <same name>_check.json and one printed line; options check.res_level (4), check.tau (0.5), check.min_opacity (0.5),
                   check.max_views (0: all), with the meaning of their tsdf.* namesakes.  Default false: nothing changes
  mesh.texture     true: the mesh just written is also exported with a baked texture (runner.bake_texture: one right-triangle chart per
                   face in a power-of-two atlas, host.mesh_atlas; every owned texel takes the field's colour at its point of the
                   surface) -> <same name>_tex.obj, _tex.mtl and _tex.png, and one printed line.  It works with either mesh.source and
                   with or without mesh.simplify, and computes the per-vertex normals whether or not mesh.normals writes them to the
                   .ply.  Options: texture.texels_per_step (2.0: texels per grid step of mesh.resolution; not measured on a scene),
                   texture.max_size (8192, a power of two: the density is halved until the atlas fits), texture.max_block_log2 (7),
                   texture.source (point | ray | views: the radiance AT the texel's point seen along the inward normal, as
                   mesh.colors, the volume-rendered colour of a short ray through it, or the colours the training views observed
                   there -- fuse_view_colors with the colors.* options; a texel no view sees takes the point colour and the
                   Texture: line names the texels that came from views), texture.ray_steps (4.0 grid steps, the TSDF truncation's
                   default; not measured on a scene).  With mesh.check the check JSON gains texture_psnr and n_texture_rays.
                   Known limits: no mip-safe padding between blocks (nearest and bilinear filtering are clean, mipmaps bleed); charts
                   are per face, so filtering is not seam-free across edges beyond the replicated gutter; a chart's anisotropy is
                   bounded only by putting the longest edge on the diagonal.  Default false: nothing changes
  mesh.distance    true (needs mesh.simplify=k >= 2): the simplified mesh just written is compared with the unsimplified one (the same
                   floater filter, extracted once more without the simplification) by mesh_distance: sampled surface-to-surface
                   distances in both directions (host.mesh_sample_surface, host.mesh_closest_point) -> <same name>_distance.json
                   (a_to_b: from this mesh to the other, b_to_a: back; chamfer, a sampled hausdorff, precision / recall / F-score per
                   threshold, all in grid steps) and one printed line.  It works with either mesh.source.  Default false: nothing changes
  mesh.distance_to  <file.ply>: the mesh just written is compared with that triangle mesh instead (read_ply), both in the data set's
                   WORLD frame -- another export of the same scene (the TSDF mesh against the density mesh) or a scan a user brings.
                   It excludes mesh.distance=true (one JSON per mesh).  mesh.distance=true compares in the world frame too, on the
                   float32 vertices a .ply carries, so mesh.distance_to=<the same run's unsimplified .ply> gives its figures.  Options of both: distance.samples (200 000 per side),
                   distance.seed (0), distance.thresholds ([0.5, 1, 2] grid steps), distance.max_dist_steps (none: samples farther than
                   this many grid steps from the other mesh are counted as missed and left out of the statistics).  The sample
                   count and the thresholds are choices, not measurements
  mesh.refine      true: after the mesh is written as ever, a refined copy is made by the refine stage (after the floater removal and the
                   simplification, before normals, colours, texture, check and distance, which then all see the refined vertices):
                   refine.smooth_passes Taubin lambda|mu pairs over the vertex one-ring (host.mesh_smooth; default 2, a choice;
                   refine.lam 0.5 and refine.mu -0.53: Taubin's pass band 1/lam + 1/mu ~ 0.1, a literature value), then every vertex
                   is moved onto the level set by a damped Newton iteration on ln(sigma) - ln(level) along the field's analytic
                   gradient (runner.project_to_level; refine.project, default true; refine.iters 8 field evaluations; refine.tol 1e-3
                   in ln(sigma), a 0.1 % density error: a choice; refine.max_step_steps 0.5: a choice; refine.max_move_steps 1.0 grid
                   steps from where the mesher put the vertex: the surface crosses the very edge the vertex sits on, at most sqrt(3)
                   steps long -- a geometric argument, not a measurement; both are multiplied by mesh.simplify when that is >= 2)
                   -> <same name>_r.ply, <same name>_r_refine.json (status counts, |ln(sigma/level)| before and after, the distance
                   moved in grid steps, face quality before and after, flipped_faces, boundary_edges, nonmanifold_edges) and one
                   printed line.  mesh.source=tsdf: the smoothing applies, the projection does not (the TSDF surface is no density
                   level set: refine.project=true is an error there, unset means off).  Known limits: vertices on a boundary or
                   non-manifold edge are pinned by the smoothing, so an open rim keeps its shape; nothing prevents
                   self-intersection (flipped_faces only counts faces whose normal turned over); the projection follows ln(sigma),
                   so a vertex in an empty leaf stays where it is.  Default false: nothing changes
  mesh.source      density | tsdf (default density): the iso-surface of the raw density at mesh.level, or the zero crossing of a
                   truncated signed distance field fused from the training views' rendered depth (fuse_tsdf; mesh.level is not
                   used, normals of source "grid" come from the TSDF) -> <exp>/meshes/<iter>_<res>_tsdf.ply
  mesh.sparse      true | 4 | 8 | 16 (true = 8; default false): the same mesh, bit for bit, without the dense grid
                   (runner.extract_mesh_sparse): the box is cut into bricks of B^3 cells, only the bricks whose box meets a live octree
                   leaf are evaluated (f2n_brick_mark), in batches, and meshed brick by brick (f2n_brick_mesh_count / _emit); memory
                   follows the batch and the mesh, not the box, and mesh.resolution may go up to 8192.  The file names are unchanged and
                   the printed line gains the active and total brick counts.  It composes with mesh.simplify, mesh.refine,
                   mesh.texture, mesh.check and mesh.distance* as the dense path does.  No dense grid exists, so normals and colours
                   (mesh.normals, mesh.colors, mesh.texture) need mesh.normal_source=field -- a vertex where the field's gradient
                   vanishes then keeps the normal (0, 0, 0) -- and mesh.source=tsdf is refused (its sparse path is tsdf.sparse):
                   both are a ValueError before anything is extracted.  mesh.level must be >= 0 (the cull is exact only then).
                   B = 8 is a choice, not a measurement: a brick evaluates (B + 1)^3 corners for B^3 cells, (9/8)^3 = 1.42x
                   duplicated corners against 1.20x at 16, and culls at a finer grain

TSDF fusion (mesh.source=tsdf): every training camera is rendered with runner.render_geometry at 1/res_level of its resolution, the rays'
surface distances (surf_t, weighted by the rays' opacity) are fused into the grid of mesh.resolution / mesh.bbox_* (f2n_tsdf_integrate),
and the masked mesher leaves the surface open where no camera looked (f2n_mesh_count_masked).  Options:
  tsdf.res_level     the depth maps are rendered at 1/res_level of the cameras' resolution (default 4)
  tsdf.trunc_voxels  truncation distance in grid steps (default 4)
  tsdf.tau           the surface of a ray is its first sample at which the accumulated weight reaches tau (default 0.5)
  tsdf.min_opacity   rays whose opacity is below this carry no surface (default 0.5)
  tsdf.min_weight    a grid point is known where its summed weight reaches this (default 1.0)
  tsdf.views_per_batch  cameras rendered per integration launch (default 8); the result does not depend on it
  tsdf.max_views     only the first N training cameras are fused (default 0: all)
  tsdf.sparse        true | 4 | 8 | 16 (true = 8; default false): the same mesh, bit for bit, without the dense sums (fuse_tsdf_sparse):
                     the views' depth maps are kept on the device, the bricks of B^3 cells whose corners some view sees at most the
                     truncation behind its surface are marked (f2n_tsdf_brick_mark), and only those are integrated, finalized and
                     meshed, a batch of rows at a time; memory follows the batch, the mesh and the depth maps (8 B per depth pixel
                     and view), not the box, and mesh.resolution may go up to 8192.  The mark costs what a dense integration costs in
                     arithmetic (grid points x views): the option saves memory, not time.  The file name is unchanged and the printed
                     line names the brick counts in the place of the known grid points.  No dense TSDF exists, so mesh.normals,
                     mesh.colors and mesh.texture need mesh.normal_source=field (a vertex where the field's gradient vanishes keeps
                     the normal (0, 0, 0)): anything else is a ValueError before a view is rendered.  B = 8 is inherited from
                     mesh.sparse, not measured for this path.  (mesh.sparse itself stays refused with mesh.source=tsdf.)

View colours (mesh.color_source=views, texture.source=views): every surface point is projected into the training views that see it
(f2n_view_colors_accumulate: the camera model of the TSDF, a bilinear lookup whose four taps are each tested for occlusion against the
view's rendered depth) and the observed colours are blended, weighted by the rendered opacity times the cosine between the normal
and the viewing direction -- a weighted mean over all views, no best-view pick: a choice, not a measurement.  Options, every default
a choice (the thresholds are those of tsdf.* and points.*), none measured on a converged scene:
  colors.res_level   the views are rendered at 1/res_level of the cameras' resolution (default 2)
  colors.tol_steps   a tap sees the point when its depth is within this many grid steps of the point's distance (default 2.0)
  colors.cos_min     views that meet the surface at a cosine at or below this are skipped (default 0.1; a point without a normal
                     skips none)
  colors.min_views   a point is known when at least this many views contributed (default 1)
  colors.max_views   only the first N training cameras are used (default 0: all)
  colors.views_per_batch  cameras rendered per launch (default 8); the result does not depend on it
  colors.tau, colors.min_opacity  as tsdf.tau and tsdf.min_opacity (default 0.5 both)
  colors.image       render | photo (default render): the colours the field renders from the view, or the photograph's pixels

Point-cloud export: `mode=extract_points is_continue=true` renders every training camera with runner.render_geometry and writes the
rays' surface points, oriented and coloured, to <exp>/points/<iter>.ply in the data set's world frame (the usual input of a Poisson
reconstruction, and the cheapest check on a mesh export).  Options:
  points.res_level   the cameras are rendered at 1/res_level of their resolution (default 4)
  points.tau         the surface of a ray is its first sample at which the accumulated weight reaches tau (default 0.5)
  points.min_opacity rays whose opacity (the sum of their weights) is below this are dropped (default 0.5)
  points.normals     surface | composited (default surface): the field's normal at the surface sample, or the weight-composited one
  points.max_points  at most this many points are kept (default 2 000 000), by a fixed stride over the kept rays: no random draw
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
            "min_component_faces": int(m.get("min_component_faces", 0)), "normal_source": _normal_source(m.get("normal_source", "grid")),
            "source": _source(m.get("source", "density")), "simplify": _simplify(m.get("simplify", 0)),
            "refine": refine_options(cfg, _source(m.get("source", "density"))), "sparse": _sparse(m.get("sparse", False))}


def _sparse(v):
    """mesh.sparse: 0 (off) or the brick size 4 | 8 | 16; true means 8"""
    s = str(v).strip().lower()
    if s in ("false", "0", "no", "off", "none", ""):
        return 0
    if s in ("true", "yes", "on"):
        return 8
    if s in ("4", "8", "16"):
        return int(s)
    raise ValueError("mesh.sparse must be true, false, 4, 8 or 16, got %r" % (v,))


def refine_options(cfg, source="density"):
    """mesh.refine and the refine.* options: None when the stage is off, else the dict runner.extract_mesh_attrs(..., refine=) takes.
    Every default is a choice or a literature value, none is measured on a scene (the module's docstring says which)."""
    import math
    m = cfg.get("mesh") or {}
    r = cfg.get("refine") or {}
    if not _flag(m.get("refine", False)):
        return None

    def whole(name, default):
        v = r.get(name, default)
        if v is None or isinstance(v, bool) or (isinstance(v, float) and v != int(v)):
            raise ValueError("refine.%s must be an integer, got %r" % (name, v))
        return int(v)  # (ValueError for a string that is not an integer)
    project = r.get("project", None)
    if project is not None and _flag(project) and source == "tsdf":
        raise ValueError("refine.project=true with mesh.source=tsdf: the TSDF surface is no level set of the density (the smoothing applies; "
                         "leave refine.project unset)")
    o = {"smooth_passes": whole("smooth_passes", 2), "lam": float(r.get("lam", 0.5)), "mu": float(r.get("mu", -0.53)),
         "project": source != "tsdf" if project is None else _flag(project), "iters": whole("iters", 8),
         "max_step_steps": float(r.get("max_step_steps", 0.5)), "max_move_steps": float(r.get("max_move_steps", 1.0)),
         "tol": float(r.get("tol", 1e-3))}
    if (o["smooth_passes"] < 0 or o["iters"] < 1 or not math.isfinite(o["lam"]) or not math.isfinite(o["mu"]) or not o["max_step_steps"] > 0.0 or
            not o["max_move_steps"] > 0.0 or not 0.0 <= o["tol"] < float("inf")):
        raise ValueError("refine.smooth_passes must be >= 0, refine.iters >= 1, refine.lam and refine.mu finite, refine.max_step_steps and "
                         "refine.max_move_steps > 0, refine.tol >= 0 and finite, got %r" % (o,))
    return o


def _lower(x, q):
    """the element floor(q (n - 1)) of the n ascending values (as the runner's refine statistics): a sort, no interpolation"""
    e = np.sort(np.asarray(x, np.float64).reshape(-1))
    return float(e[int(np.floor(q * (len(e) - 1)))]) if len(e) else float("nan")


def _write_refined(path, scene, verts, faces, normals, colors, stats):
    """<path without .ply>_r.ply, <the same>_r_refine.json and the Refine: line; returns the refined file's path"""
    import json
    rpath = path[:-4] + "_r.ply"
    v = to_world(verts.cpu().numpy(), scene["center"], scene["radius"])
    write_ply(rpath, v, faces.cpu().numpy(), normals, colors)
    out = rpath[:-4] + "_refine.json"
    with open(out, "w") as fh:
        json.dump(stats, fh, indent=1, sort_keys=True)
    g = lambda key: stats.get(key, float("nan"))  # noqa: E731
    n = lambda key: int(stats.get(key, 0))  # noqa: E731
    proj = ("|ln(sigma/level)| median %.4g -> %.4g, p90 %.4g -> %.4g, %d converged, %d empty" % (
        g("h_median_before"), g("h_median_after"), g("h_p90_before"), g("h_p90_after"), n("converged"), n("empty"))) if "h_median_before" in stats \
        else "no projection"
    print("Refine: %d vertices, %d smoothing pairs, %s; moved %.3f / %.3f / %.3f grid steps (median / p90 / max), face quality p05 %.3f -> %.3f, "
          "median %.3f -> %.3f, %d flipped faces, %d boundary and %d non-manifold edges -> %s, %s" % (
              len(v), n("smooth_passes"), proj, g("moved_median"), g("moved_p90"), g("moved_max"), g("quality_p05_before"), g("quality_p05_after"),
              g("quality_median_before"), g("quality_median_after"), n("flipped_faces"), n("boundary_edges"), n("nonmanifold_edges"), rpath, out))
    return rpath


def _simplify(v):
    if v is None or isinstance(v, bool) or (isinstance(v, float) and v != int(v)):
        raise ValueError("mesh.simplify must be an integer >= 0, got %r" % (v,))
    k = int(v)  # (ValueError for a string that is not an integer)
    if k < 0:
        raise ValueError("mesh.simplify must be an integer >= 0 (cells of k grid steps; 0 or 1: off), got %r" % (v,))
    return k


SOURCES = ("density", "tsdf")


def _source(v):
    s = str(v).strip().lower()
    if s not in SOURCES:
        raise ValueError("mesh.source must be one of %s, got %r" % (" | ".join(SOURCES), v))
    return s


def tsdf_options(cfg):
    """The tsdf.* options.  The defaults follow common practice (a truncation of a few voxels, the point-cloud export's thresholds); none
    of them is measured on a scene."""
    t = cfg.get("tsdf") or {}
    o = {"res_level": int(t.get("res_level", 4)), "trunc_voxels": float(t.get("trunc_voxels", 4.0)), "tau": float(t.get("tau", 0.5)),
         "min_opacity": float(t.get("min_opacity", 0.5)), "min_weight": float(t.get("min_weight", 1.0)),
         "views_per_batch": int(t.get("views_per_batch", 8)), "max_views": int(t.get("max_views", 0))}
    if "sparse" in t:  # (absent without the key: the dense export's options are what they were)
        try:
            o["sparse"] = _sparse(t["sparse"])
        except ValueError:
            raise ValueError("tsdf.sparse must be true, false, 4, 8 or 16, got %r" % (t["sparse"],)) from None
    if (o["res_level"] < 1 or o["views_per_batch"] < 1 or o["max_views"] < 0 or not 0.0 < o["tau"] <= 1.0 or
            not 0.0 < o["trunc_voxels"] < float("inf") or not o["min_weight"] >= 0.0 or not o["min_opacity"] >= 0.0):
        raise ValueError("tsdf.res_level and tsdf.views_per_batch must be >= 1, tsdf.max_views >= 0, tsdf.tau in (0, 1], tsdf.trunc_voxels "
                         "> 0 and finite, tsdf.min_weight and tsdf.min_opacity >= 0, got %r" % (o,))
    return o


NORMAL_SOURCES = ("grid", "field")


def _normal_source(v):
    s = str(v).strip().lower()
    if s not in NORMAL_SOURCES:
        raise ValueError("mesh.normal_source must be one of %s, got %r" % (" | ".join(NORMAL_SOURCES), v))
    return s


POINT_NORMALS = ("surface", "composited")


def points_options(cfg):
    p = cfg.get("points") or {}
    nrm = str(p.get("normals", "surface")).strip().lower()
    if nrm not in POINT_NORMALS:
        raise ValueError("points.normals must be one of %s, got %r" % (" | ".join(POINT_NORMALS), p.get("normals")))
    o = {"res_level": int(p.get("res_level", 4)), "min_opacity": float(p.get("min_opacity", 0.5)), "tau": float(p.get("tau", 0.5)),
         "normals": nrm, "max_points": int(p.get("max_points", 2000000))}
    if o["res_level"] < 1 or o["max_points"] < 1 or not 0.0 < o["tau"] <= 1.0:
        raise ValueError("points.res_level and points.max_points must be >= 1 and points.tau in (0, 1], got %r" % (o,))
    return o


def stride_subset(n, cap):
    """Indices of at most `cap` of n items: every k-th with the smallest k that fits (all of them when n <= cap)."""
    k = max(1, -(-int(n) // int(cap)))
    return np.arange(0, int(n), k)


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


def write_points_ply(path, points, normals=None, colors=None):
    """Binary little-endian PLY of a point cloud: the vertex element of write_ply (float x, y, z, then float nx, ny, nz and / or uchar
    red, green, blue when given) and no face element."""
    v = np.ascontiguousarray(points, dtype="<f4").reshape(-1, 3)
    props = "property float x\nproperty float y\nproperty float z\n"
    fields = [("xyz", "<f4", (3,))]
    for name, arr in (("normals", normals), ("colors", colors)):
        if arr is not None and np.asarray(arr).reshape(-1, 3).shape[0] != len(v):
            raise ValueError("%s: %d rows for %d points" % (name, np.asarray(arr).reshape(-1, 3).shape[0], len(v)))
    if normals is not None:
        props += "property float nx\nproperty float ny\nproperty float nz\n"
        fields.append(("n", "<f4", (3,)))
    if colors is not None:
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        fields.append(("rgb", "u1", (3,)))
    rec = np.empty(len(v), dtype=fields)
    rec["xyz"] = v
    if normals is not None:
        rec["n"] = np.asarray(normals, "<f4").reshape(len(v), 3)
    if colors is not None:
        rec["rgb"] = quantize_colors(colors).reshape(len(v), 3)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v) + props + "end_header\n").encode("ascii"))
        fh.write(rec.tobytes())
    return path


def camera_rays(dataset, bounds, idx, res_level):
    """Rays of camera idx at 1 / res_level of its resolution (the pixel grid of Dataset::RaysFromPose), with that camera's bounds."""
    import torch
    H, W = max(1, int(dataset.height) // res_level), max(1, int(dataset.width) // res_level)
    ii = torch.linspace(0.0, dataset.height - 1.0, H, device="cuda").to(torch.int32)
    jj = torch.linspace(0.0, dataset.width - 1.0, W, device="cuda").to(torch.int32)
    gi, gj = torch.meshgrid(ii, jj, indexing="ij")
    ij = torch.stack([gi.reshape(-1), gj.reshape(-1)], -1).contiguous()
    ro, rd = dataset.img2world_ray_flex(torch.full((H * W,), int(idx), dtype=torch.int32, device="cuda"), ij)
    b = torch.as_tensor(np.asarray(bounds, np.float32)[idx], device="cuda").reshape(1, 2).repeat(H * W, 1).contiguous()
    return ro, rd, b


def extract_points(runner, cfg, scene, dataset, exp_dir):
    """Every training camera -> runner.render_geometry -> the rays that found a surface -> <exp_dir>/points/<iter>.ply."""
    o = points_options(cfg)
    pts, nrm, col = [], [], []
    for idx in scene["train_set"]:
        ro, rd, b = camera_rays(dataset, scene["bounds"], int(idx), o["res_level"])
        g = runner.render_geometry(ro, rd, b, tau=o["tau"])
        keep = (g["surf_idx"] >= 0) & (g["opacity"] >= o["min_opacity"])
        pts.append(g["surf_points"][keep].cpu().numpy())
        nrm.append(g["surf_normals" if o["normals"] == "surface" else "normals"][keep].cpu().numpy())
        col.append(g["colors"][keep].cpu().numpy())
    pts, nrm, col = (np.concatenate(a).reshape(-1, 3) if a else np.zeros((0, 3), np.float32) for a in (pts, nrm, col))
    n_kept = len(pts)
    sel = stride_subset(n_kept, o["max_points"])
    path = os.path.join(exp_dir, "points", "%d.ply" % runner.iter_step)
    # (the world frame is a uniform scale and a shift of the normalised one: normals are the same in both)
    write_points_ply(path, to_world(pts[sel], scene["center"], scene["radius"]), nrm[sel], col[sel])
    print("Points: %d of %d rays with a surface from %d cameras (tau %g, opacity >= %g) -> %s" % (
        len(sel), n_kept, len(scene["train_set"]), o["tau"], o["min_opacity"], path))
    return path


def tsdf_camera_rays(dataset, bounds, idx, s):
    """Rays of camera idx on the regular sub-grid of the TSDF depth maps: h = H // s, w = W // s, entry (a, b) looks through pixel
    (a s + s // 2, b s + s // 2) -- inside pixel (a, b) of an image s times smaller, whose intrinsics are fx, fy, cx, cy divided by s.
    Returns (rays_o, rays_d, bounds, h, w)."""
    import torch
    ij, h, w = tsdf_pixels(dataset, s)
    ro, rd = dataset.img2world_ray_flex(torch.full((h * w,), int(idx), dtype=torch.int32, device="cuda"), ij)
    b = torch.as_tensor(np.asarray(bounds, np.float32)[idx], device="cuda").reshape(1, 2).repeat(h * w, 1).contiguous()
    return ro, rd, b, h, w


def tsdf_pixels(dataset, s):
    """(ij [h w, 2] int32, h, w): the full-resolution pixels (a s + s // 2, b s + s // 2) the map entries (a, b) of tsdf_camera_rays look
    through, row-major."""
    import torch
    s = int(s)
    h, w = int(dataset.height) // s, int(dataset.width) // s
    if h < 1 or w < 1:
        raise ValueError("tsdf.res_level %d leaves no pixel of a %d x %d image" % (s, int(dataset.height), int(dataset.width)))
    ii = torch.arange(h, dtype=torch.int32, device="cuda") * s + s // 2
    jj = torch.arange(w, dtype=torch.int32, device="cuda") * s + s // 2
    gi, gj = torch.meshgrid(ii, jj, indexing="ij")
    return torch.stack([gi.reshape(-1), gj.reshape(-1)], -1).contiguous(), h, w


def tsdf_intrinsics(intri, s):
    """intri [V,3,3] in units of the depth maps' pixels: fx, fy, cx, cy divided by s (float32)."""
    k = np.array(intri, np.float32, copy=True).reshape(-1, 3, 3)
    for r, c in ((0, 0), (1, 1), (0, 2), (1, 2)):
        k[:, r, c] = k[:, r, c] / np.float32(s)
    return k


def _tsdf_view_maps(runner, dataset, scene, o, idx, with_colors=False):
    """(depth, conf) [h, w] of training camera idx as the TSDF takes them: the rays' surface distance where the ray has a surface and
    its opacity reaches o["min_opacity"] (0 elsewhere), and the opacity.  with_colors: the rays' rendered colours [h, w, 3] as a third."""
    import torch
    ro, rd, b, h, w = tsdf_camera_rays(dataset, scene["bounds"], idx, int(o["res_level"]))
    g = runner.render_geometry(ro, rd, b, tau=o["tau"])
    hit = (g["surf_idx"] >= 0) & (g["opacity"] >= o["min_opacity"])
    maps = torch.where(hit, g["surf_t"], torch.zeros_like(g["surf_t"])).reshape(h, w), g["opacity"].reshape(h, w)
    return maps + (g["colors"].reshape(h, w, 3),) if with_colors else maps


def view_intrinsics(intri, s):
    """intri [V,3,3] in units of the maps' pixels WITH the pixel centres in place (float32): entry (a, b) of the maps of
    tsdf_camera_rays looks through the centre (b s + s // 2 + 0.5, a s + s // 2 + 0.5) of a full-resolution pixel (the + 0.5 of
    f2n_img2world_rays), and these intrinsics put that ray at the entry's centre (b + 0.5, a + 0.5): fx / s, fy / s,
    cx' = (cx - s // 2 - 0.5) / s + 0.5, cy' likewise.  What a bilinear lookup needs; tsdf_intrinsics (cx / s) is right to within the
    pixel, which is all a nearest lookup asks for."""
    k = np.array(intri, np.float32, copy=True).reshape(-1, 3, 3)
    s32, off = np.float32(s), np.float32(int(s) // 2) + np.float32(0.5)
    for r in (0, 1):
        k[:, r, r] = k[:, r, r] / s32
        k[:, r, 2] = (k[:, r, 2] - off) / s32 + np.float32(0.5)
    return k


COLOR_SOURCES = ("radiance", "views")
COLOR_IMAGES = ("render", "photo")


def view_color_options(cfg):
    """mesh.color_source and the colors.* options (a dict of its own: options() keeps its keys).  Every default is a choice: the
    thresholds are those of tsdf.* and points.*, res_level 2 is one step finer than the TSDF's depth maps, tol_steps 2 half of the TSDF's
    truncation, cos_min 0.1 drops views within 6 degrees of grazing; none of them is measured on a converged scene."""
    m = cfg.get("mesh") or {}
    c = cfg.get("colors") or {}
    src = str(m.get("color_source", "radiance")).strip().lower()
    if src not in COLOR_SOURCES:
        raise ValueError("mesh.color_source must be one of %s, got %r" % (" | ".join(COLOR_SOURCES), m.get("color_source")))
    img = str(c.get("image", "render")).strip().lower()
    if img not in COLOR_IMAGES:
        raise ValueError("colors.image must be one of %s, got %r" % (" | ".join(COLOR_IMAGES), c.get("image")))
    o = {"color_source": src, "res_level": int(c.get("res_level", 2)), "tol_steps": float(c.get("tol_steps", 2.0)),
         "cos_min": float(c.get("cos_min", 0.1)), "min_views": int(c.get("min_views", 1)), "max_views": int(c.get("max_views", 0)),
         "views_per_batch": int(c.get("views_per_batch", 8)), "tau": float(c.get("tau", 0.5)), "min_opacity": float(c.get("min_opacity", 0.5)),
         "image": img}
    if (o["res_level"] < 1 or o["views_per_batch"] < 1 or o["max_views"] < 0 or o["min_views"] < 1 or not 0.0 < o["tau"] <= 1.0 or
            not 0.0 < o["tol_steps"] < float("inf") or not -1.0 <= o["cos_min"] < 1.0 or not o["min_opacity"] >= 0.0):
        raise ValueError("colors.res_level, colors.views_per_batch and colors.min_views must be >= 1, colors.max_views >= 0, colors.tau in "
                         "(0, 1], colors.tol_steps > 0 and finite, colors.cos_min in [-1, 1), colors.min_opacity >= 0, got %r" % (o,))
    return o


def fuse_view_colors(runner, dataset, scene, points, normals, o):
    """The colours the training views observed at points [n,3] (NORMALISED frame; outward normals [n,3] or None), blended
    (f2n_view_colors_accumulate / _finalize).  o: view_color_options() plus "step", the grid step the tolerance is counted in
    (tol = tol_steps * step as ONE float32 product).  The selected training cameras are rendered in batches of o["views_per_batch"]
    exactly as fuse_tsdf renders them (depth and conf of _tsdf_view_maps at o["res_level"]); the image is the render's colours, or with
    o["image"] == "photo" the photographs at the same pixels (dataset.gather_colors); the intrinsics are view_intrinsics.  The sums of
    all points stay resident, one batch of maps is alive at a time, and the batch size does not show in the result's bits.  Returns
    dict(colors [n,3], known [n] bool, weight [n], count [n] int32, n_views, tol), tensors on the device.  No side effect on training:
    nothing is drawn, no vote is cast, a pending step is flushed first."""
    import torch
    from . import runtime
    host = runtime.host()
    runner.flush()
    pts = points.to("cuda", torch.float32).reshape(-1, 3).contiguous()
    nrm = None if normals is None else normals.to("cuda", torch.float32).reshape(-1, 3).contiguous()
    n = int(pts.shape[0])
    acc = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    wsum = torch.zeros((n,), dtype=torch.float32, device="cuda")
    count = torch.zeros((n,), dtype=torch.int32, device="cuda")
    views = [int(v) for v in scene["train_set"]]
    if o["max_views"] > 0:
        views = views[:o["max_views"]]
    s = int(o["res_level"])
    tol = float(np.float32(o["tol_steps"]) * np.float32(o["step"]))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    ij, h, w = tsdf_pixels(dataset, s)
    for k in range(0, len(views), o["views_per_batch"]):
        batch = views[k:k + o["views_per_batch"]]
        depth, conf, image = [], [], []
        for idx in batch:
            d, c, im = _tsdf_view_maps(runner, dataset, scene, o, idx, True)
            if o["image"] == "photo":
                im = dataset.gather_colors(torch.full((h * w,), idx, dtype=torch.int32, device="cuda"), ij).reshape(h, w, 3)
            depth.append(d)
            conf.append(c)
            image.append(im)
        host.view_colors_accumulate(acc, wsum, count, pts, nrm, dev(np.asarray(scene["poses"], np.float32)[batch]),
                                    dev(view_intrinsics(np.asarray(scene["intri"])[batch], s)),
                                    dev(np.asarray(scene["dist_params"], np.float32)[batch]), torch.stack(depth).contiguous(),
                                    torch.stack(conf).contiguous(), torch.stack(image).contiguous(), tol, float(o["cos_min"]))
    rgb, known = host.view_colors_finalize(acc, wsum, count, int(o["min_views"]))
    return {"colors": rgb, "known": known != 0, "weight": wsum, "count": count, "n_views": len(views), "tol": tol}


def _view_colors_fn(runner, cfg, scene, dataset, step, totals=None):
    """fn(points, normals) -> (rgb, known) of fuse_view_colors with the options of cfg, as bake_texture's view_colors takes it; totals (a
    dict, optional) receives n_views and tol of the last call."""
    if dataset is None:
        raise ValueError("mesh.color_source=views and texture.source=views render the training cameras: they need the data set")
    o = view_color_options(cfg)
    o["step"] = float(step)

    def fn(points, normals):
        r = fuse_view_colors(runner, dataset, scene, points, normals, o)
        if totals is not None:
            totals.update(n_views=r["n_views"], tol=r["tol"], res_level=o["res_level"])
        return r["colors"], r["known"]
    return fn


def _colors_from_views(fn, totals, verts, normals, colors):
    """mesh.color_source=views: the radiance colours [n,3] (numpy) of the vertices with the fused view colour where that is known, and the
    Colors: line."""
    import torch
    rgb, known = fn(verts, normals)
    out = torch.where(known[:, None], rgb, torch.as_tensor(np.asarray(colors, np.float32), device=rgb.device).reshape(-1, 3))
    print("Colors: %d of %d vertices from %d views (1/%d, tol %g)" % (int(known.sum()), int(known.numel()), totals["n_views"],
                                                                     totals["res_level"], totals["tol"]))
    return out.cpu().numpy()


def fuse_tsdf(runner, dataset, scene, o):
    """The training views' rendered depth fused into a TSDF on the grid of o["bbox_min"] / o["bbox_max"] / o["resolution"] (the grid of
    runner.density_grid).  o: options() and tsdf_options() in one dict.  Returns dict(g [nz, ny, nx] positive inside, valid uint8, S, W,
    lo, step), tensors on the device.  No side effect on training: nothing is drawn, no vote is cast, a pending step is flushed first."""
    import torch
    from . import runtime
    host = runtime.host()
    runner.flush()
    lo = [float(v) for v in o["bbox_min"]]
    step, nx, ny, nz = host.grid_spec(lo, [float(v) for v in o["bbox_max"]], int(o["resolution"]))
    S = torch.zeros((nz, ny, nx), dtype=torch.float32, device="cuda")
    W = torch.zeros((nz, ny, nx), dtype=torch.float32, device="cuda")
    views = [int(v) for v in scene["train_set"]]
    if o["max_views"] > 0:
        views = views[:o["max_views"]]
    s = int(o["res_level"])
    trunc = float(np.float32(o["trunc_voxels"]) * np.float32(step))
    for k in range(0, len(views), o["views_per_batch"]):
        batch = views[k:k + o["views_per_batch"]]
        depth, conf = [], []
        for idx in batch:
            d, c = _tsdf_view_maps(runner, dataset, scene, o, idx)
            depth.append(d)
            conf.append(c)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
        host.tsdf_integrate(S, W, lo, step, dev(np.asarray(scene["poses"], np.float32)[batch]), dev(tsdf_intrinsics(np.asarray(scene["intri"])[batch], s)),
                            dev(np.asarray(scene["dist_params"], np.float32)[batch]), torch.stack(depth).contiguous(),
                            torch.stack(conf).contiguous(), trunc)
    g, valid = host.tsdf_finalize(S, W, float(o["min_weight"]))
    return {"g": g, "valid": valid, "S": S, "W": W, "lo": lo, "step": step, "n_views": len(views), "trunc": trunc}


SPARSE_MAX_RES = 8192  # (the virtual grid of the sparse exports)


def fuse_tsdf_sparse(runner, dataset, scene, o, brick=8):
    """fuse_tsdf followed by the masked mesher at level 0, bit for bit, without the dense sums: every selected view is rendered exactly as
    fuse_tsdf renders it and its depth and conf maps are KEPT on the device as [V, h, w] (8 B per depth pixel and view: the mark needs
    every view before any brick is integrated); host.tsdf_mesh_sparse then marks the bricks of brick^3 cells whose row holds a corner some
    view sees at most trunc behind its surface, and takes the flagged bricks in ascending order in batches of
    max(1, runner.density_slab_points // (brick + 1)^3): zeroed S / W rows -> f2n_tsdf_integrate_bricks over all views -> f2n_tsdf_finalize
    -> one masked mesh batch; only one batch of rows is alive at a time.  The mark costs what a dense integration costs (grid points x
    views): memory is saved, not arithmetic.  Returns dict(verts, faces, lo, step, n_views, trunc, stats) with stats = {bricks,
    active_bricks, meshed_bricks, points_evaluated, points_known, batches, grid}.  No side effect on training, as fuse_tsdf."""
    import torch
    from . import runtime
    host = runtime.host()
    runner.flush()
    B = int(brick)
    lo = [float(v) for v in o["bbox_min"]]
    step, nx, ny, nz = host.grid_spec(lo, [float(v) for v in o["bbox_max"]], int(o["resolution"]), SPARSE_MAX_RES)
    views = [int(v) for v in scene["train_set"]]
    if o["max_views"] > 0:
        views = views[:o["max_views"]]
    s = int(o["res_level"])
    trunc = float(np.float32(o["trunc_voxels"]) * np.float32(step))
    maps = [_tsdf_view_maps(runner, dataset, scene, o, idx) for idx in views]
    h, w = int(dataset.height) // s, int(dataset.width) // s
    depth = torch.stack([m[0] for m in maps]).contiguous() if maps else torch.zeros((0, h, w), device="cuda")
    conf = torch.stack([m[1] for m in maps]).contiguous() if maps else torch.zeros((0, h, w), device="cuda")
    del maps
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    per = max(1, int(runner.density_slab_points) // (B + 1) ** 3)
    verts, faces, stats = host.tsdf_mesh_sparse(lo, step, [nx, ny, nz], B, dev(np.asarray(scene["poses"], np.float32)[views]),
                                                dev(tsdf_intrinsics(np.asarray(scene["intri"])[views], s)),
                                                dev(np.asarray(scene["dist_params"], np.float32)[views]), depth, conf, trunc,
                                                float(o["min_weight"]), per)
    return {"verts": verts, "faces": faces, "lo": lo, "step": step, "n_views": len(views), "trunc": trunc, "stats": dict(stats)}


def extract_tsdf(runner, cfg, scene, dataset, exp_dir):
    """fuse_tsdf -> the masked mesher at level 0 -> <exp_dir>/meshes/<iter>_<res>_tsdf.ply, with the floater removal, normals and colours
    of the density export (mesh.min_component_faces, mesh.normals, mesh.normal_source, mesh.colors)."""
    if dataset is None:
        raise ValueError("mesh.source=tsdf renders the training cameras: it needs the data set")
    import torch
    from . import runtime
    o = options(cfg)
    o.update(tsdf_options(cfg))
    dist = distance_options(cfg)
    tex_on = texture_options(cfg)["texture"]
    cviews = o["colors"] and view_color_options(cfg)["color_source"] == "views"
    sp = o.get("sparse", 0)
    if sp and o["normal_source"] == "grid" and (o["normals"] or o["colors"] or tex_on):
        raise ValueError("tsdf.sparse builds no dense TSDF: mesh.normals, mesh.colors and mesh.texture need mesh.normal_source=field")
    host = runtime.host()
    if sp:
        t = fuse_tsdf_sparse(runner, dataset, scene, o, sp)
        verts, faces = t["verts"], t["faces"]
    else:
        t = fuse_tsdf(runner, dataset, scene, o)
        verts, faces = host.mesh_from_grid_masked(t["g"], t["valid"], t["lo"], t["step"], 0.0)
    if o["min_component_faces"] > 1:
        verts, faces, _ = host.mesh_filter_components(verts, faces, o["min_component_faces"])
    k, faces_in = o["simplify"], len(faces)
    full_verts, full_faces = verts, faces  # (mesh.distance compares with the mesh before the simplification)
    if k >= 2:  # (cell = k * step as ONE float32 product: what extract_mesh_attrs uses)
        verts, faces, _ = host.mesh_simplify(verts, faces, float(np.float32(k) * np.float32(t["step"])), t["lo"])

    def attributes(verts):
        normals = colors = nrm = None
        if (o["normals"] or o["colors"] or tex_on) and len(verts) > 0 and sp:
            nrm = runner.field_normals(verts).contiguous()  # ((0, 0, 0) where the field's gradient vanishes: there is no grid to fall back on)
        elif (o["normals"] or o["colors"] or tex_on) and len(verts) > 0:
            nrm = host.grid_normals(t["g"], verts, t["lo"], t["step"])  # (g is positive inside, as a density is: the same sign)
            if o["normal_source"] == "field":  # the field's own gradient at the vertex; the grid's where that vanishes
                fn = runner.field_normals(verts)
                nrm = torch.where((fn == 0).all(1, keepdim=True), nrm, fn).contiguous()
        if nrm is not None:
            if o["normals"]:
                normals = nrm.cpu().numpy()
            if o["colors"]:  # the radiance AT the vertex seen along the inward normal, as in the density export
                flat = (nrm == 0).all(1, keepdim=True)
                dirs = torch.where(flat, torch.tensor([[0.0, 0.0, -1.0]], device=nrm.device), -nrm).contiguous()
                colors = runner.query_radiance(verts, dirs)[1].cpu().numpy()
        elif o["normals"] or o["colors"]:
            normals = np.zeros((0, 3), np.float32) if o["normals"] else None
            colors = np.zeros((0, 3), np.float32) if o["colors"] else None
        if cviews and nrm is not None:  # the colours the views observed; a vertex none of them sees keeps the radiance colour
            totals = {}
            colors = _colors_from_views(_view_colors_fn(runner, cfg, scene, dataset, t["step"], totals), totals, verts, nrm, colors)
        return nrm, normals, colors

    nrm, normals, colors = attributes(verts)
    path = os.path.join(exp_dir, "meshes", "%d_%d_tsdf%s.ply" % (runner.iter_step, o["resolution"], "_s%d" % k if k >= 2 else ""))
    v = to_world(verts.cpu().numpy(), scene["center"], scene["radius"])
    write_ply(path, v, faces.cpu().numpy(), normals, colors)
    if sp:
        print("Mesh: %d vertices, %d faces%s from the TSDF of %d views (sparse: %d of %d bricks of %d^3 cells active, truncation %g) -> %s" % (
            len(v), len(faces), _simplified(k, faces_in), t["n_views"], t["stats"]["active_bricks"], t["stats"]["bricks"], sp, t["trunc"], path))
    else:
        print("Mesh: %d vertices, %d faces%s from the TSDF of %d views (%d of %d grid points known, truncation %g) -> %s" % (
            len(v), len(faces), _simplified(k, faces_in), t["n_views"], int(t["valid"].sum()), t["valid"].numel(), t["trunc"], path))
    if o["refine"] is not None:  # the smoothing alone: the TSDF surface is no level set of the density
        rf = o["refine"]
        max_move = float(np.float32(rf["max_move_steps"]) * np.float32(t["step"]) * np.float32(k if k >= 2 else 1))
        v0, q0 = verts, host.mesh_face_quality(verts, faces).cpu().numpy()
        if rf["smooth_passes"] > 0:
            verts = host.mesh_smooth(verts, faces, rf["smooth_passes"], rf["lam"], rf["mu"], max_move)
        q1 = host.mesh_face_quality(verts, faces).cpu().numpy()
        moved = (verts.double() - v0.double()).norm(dim=1).cpu().numpy() / float(t["step"])
        fl = faces.long()
        nb = torch.cross(v0.double()[fl[:, 1]] - v0.double()[fl[:, 0]], v0.double()[fl[:, 2]] - v0.double()[fl[:, 0]], dim=1)
        na = torch.cross(verts.double()[fl[:, 1]] - verts.double()[fl[:, 0]], verts.double()[fl[:, 2]] - verts.double()[fl[:, 0]], dim=1)
        edges = host.mesh_ring(faces, len(verts))[3]
        stats = {"smooth_passes": rf["smooth_passes"], "project": 0, "max_move": max_move, "points": len(verts),
                 "moved_median": _lower(moved, 0.5), "moved_p90": _lower(moved, 0.9), "moved_max": _lower(moved, 1.0),
                 "quality_median_before": _lower(q0, 0.5), "quality_p05_before": _lower(q0, 0.05), "quality_median_after": _lower(q1, 0.5),
                 "quality_p05_after": _lower(q1, 0.05), "flipped_faces": int(((nb * na).sum(1) < 0).sum()), "boundary_edges": int(edges[0]),
                 "nonmanifold_edges": int(edges[1])}
        nrm, normals, colors = attributes(verts)
        path = _write_refined(path, scene, verts, faces, normals, colors, stats)
    tex = _run_texture(runner, cfg, scene, verts, faces, nrm, t["step"], path, dataset) if tex_on else None
    if check_options(cfg)["check"]:
        _run_check(runner, cfg, scene, dataset, verts, faces, t["step"], path, tex)
    if dist["distance"] or dist["distance_to"] is not None:
        _distance_in_world(cfg, scene, verts, faces, t["step"], path, (full_verts, full_faces) if dist["distance"] else None)
    return path


def check_options(cfg):
    """mesh.check and the check.* options.  The defaults mirror tsdf.*; none of them is measured on a scene."""
    m = cfg.get("mesh") or {}
    c = cfg.get("check") or {}
    o = {"check": _flag(m.get("check", False)), "res_level": int(c.get("res_level", 4)), "tau": float(c.get("tau", 0.5)),
         "min_opacity": float(c.get("min_opacity", 0.5)), "max_views": int(c.get("max_views", 0))}
    if o["res_level"] < 1 or o["max_views"] < 0 or not 0.0 < o["tau"] <= 1.0 or not o["min_opacity"] >= 0.0:
        raise ValueError("check.res_level must be >= 1, check.max_views >= 0, check.tau in (0, 1] and check.min_opacity >= 0, got %r" % (o,))
    return o


def render_mesh(verts, faces, rays_o, rays_d, bounds=None, accel=None, normals=None, colors=None, uv=None, texture=None):
    """The mesh seen along rays (host.mesh_raycast; accel None: one is built with the default cell): dict of hit [R] bool, t [R],
    face [R] int32 (-1: none), bary [R,3], points (o + t d), face_normals (the unit geometric normal of the hit face, (B - A) x (C - A)),
    facing (-n.d > 0: the ray meets the face's front) and, for per-vertex normals / colors [V,3], their barycentric blend at the hit
    (the normal renormalised).  With uv [F,3,2] and texture [S,S,C] (host.mesh_atlas, runner.bake_texture) two more: uv [R,2], the
    blend of the hit face's three corners' uv, and tex_colors [R,C], host.texture_sample there.  Rows without a hit are zero.
    Everything but the ray cast and the texture lookup is plain torch."""
    import torch
    from . import runtime
    host = runtime.host()
    if accel is None:
        accel = host.mesh_raycast_build(verts, faces)
    t, face, bary = host.mesh_raycast(verts, faces, accel, rays_o, rays_d, bounds)
    hit = face >= 0
    out = {"hit": hit, "t": t, "face": face, "bary": bary}
    R = int(t.shape[0])
    zero3 = torch.zeros((R, 3), dtype=torch.float32, device=t.device)
    if int(faces.shape[0]) == 0 or R == 0:
        out.update(points=zero3, face_normals=zero3.clone(), facing=torch.zeros_like(hit))
        for name, attr in (("normals", normals), ("colors", colors)):
            if attr is not None:
                out[name] = zero3.clone()
        if uv is not None and texture is not None:
            out.update(uv=zero3[:, :2].clone(), tex_colors=torch.zeros((R, int(texture.shape[2])), dtype=torch.float32, device=t.device))
        return out
    v = verts.to(torch.float32).reshape(-1, 3)
    corners = faces.reshape(-1, 3).long()[face.clamp_min(0).long()]  # [R,3]
    P = v[corners]  # [R,3,3]
    n = torch.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], dim=1)
    ln = n.norm(dim=1, keepdim=True)
    n = torch.where(hit[:, None] & (ln > 0), n / ln.clamp_min(1e-38), zero3)
    rd = rays_d.to(torch.float32).reshape(-1, 3)
    out["points"] = torch.where(hit[:, None], rays_o.to(torch.float32).reshape(-1, 3) + t[:, None] * rd, zero3)
    out["face_normals"] = n
    out["facing"] = hit & (-(n * rd).sum(1) > 0)
    for name, attr in (("normals", normals), ("colors", colors)):
        if attr is not None:
            x = (attr.to(torch.float32).reshape(-1, 3)[corners] * bary[:, :, None]).sum(1)
            if name == "normals":
                lx = x.norm(dim=1, keepdim=True)
                x = torch.where(lx > 0, x / lx.clamp_min(1e-38), zero3)
            out[name] = torch.where(hit[:, None], x, zero3)
    if uv is not None and texture is not None:
        at = (uv.to(torch.float32).reshape(-1, 3, 2)[face.clamp_min(0).long()] * bary[:, :, None]).sum(1)
        out["uv"] = torch.where(hit[:, None], at, torch.zeros_like(at)).contiguous()
        tc = host.texture_sample(texture, out["uv"])
        out["tex_colors"] = torch.where(hit[:, None], tc, torch.zeros_like(tc))
    return out


def compare_depth(t_field, has_field, t_mesh, has_mesh, step):
    """Depth of a mesh against the field's along the same rays, a pure function of its tensors: counts n_rays, n_field, n_mesh, n_both;
    completeness = n_both / n_field; extra = the share of rays where only the mesh has a surface; over the rays where both have one,
    e = |t_mesh - t_field| / step (float32): mean, median, p90, max, within_1 / within_2 (the share with e <= 1 / e <= 2).  The quantile q
    is the element min(n - 1, floor(q n)) of the ascending errors: a sort, no interpolation.  Empty classes give 0, never NaN."""
    import torch
    tf, tm = t_field.reshape(-1).to(torch.float32), t_mesh.reshape(-1).to(torch.float32)
    hf, hm = has_field.reshape(-1).bool(), has_mesh.reshape(-1).bool()
    both = hf & hm
    e = torch.sort((tm[both] - tf[both]).abs() / torch.tensor(float(step), dtype=torch.float32, device=tf.device))[0]
    n, nf, nm, nb = int(tf.numel()), int(hf.sum()), int(hm.sum()), int(both.sum())
    share = lambda a, b: float(a) / float(b) if b else 0.0  # noqa: E731
    at = lambda q: float(e[min(nb - 1, int(np.floor(q * nb)))]) if nb else 0.0  # noqa: E731
    return {"n_rays": n, "n_field": nf, "n_mesh": nm, "n_both": nb, "completeness": share(nb, nf), "extra": share(int((hm & ~hf).sum()), n),
            "mean": float(e.double().mean()) if nb else 0.0, "median": at(0.5), "p90": at(0.9), "max": float(e[-1]) if nb else 0.0,
            "within_1": share(int((e <= 1).sum()), nb), "within_2": share(int((e <= 2).sum()), nb)}


def check_mesh(runner, dataset, scene, verts, faces, o, uv=None, texture=None):
    """A mesh (verts, faces in the NORMALISED frame, before to_world) against the field it came from, seen from the training cameras: for
    every checked camera the rays of tsdf_camera_rays at o["res_level"] are rendered (runner.render_geometry: has_field = a surface
    sample with opacity >= o["min_opacity"], t_field = surf_t) and cast at the mesh (render_mesh, the same rays and bounds).  Returns the
    pooled compare_depth statistics in grid steps of o["step"], plus faces_seen (the share of faces that are some checked ray's first
    hit), normal_agreement (the mean |face normal . surface normal| where both have a surface), n_views, n_faces and views (the
    per-view statistics).  With uv and texture (runner.bake_texture) also texture_psnr, -10 log10 of the mean squared difference between
    the texture seen along the ray (render_mesh's tex_colors) and the field's rendered colour over the n_texture_rays rays where both
    have a surface (the mean square floored at 1e-10; 0 without such a ray).  No side effect on training: nothing is drawn, no vote is
    cast, a pending step is flushed first."""
    import torch
    from . import runtime
    host = runtime.host()
    runner.flush()
    views = [int(v) for v in scene["train_set"]]
    if o["max_views"] > 0:
        views = views[:o["max_views"]]
    nf = int(faces.shape[0])
    accel = host.mesh_raycast_build(verts, faces)
    seen = torch.zeros(nf + 1, dtype=torch.bool, device=verts.device)
    pool = {k: [] for k in ("tf", "hf", "tm", "hm", "agree")}
    per_view = []
    tex, sq_err, n_tex = uv is not None and texture is not None, 0.0, 0
    for idx in views:
        ro, rd, b, _, _ = tsdf_camera_rays(dataset, scene["bounds"], idx, int(o["res_level"]))
        g = runner.render_geometry(ro, rd, b, tau=o["tau"])
        hf = (g["surf_idx"] >= 0) & (g["opacity"] >= o["min_opacity"])
        m = render_mesh(verts, faces, ro, rd, b, accel=accel, **(dict(uv=uv, texture=texture) if tex else {}))
        if tex:
            both = hf & m["hit"]
            sq_err += float(((m["tex_colors"][both] - g["colors"][both]).double() ** 2).sum())
            n_tex += int(both.sum())
        seen[torch.where(m["hit"], m["face"], torch.full_like(m["face"], nf)).long()] = True
        agree = (m["face_normals"] * g["surf_normals"]).sum(1).abs()[hf & m["hit"]]
        stats = compare_depth(g["surf_t"], hf, m["t"], m["hit"], o["step"])
        stats["view"] = idx
        stats["normal_agreement"] = float(agree.double().mean()) if agree.numel() else 0.0
        per_view.append(stats)
        for k, x in (("tf", g["surf_t"]), ("hf", hf), ("tm", m["t"]), ("hm", m["hit"]), ("agree", agree)):
            pool[k].append(x)
    cat = lambda k, dt: torch.cat(pool[k]) if pool[k] else torch.zeros(0, dtype=dt, device=verts.device)  # noqa: E731
    out = compare_depth(cat("tf", torch.float32), cat("hf", torch.bool), cat("tm", torch.float32), cat("hm", torch.bool), o["step"])
    agree = cat("agree", torch.float32)
    out.update(faces_seen=float(int(seen[:nf].sum())) / nf if nf else 0.0, normal_agreement=float(agree.double().mean()) if agree.numel() else 0.0,
               n_views=len(views), n_faces=nf, step=float(o["step"]), res_level=int(o["res_level"]), tau=float(o["tau"]),
               min_opacity=float(o["min_opacity"]), views=per_view)
    if tex:
        out.update(texture_psnr=float(-10.0 * np.log10(max(sq_err / (3 * n_tex), 1e-10))) if n_tex else 0.0, n_texture_rays=n_tex)
    return out


def _run_check(runner, cfg, scene, dataset, verts, faces, step, path, tex=None):
    """mesh.check=true: check_mesh of the mesh just written -> <path without .ply>_check.json and one printed line."""
    import json
    if dataset is None:
        raise ValueError("mesh.check=true casts the training cameras' rays at the mesh: it needs the data set")
    o = check_options(cfg)
    o["step"] = float(step)
    res = check_mesh(runner, dataset, scene, verts, faces, o, **(dict(uv=tex["uv"], texture=tex["texture"]) if tex else {}))
    out = path[:-4] + "_check.json"
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print("Check: completeness %.4f, depth error median %.3f / p90 %.3f grid steps, extra %.4f, faces seen %.4f (%d views at 1/%d) -> %s" % (
        res["completeness"], res["median"], res["p90"], res["extra"], res["faces_seen"], res["n_views"], o["res_level"], out))
    return out


TEXTURE_SOURCES = ("point", "ray", "views")


def texture_options(cfg):
    """mesh.texture and the texture.* options.  texels_per_step = 2 and ray_steps = 4 (the TSDF truncation's default) are not measured on
    a scene."""
    m = cfg.get("mesh") or {}
    t = cfg.get("texture") or {}
    src = str(t.get("source", "point")).strip().lower()
    if src not in TEXTURE_SOURCES:
        raise ValueError("texture.source must be one of %s, got %r" % (" | ".join(TEXTURE_SOURCES), t.get("source")))
    o = {"texture": _flag(m.get("texture", False)), "texels_per_step": float(t.get("texels_per_step", 2.0)), "max_size": int(t.get("max_size", 8192)),
         "max_block_log2": int(t.get("max_block_log2", 7)), "source": src, "ray_steps": float(t.get("ray_steps", 4.0))}
    if (not 0.0 < o["texels_per_step"] < float("inf") or not 0.0 < o["ray_steps"] < float("inf") or not 2 <= o["max_block_log2"] <= 13 or
            not 4 <= o["max_size"] <= 8192 or o["max_size"] & (o["max_size"] - 1)):
        raise ValueError("texture.texels_per_step and texture.ray_steps must be > 0 and finite, texture.max_block_log2 in [2, 13] and "
                         "texture.max_size a power of two in [4, 8192], got %r" % (o,))
    return o


BAKE_CHUNK = 1 << 20  # texels per radiance query / rays per render of bake_texture


def bake_texture(runner, verts, faces, normals, density, max_size=8192, max_log=7, source="point", ray_steps=4.0, step=None, view_colors=None):
    """runner.bake_texture: a texture atlas of the mesh (verts, faces, per-vertex normals [V,3] in the NORMALISED frame; density in texels
    per length unit) filled from the field.  host.mesh_atlas lays one right-triangle chart per face into an atlas of at most max_size
    (the density is halved until it fits) and host.mesh_atlas_texels (clamp on) gives every owned texel its point of the surface and
    its weights; the texel's direction is minus the normalised blend of its corners' normals by those weights (the face's geometric
    normal where the blend vanishes, (0, 0, -1) where that vanishes too).  source "point": the colour is
    runner.query_radiance(point, dir)[1], the definition of mesh.colors, so a texel on a vertex carries that vertex's colour;
    source "ray": the volume-rendered colour of runner.render_geometry along the ray from point - h dir in direction dir over (0, 2 h)
    with h = ray_steps * step (step: the grid step of the mesh, required) -- it starts h outside the surface and ends h inside it.
    ray_steps = 4 grid steps is the TSDF truncation's default, not measured on a scene.
    source "views": view_colors(points [T,3], normals [T,3]) -> (rgb [T,3], known [T] bool) (fuse_view_colors through the launcher: the
    colours the training views observed) is called ONCE on the owned texels' points and their blended corner normals (minus the
    direction above); a texel that is not known takes the "point" colour.  Without view_colors it is a ValueError.
    Returns dict of uv [F,3,2], size, texture [S,S,3] (0 where no face owns the texel), tex_face [S,S] int32, density_used, texels_used
    and, for source "views", texels_from_views.  No side effect on training: a pending step is flushed first, nothing is drawn, no vote
    is cast."""
    import torch
    from . import runtime
    host = runtime.host()
    if source not in TEXTURE_SOURCES:
        raise ValueError("bake_texture: source must be one of %s, got %r" % (" | ".join(TEXTURE_SOURCES), source))
    if source == "ray" and not (step is not None and float(step) > 0.0 and float(ray_steps) > 0.0):
        raise ValueError("bake_texture: source='ray' needs the grid step of the mesh (step > 0) and ray_steps > 0")
    if source == "views" and view_colors is None:
        raise ValueError("bake_texture: source='views' needs view_colors, a function (points, normals) -> (rgb, known)")
    runner.flush()
    uv, size, blocks, used = host.mesh_atlas(verts, faces, float(density), int(max_size), int(max_log))
    tex_face, bary, pos = host.mesh_atlas_texels(verts, faces, blocks, size, True)
    texture = torch.zeros((size, size, 3), dtype=torch.float32, device=pos.device)
    own = tex_face.reshape(-1) >= 0
    at = own.nonzero().reshape(-1)
    from_views = 0
    if at.numel():
        corners = faces.reshape(-1, 3).long()[tex_face.reshape(-1)[at].long()]  # [T,3]
        w, p = bary.reshape(-1, 3)[at], pos.reshape(-1, 3)[at].contiguous()
        n = (normals.to(torch.float32).reshape(-1, 3)[corners] * w[:, :, None]).sum(1)
        P = verts.to(torch.float32).reshape(-1, 3)[corners]
        gn = torch.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], dim=1)
        ln, lg = n.norm(dim=1, keepdim=True), gn.norm(dim=1, keepdim=True)
        up = torch.tensor([[0.0, 0.0, 1.0]], device=p.device)
        gn = torch.where((lg > 0) & torch.isfinite(lg), gn / lg.clamp_min(1e-38), up)
        dirs = (-torch.where((ln > 0) & torch.isfinite(ln), n / ln.clamp_min(1e-38), gn)).contiguous()
        cols = []
        for k in range(0, int(at.numel()), BAKE_CHUNK):
            pk, dk = p[k:k + BAKE_CHUNK].contiguous(), dirs[k:k + BAKE_CHUNK].contiguous()
            if source != "ray":
                cols.append(runner.query_radiance(pk, dk)[1])
            else:
                h = float(np.float32(ray_steps) * np.float32(step))
                b = torch.tensor([[0.0, 2.0 * h]], dtype=torch.float32, device=p.device).repeat(len(pk), 1).contiguous()
                cols.append(runner.render_geometry((pk - h * dk).contiguous(), dk, b)["colors"])
        cols = torch.cat(cols)
        if source == "views":
            rgb, known = view_colors(p, (-dirs).contiguous())
            cols = torch.where(known.bool()[:, None], rgb, cols)
            from_views = int(known.sum())
        texture.reshape(-1, 3)[at] = cols
    out = {"uv": uv, "size": int(size), "texture": texture, "tex_face": tex_face, "density_used": float(used), "texels_used": int(at.numel())}
    if source == "views":
        out["texels_from_views"] = from_views
    return out


def write_png(path, rgb_uint8):
    """8-bit RGB PNG of rgb_uint8 [H,W,3] from the standard library alone (zlib, struct): one IDAT, filter 0 on every row."""
    import struct
    import zlib
    a = np.ascontiguousarray(rgb_uint8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: rgb_uint8 must be a uint8 array [H,W,3]")
    h, w = int(a.shape[0]), int(a.shape[1])
    rows = np.zeros((h, 1 + w * 3), np.uint8)
    rows[:, 1:] = a.reshape(h, w * 3)
    chunk = lambda kind, data: struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)  # noqa: E731
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                 chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))
    return path


def write_obj(path, verts, faces, uv, normals=None, texture_name="texture.png"):
    """Wavefront OBJ with a material: `v` lines, `vn` lines when normals [V,3] are given, three `vt` per face (uv [F,3,2] in image
    convention -> vt = (x, 1 - y)), then `f a/ta[/na]` with 1-based indices; <path without .obj>.mtl names texture_name in map_Kd."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    t = np.asarray(uv, np.float32).reshape(-1, 3, 2)
    if len(t) != len(f) or (normals is not None and np.asarray(normals).reshape(-1, 3).shape[0] != len(v)):
        raise ValueError("write_obj: uv must be [F,3,2] and normals [V,3]")
    mtl = path[:-4] + ".mtl" if path.lower().endswith(".obj") else path + ".mtl"
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(mtl, "w") as fh:
        fh.write("newmtl baked\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd %s\n" % texture_name)
    lines = ["mtllib %s" % os.path.basename(mtl)]
    lines += ["v %.9g %.9g %.9g" % tuple(r) for r in v.tolist()]
    if normals is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(r) for r in np.asarray(normals, np.float32).reshape(-1, 3).tolist()]
    t2 = t.reshape(-1, 2)
    lines += ["vt %.9g %.9g" % (x, y) for x, y in zip(t2[:, 0].tolist(), (np.float32(1.0) - t2[:, 1]).tolist())]
    lines.append("usemtl baked")
    for k, (a, b, c) in enumerate(f.tolist()):
        ta = 3 * k + 1
        if normals is not None:
            lines.append("f %d/%d/%d %d/%d/%d %d/%d/%d" % (a + 1, ta, a + 1, b + 1, ta + 1, b + 1, c + 1, ta + 2, c + 1))
        else:
            lines.append("f %d/%d %d/%d %d/%d" % (a + 1, ta, b + 1, ta + 1, c + 1, ta + 2))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return path


def _run_texture(runner, cfg, scene, verts, faces, normals, step, path, dataset=None):
    """mesh.texture=true: runner.bake_texture of the mesh just written -> <path without .ply>_tex.obj / .mtl / .png and one printed line.
    Returns bake_texture's dict (mesh.check reads uv and texture from it)."""
    import torch
    t = texture_options(cfg)
    base = path[:-4] + "_tex"
    density = float(np.float32(t["texels_per_step"]) / np.float32(step))
    if normals is None:
        normals = torch.zeros((int(verts.shape[0]), 3), dtype=torch.float32, device=verts.device)
    views = {"view_colors": _view_colors_fn(runner, cfg, scene, dataset, step)} if t["source"] == "views" else {}
    r = runner.bake_texture(verts, faces, normals, density, t["max_size"], t["max_block_log2"], t["source"], t["ray_steps"], step, **views)
    write_png(base + ".png", quantize_colors(r["texture"].cpu().numpy()))
    write_obj(base + ".obj", to_world(verts.cpu().numpy(), scene["center"], scene["radius"]), faces.cpu().numpy(), r["uv"].cpu().numpy(),
              normals.cpu().numpy(), os.path.basename(base + ".png"))
    halved = "" if r["density_used"] == density else " (halved from %g to fit texture.max_size=%d)" % (density, t["max_size"])
    print("Texture: atlas %d x %d, %d texels used, %g texels per unit%s, source %s -> %s" % (
        r["size"], r["size"], r["texels_used"], r["density_used"], halved,
        t["source"] + (" (%d texels from views)" % r["texels_from_views"] if t["source"] == "views" else ""), base + ".obj"))
    return r


def read_ply(path):
    """(verts [V,3] float32, faces [F,3] int32) of a triangle-mesh PLY: what write_ply writes (further vertex properties are skipped), and
    ASCII / binary_little_endian files with float x, y, z and a face list `vertex_indices` or `vertex_index` of three entries each.
    ValueError for anything else: another format, further elements, a face that is no triangle, a truncated file."""
    scalar = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
              "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("read_ply: %s is not a PLY file" % path)
    body = data[end + len(b"end_header\n"):]
    fmt, elements = None, []
    for ln in data[:end].decode("ascii", "replace").replace("\r", "").split("\n")[1:]:
        w = ln.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format" and len(w) == 3:
            fmt = w[1]
        elif w[0] == "element" and len(w) == 3:
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements and len(w) in (3, 5):
            elements[-1][2].append(w[1:])
        else:
            raise ValueError("read_ply: header line %r" % ln)
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("read_ply: format %r (ascii and binary_little_endian are read)" % fmt)
    if [e[0] for e in elements] not in (["vertex", "face"], ["vertex"]):
        raise ValueError("read_ply: elements %r (a vertex element, then a face element)" % [e[0] for e in elements])
    nv, vprops = elements[0][1], elements[0][2]
    if any(len(p) != 2 or p[0] not in scalar for p in vprops):
        raise ValueError("read_ply: a vertex property is a list or of an unknown type")
    names = [p[1] for p in vprops]
    if any(names.count(k) != 1 or scalar[vprops[names.index(k)][0]] != "<f4" for k in ("x", "y", "z")):
        raise ValueError("read_ply: the vertex element needs float x, y and z")
    nf, fprops = (elements[1][1], elements[1][2]) if len(elements) > 1 else (0, [])
    if nf or fprops:
        if (len(fprops) != 1 or len(fprops[0]) != 4 or fprops[0][0] != "list" or fprops[0][3] not in ("vertex_indices", "vertex_index") or
                scalar.get(fprops[0][1], "<f4")[-2] not in "iu" or scalar.get(fprops[0][2], "<f4")[-2] not in "iu"):
            raise ValueError("read_ply: the face element must be one integer list vertex_indices / vertex_index")
    if fmt == "ascii":
        tok = body.split()
        need = nv * len(vprops)
        if len(tok) != need + 4 * nf:
            raise ValueError("read_ply: %d values for %d vertices and %d triangles (a face that is no triangle?)" % (len(tok), nv, nf))
        try:
            vt = np.array(tok[:need], dtype=np.float64).reshape(nv, len(vprops))
            ft = np.array(tok[need:], dtype=np.int64).reshape(nf, 4)
        except ValueError:
            raise ValueError("read_ply: a value of the body is not a number")
        verts = np.stack([vt[:, names.index(k)] for k in ("x", "y", "z")], 1).astype(np.float32)
        count, idx = ft[:, 0], ft[:, 1:]
    else:
        vdt = np.dtype([(p[1], scalar[p[0]]) for p in vprops])
        fdt = np.dtype([("n", scalar[fprops[0][1]]), ("idx", scalar[fprops[0][2]], (3,))]) if nf else np.dtype([("n", "u1"), ("idx", "<i4", (3,))])
        if len(body) != nv * vdt.itemsize + nf * fdt.itemsize:
            raise ValueError("read_ply: the body holds %d bytes, %d vertices and %d triangles need %d (a face that is no triangle?)" % (
                len(body), nv, nf, nv * vdt.itemsize + nf * fdt.itemsize))
        vrec = np.frombuffer(body, vdt, nv)
        frec = np.frombuffer(body, fdt, nf, nv * vdt.itemsize)
        verts = np.stack([vrec[k] for k in ("x", "y", "z")], 1).astype(np.float32)
        count, idx = frec["n"].astype(np.int64), frec["idx"].astype(np.int64)
    if (count != 3).any():
        raise ValueError("read_ply: a face that is no triangle")
    if nf and (idx.min() < 0 or idx.max() >= max(nv, 1) or idx.max() > 2 ** 31 - 1):
        raise ValueError("read_ply: a face names a vertex that is not there")
    return np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(idx, np.int32).reshape(-1, 3)


def distance_options(cfg):
    """mesh.distance, mesh.distance_to and the distance.* options.  200 000 samples per side and thresholds of 0.5, 1 and 2 grid steps are
    choices, not measurements.  mesh.distance=true needs something to compare with: mesh.simplify >= 2 (the unsimplified mesh); a
    mesh.distance_to=<file.ply> compares with that file instead, and the two exclude each other (one JSON per mesh)."""
    m = cfg.get("mesh") or {}
    d = cfg.get("distance") or {}
    to = m.get("distance_to", None)
    to = None if to is None or str(to).strip() == "" else str(to)
    th = d.get("thresholds", [0.5, 1.0, 2.0])
    if isinstance(th, str):
        th = [x for x in th.strip("[]() ").split(",") if x.strip()]
    elif not isinstance(th, (list, tuple)) and not hasattr(th, "__iter__"):
        th = [th]
    md = d.get("max_dist_steps", None)
    o = {"distance": _flag(m.get("distance", False)), "distance_to": to, "samples": int(d.get("samples", 200000)), "seed": int(d.get("seed", 0)),
         "thresholds": [float(x) for x in th], "max_dist_steps": None if md is None else float(md)}
    if (o["samples"] < 1 or o["samples"] >= 2 ** 31 or o["seed"] < 0 or not o["thresholds"] or
            any(not 0.0 < t < float("inf") for t in o["thresholds"]) or (o["max_dist_steps"] is not None and not o["max_dist_steps"] > 0.0)):
        raise ValueError("distance.samples must lie in [1, 2^31), distance.seed be >= 0, distance.thresholds a list of positive finite "
                         "numbers and distance.max_dist_steps > 0, got %r" % (o,))
    if o["distance"] and o["distance_to"] is not None:
        raise ValueError("mesh.distance=true (against the unsimplified mesh) and mesh.distance_to=<file> write the same JSON: choose one")
    if o["distance"] and _simplify(m.get("simplify", 0)) < 2:
        raise ValueError("mesh.distance=true compares the simplified mesh with the unsimplified one: it needs mesh.simplify >= 2 (or "
                         "mesh.distance_to=<file.ply> instead)")
    return o


class _HostDistance:
    """the device primitives of mesh_distance on torch tensors (runtime.host())"""
    def __init__(self):
        from . import runtime
        self.host = runtime.host()

    def _dev(self, verts, faces):
        import torch
        v = torch.as_tensor(np.asarray(verts, np.float32) if not torch.is_tensor(verts) else verts).to("cuda", torch.float32).reshape(-1, 3)
        f = torch.as_tensor(np.asarray(faces, np.int32) if not torch.is_tensor(faces) else faces).to("cuda", torch.int32).reshape(-1, 3)
        return v.contiguous(), f.contiguous()

    def sample(self, verts, faces, n, seed):
        return self.host.mesh_sample_surface(*self._dev(verts, faces), int(n), int(seed))[0]

    def distances(self, verts, faces, points, max_dist):
        v, f = self._dev(verts, faces)
        accel = self.host.mesh_raycast_build(v, f)
        return self.host.mesh_closest_point(v, f, accel, points, float(max_dist))[0].cpu().numpy()


def _direction(dist, unit, thresholds):
    """the statistics of one direction from its samples' distances [n] (+inf: missed), in units of `unit`; the quantile q is the element
    min(m - 1, floor(q m)) of the m ascending distances that are not missed: a sort, no interpolation.  No sample within max_dist: zeros."""
    d = np.asarray(dist, np.float32).reshape(-1)
    got = np.isfinite(d)
    e = np.sort(d[got].astype(np.float64) / float(unit))
    m = len(e)
    at = lambda q: float(e[min(m - 1, int(np.floor(q * m)))]) if m else 0.0  # noqa: E731
    stats = {"n": int(len(d)), "missed": int(len(d) - m), "mean": float(e.mean()) if m else 0.0, "rms": float(np.sqrt((e * e).mean())) if m else 0.0,
             "median": at(0.5), "p90": at(0.9), "p95": at(0.95), "max": float(e[-1]) if m else 0.0}
    within = [float((e <= t).sum()) / len(d) if len(d) else 0.0 for t in thresholds]  # (a missed sample is within no threshold)
    return stats, within


def mesh_distance(verts_a, faces_a, verts_b, faces_b, n=200000, seed=0, thresholds=(0.5, 1.0, 2.0), unit=1.0, max_dist=None, backend=None):
    """The distance between two triangle meshes in the same frame, sampled: n area-uniform, stratified points of each surface
    (host.mesh_sample_surface, a pure function of (mesh, n, seed)) and the distance of each to the closest point of the OTHER mesh
    (host.mesh_closest_point over host.mesh_raycast_build's grid).  Returns a dict of
      a_to_b, b_to_a   n, missed (samples farther than max_dist: counted, left out of the statistics), and over the others mean, rms, median,
                       p90, p95, max -- a_to_b is measured at the samples of A (how far A strays from B: accuracy when B is the
                       truth), b_to_a at those of B (what of B is missing in A: completeness)
      chamfer          the mean of the two means
      hausdorff        the larger of the two maxima: a SAMPLED estimate, taken at the sample points only and therefore a lower bound of the
                       true Hausdorff distance, which sits at one point of one surface and which no finite sample is sure to hit
      thresholds, precision, recall, fscore   per threshold t: the share of A's samples within t of B, of B's within t of A, and their
                       harmonic mean (0 where both are 0); a missed sample is within no threshold
      unit, seed, n_faces_a, n_faces_b, max_dist
    All lengths are divided by `unit` (the launcher passes the grid step, so that they read in grid steps); max_dist (None: no cut-off)
    is in the meshes' own units.  n = 200 000 per side and thresholds of 0.5, 1 and 2 units are choices, not measurements.  Nothing
    depends on the schedule: the same call gives the same dict.  backend: an object with sample(verts, faces, n, seed) -> points and
    distances(verts, faces, points, max_dist) -> numpy [N] (the tests drive the emulated library through it); None: the device."""
    if not (float(unit) > 0.0 and float(unit) < float("inf")) or int(n) < 1 or (max_dist is not None and not float(max_dist) >= 0.0):
        raise ValueError("mesh_distance: unit must be positive and finite, n >= 1 and max_dist >= 0")
    th = [float(t) for t in thresholds]
    be = backend if backend is not None else _HostDistance()
    md = float("inf") if max_dist is None else float(max_dist)
    pa, pb = be.sample(verts_a, faces_a, n, seed), be.sample(verts_b, faces_b, n, seed)
    ab, p = _direction(be.distances(verts_b, faces_b, pa, md), unit, th)
    ba, r = _direction(be.distances(verts_a, faces_a, pb, md), unit, th)
    return {"a_to_b": ab, "b_to_a": ba, "chamfer": 0.5 * (ab["mean"] + ba["mean"]), "hausdorff": max(ab["max"], ba["max"]), "thresholds": th,
            "precision": p, "recall": r, "fscore": [2.0 * x * y / (x + y) if x + y > 0.0 else 0.0 for x, y in zip(p, r)],
            "unit": float(unit), "seed": int(seed), "n_faces_a": int(np.shape(faces_a)[0]), "n_faces_b": int(np.shape(faces_b)[0]),
            "max_dist": None if max_dist is None else float(max_dist)}


def _run_distance(cfg, verts, faces, ref_verts, ref_faces, unit, against, path):
    """mesh_distance(the mesh just written, the other mesh) -> <path without .ply>_distance.json and one printed line, lengths in grid
    steps (`unit`: the grid step in the frame of the vertices)."""
    import json
    d = distance_options(cfg)
    md = None if d["max_dist_steps"] is None else float(d["max_dist_steps"]) * float(unit)
    res = mesh_distance(verts, faces, ref_verts, ref_faces, n=d["samples"], seed=d["seed"], thresholds=d["thresholds"], unit=unit, max_dist=md)
    res["against"] = against
    out = path[:-4] + "_distance.json"
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print("Distance: to %s, chamfer %.4f, p95 %.4f / %.4f (this mesh to the other / back), hausdorff %.4f grid steps, F-score %s -> %s" % (
        against, res["chamfer"], res["a_to_b"]["p95"], res["b_to_a"]["p95"], res["hausdorff"],
        ", ".join("%.4f at %g" % (f, t) for f, t in zip(res["fscore"], res["thresholds"])), out))
    return out


def _distance_in_world(cfg, scene, verts, faces, step, path, full=None):
    """mesh.distance / mesh.distance_to: the mesh just written (verts, faces: device tensors in the NORMALISED frame) against the
    unsimplified one (full = (verts, faces) likewise) or against the file of mesh.distance_to.  Both comparisons are made in the data
    set's WORLD frame, on the float32 vertices a .ply carries (a grid step there is step * radius): mesh.distance_to=<the same run's
    unsimplified .ply> therefore reproduces the figures of mesh.distance=true."""
    d = distance_options(cfg)
    world = lambda x: to_world(x.cpu().numpy(), scene["center"], scene["radius"])  # noqa: E731
    if full is not None:
        rv, rf, against = world(full[0]), full[1].cpu().numpy(), "unsimplified"
    else:
        (rv, rf), against = read_ply(d["distance_to"]), d["distance_to"]
    return _run_distance(cfg, world(verts), faces.cpu().numpy(), rv, rf, float(np.float32(step) * np.float32(scene["radius"])), against, path)


def _bricks(B, stats):
    return " (sparse: %d of %d bricks of %d^3 cells active)" % (stats["active_bricks"], stats["bricks"], B)


def _simplified(k, faces_in):
    return " (simplified from %d faces, mesh.simplify=%d)" % (faces_in, k) if k >= 2 else ""


def extract(runner, cfg, scene, exp_dir, dataset=None):
    """Density grid -> iso-surface -> <exp_dir>/meshes/<iter>_<res>.ply, vertices in the data set's world frame (mesh.source=tsdf:
    extract_tsdf, which needs the data set)."""
    o = options(cfg)
    dist = distance_options(cfg)
    sp = o["sparse"]
    if sp and o["source"] == "tsdf":
        raise ValueError("mesh.sparse with mesh.source=tsdf: mesh.sparse culls by the octree; the sparse TSDF fusion is tsdf.sparse")
    if sp and o["normal_source"] == "grid" and (o["normals"] or o["colors"] or texture_options(cfg)["texture"]):
        raise ValueError("mesh.sparse builds no dense grid: mesh.normals, mesh.colors and mesh.texture need mesh.normal_source=field")
    if o["source"] == "tsdf":
        return extract_tsdf(runner, cfg, scene, dataset, exp_dir)
    sparse = {"sparse": sp} if sp else {}  # (what every extract_mesh_attrs call below passes on)
    cviews = o["colors"] and view_color_options(cfg)["color_source"] == "views"
    totals = {}
    if cviews:  # (the facing test wants the normals whether or not the .ply carries them)
        from . import runtime
        vstep = runtime.host().grid_spec([float(x) for x in o["bbox_min"]], [float(x) for x in o["bbox_max"]], int(o["resolution"]),
                                         8192 if sp else 1024)[0]
        vfn = _view_colors_fn(runner, cfg, scene, dataset, vstep, totals)

    def vertex_colors(m):
        if not o["colors"]:
            return None
        colors = m["colors"].cpu().numpy()
        return _colors_from_views(vfn, totals, m["verts"], m["normals"], colors) if cviews and len(colors) else colors
    bricks = ""
    k, faces_in = o["simplify"], 0
    path = os.path.join(exp_dir, "meshes", "%d_%d%s.ply" % (runner.iter_step, o["resolution"], "_s%d" % k if k >= 2 else ""))
    if not (o["normals"] or o["colors"] or o["min_component_faces"] > 1 or k >= 2):
        if sp:
            m = runner.extract_mesh_sparse(o["bbox_min"], o["bbox_max"], o["resolution"], o["level"], sp)
            verts, faces, bricks = m["verts"], m["faces"], _bricks(sp, m["stats"])
        else:
            verts, faces = runner.extract_mesh(o["bbox_min"], o["bbox_max"], o["resolution"], o["level"])
        v = to_world(verts.cpu().numpy(), scene["center"], scene["radius"])
        write_ply(path, v, faces.cpu().numpy())
    else:
        m = runner.extract_mesh_attrs(o["bbox_min"], o["bbox_max"], o["resolution"], o["level"], o["min_component_faces"],
                                      o["normals"] or cviews, o["colors"], o["normal_source"], *((k,) if k >= 2 else ()), **sparse)
        verts, faces, faces_in = m["verts"], m["faces"], m.get("faces_in", 0)
        bricks = _bricks(sp, m["sparse"]) if sp else ""
        v = to_world(verts.cpu().numpy(), scene["center"], scene["radius"])
        # (the world frame is a uniform scale and a shift of the normalised one: normals are the same in both)
        write_ply(path, v, faces.cpu().numpy(), m["normals"].cpu().numpy() if o["normals"] else None, vertex_colors(m))
    print("Mesh: %d vertices, %d faces%s at level %g%s -> %s" % (len(v), len(faces), _simplified(k, faces_in), o["level"], bricks, path))
    refine = {} if o["refine"] is None else {"refine": o["refine"]}  # (what every later extract_mesh_attrs call passes on)
    if refine:  # the unrefined file stands as it is; everything below works on the refined mesh
        m = runner.extract_mesh_attrs(o["bbox_min"], o["bbox_max"], o["resolution"], o["level"], o["min_component_faces"],
                                      o["normals"] or cviews, o["colors"], o["normal_source"], k if k >= 2 else 0, **refine, **sparse)
        verts, faces = m["verts"], m["faces"]
        path = _write_refined(path, scene, verts, faces, m["normals"].cpu().numpy() if o["normals"] else None, vertex_colors(m),
                              dict(m["refine"]))
    tex = None
    if texture_options(cfg)["texture"] or check_options(cfg)["check"] or dist["distance"] or dist["distance_to"] is not None:
        from . import runtime
        step = runtime.host().grid_spec([float(x) for x in o["bbox_min"]], [float(x) for x in o["bbox_max"]], int(o["resolution"]),
                                        8192 if sp else 1024)[0]
    if texture_options(cfg)["texture"]:  # the normals are computed for the texture whether or not the .ply carries them
        m = runner.extract_mesh_attrs(o["bbox_min"], o["bbox_max"], o["resolution"], o["level"], o["min_component_faces"], True, False,
                                      o["normal_source"], *((k,) if k >= 2 or refine else ()), **refine, **sparse)
        verts, faces = m["verts"], m["faces"]
        tex = _run_texture(runner, cfg, scene, verts, faces, m["normals"], step, path, dataset)
    if check_options(cfg)["check"]:
        _run_check(runner, cfg, scene, dataset, verts, faces, step, path, tex)
    if dist["distance"]:  # the same floater filter, extracted once more without the simplification (as the texture path re-extracts)
        full = runner.extract_mesh_attrs(o["bbox_min"], o["bbox_max"], o["resolution"], o["level"], o["min_component_faces"], False, False,
                                         o["normal_source"], **({"simplify": 0, **refine} if refine else {}), **sparse)
        _distance_in_world(cfg, scene, verts, faces, step, path, (full["verts"], full["faces"]))
    elif dist["distance_to"] is not None:
        _distance_in_world(cfg, scene, verts, faces, step, path)
    return path
