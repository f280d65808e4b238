// pybind11 surface of the C++/LibTorch host layer (used by bench.py, __graft_entry__.smoke() and the
// end-to-end tests).  Thin: object lifetime + tensor hand-over only.
#include <torch/extension.h>

#include "DataParallel.h"
#include "ExpRunner.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>

using namespace f2n;

namespace {

Hash3DAnchored* FieldOf(ExpRunner& r) { return static_cast<Hash3DAnchored*>(r.renderer_->scene_field_.get()); }
SHShader* ShaderOf(ExpRunner& r) { return static_cast<SHShader*>(r.renderer_->shader_.get()); }
PersSampler* SamplerOf(ExpRunner& r) { return static_cast<PersSampler*>(r.renderer_->pts_sampler_.get()); }

int g_scatter_producer = 1;  // what f2n_set_scatter_producer was last given (the library keeps it per process, not per runner)

// the runner in validation mode for the length of an inference call (as ExpRunner::RenderGeometry), put back on every exit path
struct InferenceMode {
  GlobalDataPool* gdp;
  RunningMode prev;
  InferenceMode(ExpRunner& r, bool on) : gdp(r.global_data_pool_.get()), prev(gdp->mode_) {
    if (on) gdp->mode_ = RunningMode::VALIDATE;
  }
  ~InferenceMode() { gdp->mode_ = prev; }
};

py::dict StatsToDict(const TrainStats& s) {
  py::dict d;
  d["loss"] = s.loss;
  d["mse"] = s.mse;
  d["n_rays"] = s.n_rays;
  d["n_samples"] = s.n_samples;
  d["n_meaningful"] = s.n_meaningful;
  d["skipped_nan"] = s.skipped_nan;
  return d;
}

}  // namespace

// the ABI version this host layer was compiled against (include/f2n_abi.h); a kernel library of another version next to it
// means one of the two was not rebuilt -- calls would pass the wrong argument lists (observed once: a memory fault)
#define F2N_HOST_EXPECTS_ABI 13

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "f2-nerf hot path: C++/LibTorch host layer over libf2n_hip.so";
  TORCH_CHECK(f2n_abi_version() == F2N_HOST_EXPECTS_ABI, "libf2n_hip reports ABI version ", f2n_abi_version(), ", this host extension was built for ",
              F2N_HOST_EXPECTS_ABI, ": rebuild both (python -c 'import __graft_entry__ as g; g.build()')");
  m.attr("abi_version") = F2N_HOST_EXPECTS_ABI;
  auto bounded = [](const BoundedRays& r) { return std::vector<Tensor>{r.origins, r.dirs, r.bounds}; };
  auto sparse_stats = [](const SparseMeshStats& s) {  // (Renderer::ExtractMeshSparse)
    py::dict d;
    d["bricks"] = s.bricks; d["active_bricks"] = s.active_bricks; d["meshed_bricks"] = s.meshed_bricks;
    d["points_evaluated"] = s.points_evaluated; d["points_nonempty"] = s.points_nonempty; d["batches"] = s.batches;
    d["grid"] = py::make_tuple(s.grid[0], s.grid[1], s.grid[2]);
    return d;
  };
  auto ray_data = [](const std::tuple<BoundedRays, Tensor, Tensor>& t) {
    const auto& r = std::get<0>(t);
    return std::vector<Tensor>{r.origins, r.dirs, r.bounds, std::get<1>(t), std::get<2>(t)};  // + gt colours, image index
  };
  // octree / warp construction from cameras: byte blobs in the reference's checkpoint layout
  m.def("build_octree",
        [](const Tensor& c2w, const Tensor& intri, const Tensor& bounds, int max_depth, float bbox_side_len, float split_dist_thres,
           int n_rand_pts) {
          OctreeBuildResult r = BuildPersOctree(c2w, intri, bounds, max_depth, bbox_side_len, split_dist_thres, n_rand_pts);
          auto blob = [](const void* p, size_t bytes) {
            Tensor t = torch::empty({(int64_t) bytes}, CpuU8());
            if (bytes) std::memcpy(t.data_ptr(), p, bytes);
            return t;
          };
          py::dict d;
          d["tree_nodes"] = blob(r.nodes.data(), r.nodes.size() * sizeof(TreeNode));
          d["pers_trans"] = blob(r.trans.data(), r.trans.size() * sizeof(TransInfo));
          d["edge_pool"] = blob(r.edges.data(), r.edges.size() * sizeof(EdgePool));
          d["n_volumes"] = (int) r.trans.size();
          return d;
        },
        py::arg("c2w"), py::arg("intri"), py::arg("bounds"), py::arg("max_depth"), py::arg("bbox_side_len"),
        py::arg("split_dist_thres"), py::arg("n_rand_pts") = 32 * 32 * 32);
  m.def("construct_trans", [](const Tensor& rand_pts, const Tensor& c2w_vis, const Tensor& intri0, const Tensor& center, int first_cam) {
    TransInfo t = ConstructTrans(rand_pts, c2w_vis, intri0, center, first_cam);
    Tensor out = torch::empty({(int64_t) sizeof(TransInfo)}, CpuU8());
    std::memcpy(out.data_ptr(), &t, sizeof(TransInfo));
    return out;
  });
  m.def("construct_edge_pool", [](const Tensor& tree_nodes_bytes) {
    Tensor b = tree_nodes_bytes.to(torch::kCPU).contiguous();
    std::vector<TreeNode> nodes(b.numel() / sizeof(TreeNode));
    std::memcpy((void*) nodes.data(), b.data_ptr(), nodes.size() * sizeof(TreeNode));
    auto e = ConstructEdgePool(nodes);
    Tensor out = torch::empty({(int64_t) (e.size() * sizeof(EdgePool))}, CpuU8());
    if (!e.empty()) std::memcpy(out.data_ptr(), e.data(), e.size() * sizeof(EdgePool));
    return out;
  });
  py::class_<Dataset>(m, "Dataset")
      .def(py::init<const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, int, int, const std::vector<int>&,
                    const std::vector<int>&, const std::vector<int>&>(),
           py::arg("poses"), py::arg("intri"), py::arg("dist_params"), py::arg("bounds"), py::arg("images"), py::arg("height"),
           py::arg("width"), py::arg("train_set"), py::arg("test_set"), py::arg("val_set"))
      .def("img2world_ray_flex", [](Dataset& d, const Tensor& cam, const Tensor& ij) { auto r = d.Img2WorldRayFlex(cam, ij); return std::vector<Tensor>{r.origins, r.dirs}; })
      .def("gather_colors", &Dataset::GatherColors)
      .def("rays_of_camera", [bounded](Dataset& d, int idx) { return bounded(d.RaysOfCamera(idx)); })
      .def("rays_from_pose", [bounded](Dataset& d, const Tensor& pose, int reso) { return bounded(d.RaysFromPose(pose, reso)); },
           py::arg("pose"), py::arg("reso_level") = 1)
      .def("rand_rays_from_pose", [bounded](Dataset& d, int n, const Tensor& pose) { return bounded(d.RandRaysFromPose(n, pose)); })
      .def("rand_rays_whole_space", [bounded](Dataset& d, int n) { return bounded(d.RandRaysWholeSpace(n)); })
      .def("rand_rays_data", [ray_data](Dataset& d, int n, int sets, int64_t seq) { return ray_data(d.RandRaysData(n, sets, seq)); },
           py::arg("batch_size"), py::arg("sets") = DATA_TRAIN_SET, py::arg("seq") = -1)
      .def("rand_rays_data_of_camera", [ray_data](Dataset& d, int idx, int n) { return ray_data(d.RandRaysDataOfCamera(idx, n)); })
      .def_static("pose_interpolate", &PoseInterpolate)
      .def_readonly("last_cam_indices", &Dataset::last_cam_indices_)
      .def_readonly("last_ij", &Dataset::last_ij_)
      .def_readonly("n_images", &Dataset::n_images_)
      .def_readonly("height", &Dataset::height_)
      .def_readonly("width", &Dataset::width_);
  // the implicit grid of ExpRunner.density_grid: (step, nx, ny, nz), point (ix, iy, iz) = lo + step * i (no device needed)
  m.def("grid_spec", [](const std::vector<float>& lo, const std::vector<float>& hi, int res, int max_res) {
    GridSpec s = Renderer::MakeGridSpec(lo, hi, res, max_res);
    return py::make_tuple(s.step, s.n[0], s.n[1], s.n[2]);
  }, py::arg("lo"), py::arg("hi"), py::arg("res"), py::arg("max_res") = 1024);  // (8192: the virtual grid of extract_mesh_sparse)
  // sparse meshing on bricks of B^3 cells of the virtual grid (lo, step, n = (nx, ny, nz)): flags [nbz, nby, nbx] uint8 of the bricks
  // that can hold a non-empty point (f2n_brick_mark; tree_nodes = the octree records as uint8) ...
  m.def("brick_mark",
        [](const Tensor& tree_nodes, const std::vector<float>& lo, float step, const std::vector<int>& n, int B) {
          if (lo.size() != 3 || n.size() != 3) throw std::invalid_argument("lo and n must have three entries");
          return BrickMark(tree_nodes, lo.data(), step, n.data(), B);
        },
        py::arg("tree_nodes"), py::arg("lo"), py::arg("step"), py::arg("n"), py::arg("B"));
  // ... and (verts, faces) of values [n_bricks, (B+1)^3] for brick_ids [n_bricks] (f2n_brick_mesh_count / _emit, sorted by key): the
  // bits of mesh_from_grid on the dense grid when the list holds every brick with a value on either side of the level
  m.def("mesh_from_bricks",
        [](const Tensor& values, const Tensor& brick_ids, const std::vector<int>& n, const std::vector<float>& lo, float step, float level, int B,
           int64_t batch_bricks) {
          if (lo.size() != 3 || n.size() != 3) throw std::invalid_argument("lo and n must have three entries");
          auto t = MeshFromBricks(values, brick_ids, n.data(), lo.data(), step, level, B, batch_bricks);
          return std::vector<Tensor>{std::get<0>(t), std::get<1>(t)};
        },
        py::arg("values"), py::arg("brick_ids"), py::arg("n"), py::arg("lo"), py::arg("step"), py::arg("level"), py::arg("B"),
        py::arg("batch_bricks") = 0);
  // iso-surface of any float32 grid [nz, ny, nx] by marching tetrahedra (f2n_mesh_count / f2n_mesh_emit): (verts, faces)
  m.def("mesh_from_grid",
        [](const Tensor& grid, float level, const std::vector<float>& lo, float step) {
          TORCH_CHECK(lo.size() == 3, "lo must have three coordinates");
          auto t = MeshFromGrid(grid, level, lo.data(), step);
          return std::vector<Tensor>{std::get<0>(t), std::get<1>(t)};
        },
        py::arg("grid"), py::arg("level"), py::arg("lo") = std::vector<float>{0.f, 0.f, 0.f}, py::arg("step") = 1.f);
  // the same with a uint8 mask [nz, ny, nx] of the grid points that carry a value (f2n_mesh_count_masked / f2n_mesh_emit)
  m.def("mesh_from_grid_masked",
        [](const Tensor& grid, const Tensor& valid, const std::vector<float>& lo, float step, float level) {
          TORCH_CHECK(lo.size() == 3, "lo must have three coordinates");
          auto t = MeshFromGridMasked(grid, valid, level, lo.data(), step);
          return std::vector<Tensor>{std::get<0>(t), std::get<1>(t)};
        },
        py::arg("grid"), py::arg("valid"), py::arg("lo") = std::vector<float>{0.f, 0.f, 0.f}, py::arg("step") = 1.f, py::arg("level") = 0.f);
  // TSDF fusion on any grid: depth maps [V,h,w] (conf [V,h,w] or None) into the running sums S, W [nz, ny, nx], in place
  // (f2n_tsdf_integrate); then (g, valid) of the sums (f2n_tsdf_finalize)
  m.def("tsdf_integrate",
        [](const Tensor& S, const Tensor& W, const std::vector<float>& lo, float step, const Tensor& poses, const Tensor& intri,
           const Tensor& dist, const Tensor& depth, const c10::optional<Tensor>& conf, float trunc) {
          TORCH_CHECK(lo.size() == 3, "lo must have three coordinates");
          TsdfIntegrate(S, W, lo.data(), step, poses, intri, dist, depth, conf.has_value() ? *conf : Tensor(), trunc);
        },
        py::arg("S"), py::arg("W"), py::arg("lo"), py::arg("step"), py::arg("poses"), py::arg("intri"), py::arg("dist"), py::arg("depth"),
        py::arg("conf"), py::arg("trunc"));
  m.def("tsdf_finalize",
        [](const Tensor& S, const Tensor& W, float min_weight) {
          auto t = TsdfFinalize(S, W, min_weight);
          return std::vector<Tensor>{std::get<0>(t), std::get<1>(t)};
        },
        py::arg("S"), py::arg("W"), py::arg("min_weight"));
  // view-colour fusion: the views' observations (depth, conf or None, image [V,h,w,C]) of points [n,3] (normals [n,3] or None) added to
  // the running sums acc [n,C], wsum [n], count [n] int32, in place (f2n_view_colors_accumulate); then (rgb, known) of the sums
  // (f2n_view_colors_finalize)
  m.def("view_colors_accumulate",
        [](const Tensor& acc, const Tensor& wsum, const Tensor& count, const Tensor& points, const c10::optional<Tensor>& normals,
           const Tensor& poses, const Tensor& intri, const Tensor& dist, const Tensor& depth, const c10::optional<Tensor>& conf,
           const Tensor& image, float tol, float cos_min) {
          ViewColorsAccumulate(acc, wsum, count, points, normals.has_value() ? *normals : Tensor(), poses, intri, dist, depth,
                               conf.has_value() ? *conf : Tensor(), image, tol, cos_min);
        },
        py::arg("acc"), py::arg("wsum"), py::arg("count"), py::arg("points"), py::arg("normals"), py::arg("poses"), py::arg("intri"),
        py::arg("dist"), py::arg("depth"), py::arg("conf"), py::arg("image"), py::arg("tol"), py::arg("cos_min"));
  m.def("view_colors_finalize",
        [](const Tensor& acc, const Tensor& wsum, const Tensor& count, int min_views) {
          auto t = ViewColorsFinalize(acc, wsum, count, min_views);
          return std::vector<Tensor>{std::get<0>(t), std::get<1>(t)};
        },
        py::arg("acc"), py::arg("wsum"), py::arg("count"), py::arg("min_views"));
  // sparse TSDF fusion on bricks of B^3 cells of the virtual grid (lo, step, n = (nx, ny, nz)); the views as tsdf_integrate takes them:
  // flags [nbz, nby, nbx] uint8 of the bricks whose row holds a corner seen at most trunc behind a view's surface (f2n_tsdf_brick_mark) ...
  m.def("tsdf_brick_mark",
        [](const std::vector<float>& lo, float step, const std::vector<int>& n, int B, const Tensor& poses, const Tensor& intri,
           const Tensor& dist, const Tensor& depth, const c10::optional<Tensor>& conf, float trunc) {
          if (lo.size() != 3 || n.size() != 3) throw std::invalid_argument("lo and n must have three entries");
          return TsdfBrickMark(lo.data(), step, n.data(), B, poses, intri, dist, depth, conf.has_value() ? *conf : Tensor(), trunc);
        },
        py::arg("lo"), py::arg("step"), py::arg("n"), py::arg("B"), py::arg("poses"), py::arg("intri"), py::arg("dist"), py::arg("depth"),
        py::arg("conf"), py::arg("trunc"));
  // ... the views added to the rows S, W [n_bricks, (B+1)^3] of brick_ids, in place (f2n_tsdf_integrate_bricks) ...
  m.def("tsdf_integrate_bricks",
        [](const Tensor& S, const Tensor& W, const Tensor& brick_ids, const std::vector<float>& lo, float step, const std::vector<int>& n, int B,
           const Tensor& poses, const Tensor& intri, const Tensor& dist, const Tensor& depth, const c10::optional<Tensor>& conf, float trunc) {
          if (lo.size() != 3 || n.size() != 3) throw std::invalid_argument("lo and n must have three entries");
          TsdfIntegrateBricks(S, W, brick_ids, lo.data(), step, n.data(), B, poses, intri, dist, depth, conf.has_value() ? *conf : Tensor(),
                              trunc);
        },
        py::arg("S"), py::arg("W"), py::arg("brick_ids"), py::arg("lo"), py::arg("step"), py::arg("n"), py::arg("B"), py::arg("poses"),
        py::arg("intri"), py::arg("dist"), py::arg("depth"), py::arg("conf"), py::arg("trunc"));
  // ... (verts, faces) of values / valid [n_bricks, (B+1)^3] (f2n_brick_mesh_count_masked / _emit_masked, sorted by key, without the
  // vertices no face names): the bits of mesh_from_grid_masked when the list holds the owner of every face ...
  m.def("mesh_from_bricks_masked",
        [](const Tensor& values, const Tensor& valid, const Tensor& brick_ids, const std::vector<int>& n, const std::vector<float>& lo,
           float step, float level, int B, int64_t batch_bricks) {
          if (lo.size() != 3 || n.size() != 3) throw std::invalid_argument("lo and n must have three entries");
          auto t = MeshFromBricksMasked(values, valid, brick_ids, n.data(), lo.data(), step, level, B, batch_bricks);
          return std::vector<Tensor>{std::get<0>(t), std::get<1>(t)};
        },
        py::arg("values"), py::arg("valid"), py::arg("brick_ids"), py::arg("n"), py::arg("lo"), py::arg("step"), py::arg("level"), py::arg("B"),
        py::arg("batch_bricks") = 0);
  // ... and the whole chain with one batch of batch_bricks rows alive at a time: (verts, faces, stats)
  m.def("tsdf_mesh_sparse",
        [](const std::vector<float>& lo, float step, const std::vector<int>& n, int B, const Tensor& poses, const Tensor& intri,
           const Tensor& dist, const Tensor& depth, const c10::optional<Tensor>& conf, float trunc, float min_weight, int64_t batch_bricks) {
          if (lo.size() != 3 || n.size() != 3) throw std::invalid_argument("lo and n must have three entries");
          SparseTsdfStats st;
          auto t = TsdfMeshSparse(lo.data(), step, n.data(), B, poses, intri, dist, depth, conf.has_value() ? *conf : Tensor(), trunc,
                                  min_weight, batch_bricks, &st);
          py::dict stats;
          stats["bricks"] = st.bricks;
          stats["active_bricks"] = st.active_bricks;
          stats["meshed_bricks"] = st.meshed_bricks;
          stats["points_evaluated"] = st.points_evaluated;
          stats["points_known"] = st.points_known;
          stats["batches"] = st.batches;
          stats["grid"] = py::make_tuple(st.grid[0], st.grid[1], st.grid[2]);
          return py::make_tuple(std::get<0>(t), std::get<1>(t), stats);
        },
        py::arg("lo"), py::arg("step"), py::arg("n"), py::arg("B"), py::arg("poses"), py::arg("intri"), py::arg("dist"), py::arg("depth"),
        py::arg("conf"), py::arg("trunc"), py::arg("min_weight"), py::arg("batch_bricks"));
  // unit normals [n,3] at pts [n,3] from the gradient of any float32 grid [nz, ny, nx] (f2n_grid_normals)
  m.def("grid_normals",
        [](const Tensor& grid, const Tensor& pts, const std::vector<float>& lo, float step) {
          TORCH_CHECK(lo.size() == 3, "lo must have three coordinates");
          return GridNormals(grid, pts, lo.data(), step);
        },
        py::arg("grid"), py::arg("pts"), py::arg("lo") = std::vector<float>{0.f, 0.f, 0.f}, py::arg("step") = 1.f);
  // labels [V] int32 = the smallest vertex index of every vertex's connected component (f2n_mesh_components);
  // with_rounds: (labels, number of labelling rounds)
  m.def("mesh_components",
        [](const Tensor& faces, int64_t n_verts, bool with_rounds) -> py::object {
          int rounds = 0;
          Tensor labels = MeshComponents(faces, n_verts, &rounds);
          if (with_rounds) return py::make_tuple(labels, rounds);
          return py::cast(labels);
        },
        py::arg("faces"), py::arg("n_verts"), py::arg("with_rounds") = false);
  // the mesh without its components of fewer than min_faces faces, order kept: [verts, faces, vert_src]
  m.def("mesh_filter_components",
        [](const Tensor& verts, const Tensor& faces, int min_faces) {
          auto t = MeshFilterComponents(verts, faces, min_faces);
          return std::vector<Tensor>{std::get<0>(t), std::get<1>(t), std::get<2>(t)};
        },
        py::arg("verts"), py::arg("faces"), py::arg("min_faces"));
  // vertex clustering with quadric-error placement on cells of size `cell` from `lo` (None: the vertices' bounding-box minimum):
  // [verts, faces, vert_map] (f2n_mesh_cluster_*); lam ties a vertex to its cluster's mean where the planes leave it free
  m.def("mesh_simplify",
        [](const Tensor& verts, const Tensor& faces, float cell, const c10::optional<std::vector<float>>& lo, double lam) {
          TORCH_CHECK(!lo.has_value() || lo->size() == 3, "lo must have three coordinates");
          auto t = MeshSimplify(verts, faces, cell, lo.has_value() ? lo->data() : nullptr, lam);
          return std::vector<Tensor>{std::get<0>(t), std::get<1>(t), std::get<2>(t)};
        },
        py::arg("verts"), py::arg("faces"), py::arg("cell"), py::arg("lo") = py::none(), py::arg("lam") = 1e-3);
  // Mesh refinement on any mesh (f2n_mesh_ring_*, f2n_mesh_smooth, f2n_mesh_face_quality, f2n_level_step; include/f2n_abi.h).
  // the vertex one-ring: (ring_start_end [V,2], ring [E] neighbours ascending, pinned [V] uint8, [boundary_edges, nonmanifold_edges])
  m.def("mesh_ring",
        [](const Tensor& faces, int64_t n_verts) {
          if (n_verts < 0) throw std::invalid_argument("mesh_ring: n_verts must be >= 0");
          MeshRingResult r = MeshRing(faces, n_verts);
          Tensor ec = r.edge_counts.cpu();
          return py::make_tuple(r.start_end, r.ring, r.pinned, std::vector<int64_t>{ec.data_ptr<int32_t>()[0], ec.data_ptr<int32_t>()[1]});
        },
        py::arg("faces"), py::arg("n_verts"));
  // `passes` Taubin lambda|mu pairs (mu = lam: plain Laplacian pairs), boundary and non-manifold vertices pinned; max_move: the clamp
  // of every vertex to a ball around its input position.  ValueError for passes < 0, lam / mu not finite, max_move <= 0
  m.def("mesh_smooth",
        [](const Tensor& verts, const Tensor& faces, int passes, double lam, double mu, float max_move) {
          return MeshSmooth(verts, faces, passes, lam, mu, max_move);
        },
        py::arg("verts"), py::arg("faces"), py::arg("passes"), py::arg("lam") = 0.5, py::arg("mu") = -0.53,
        py::arg("max_move") = std::numeric_limits<float>::infinity());
  // [F] float64: 1 for an equilateral face, towards 0 for a sliver, 0 for a degenerate or invalid face, NaN for a coordinate not finite
  // [R]: the distortion loss of every ray on its warped intervals (f2n_distortion_fwd; no reference counterpart), on any device arrays:
  // weights [M], dt [M], idx_start_end [R,2] int32, e.g. those of render_geometry(return_samples=True)
  m.def("ray_distortion",
        [](const Tensor& weights, const Tensor& dt, const Tensor& idx_start_end) {
          TORCH_CHECK(idx_start_end.dim() == 2 && idx_start_end.size(1) == 2, "idx_start_end must be [R,2]");
          TORCH_CHECK(weights.dim() == 1 && dt.dim() == 1 && weights.size(0) == dt.size(0), "weights and dt must be [M]");
          CheckDev(weights, torch::kFloat32, "weights");
          CheckDev(dt, torch::kFloat32, "dt");
          CheckDev(idx_start_end, torch::kInt32, "idx_start_end");
          torch::NoGradGuard no_grad;
          return CustomOps::Distortion(weights, dt, idx_start_end);
        },
        py::arg("weights"), py::arg("dt"), py::arg("idx_start_end"));
  m.def("mesh_face_quality", [](const Tensor& verts, const Tensor& faces) { return MeshFaceQuality(verts, faces); }, py::arg("verts"),
        py::arg("faces"));
  // the raw per-iteration update of the level-set projection on the caller's device arrays; cand .. evals are updated in place
  m.def("level_step",
        [](bool first, bool propose, const Tensor& p0, const Tensor& sigma, const Tensor& grad, const Tensor& h, float tol, float max_step,
           float max_move, const Tensor& cand, const Tensor& best, const Tensor& h_best, const Tensor& g_best, const Tensor& scale,
           const Tensor& status, const Tensor& evals) {
          LevelStep(first, propose, p0, sigma, grad, h, tol, max_step, max_move, cand, best, h_best, g_best, scale, status, evals);
        },
        py::arg("first"), py::arg("propose"), py::arg("p0"), py::arg("sigma"), py::arg("grad"), py::arg("h"), py::arg("tol"),
        py::arg("max_step"), py::arg("max_move"), py::arg("cand"), py::arg("best"), py::arg("h_best"), py::arg("g_best"), py::arg("scale"),
        py::arg("status"), py::arg("evals"));
  // the acceleration grid of mesh_raycast over a mesh: (lo [3], cell, dims [3], cell_start, cell_faces); cell None: the documented
  // default (Renderer.h: MeshRaycastDefaultCell), lo None: the vertices' bounding-box minimum.  ValueError for a grid that is too fine
  m.def("mesh_raycast_build",
        [](const Tensor& verts, const Tensor& faces, const c10::optional<float>& cell, const c10::optional<std::vector<float>>& lo) {
          if (lo.has_value() && lo->size() != 3) throw std::invalid_argument("lo must have three coordinates");
          if (cell.has_value() && std::isnan(*cell)) throw std::invalid_argument("mesh_raycast_build: cell must be positive and finite");
          MeshRaycastAccel a = MeshRaycastBuild(verts, faces, cell.has_value() ? *cell : std::numeric_limits<float>::quiet_NaN(),
                                                lo.has_value() ? lo->data() : nullptr);
          return py::make_tuple(std::vector<float>{a.lo[0], a.lo[1], a.lo[2]}, a.cell, std::vector<int>{a.dims[0], a.dims[1], a.dims[2]},
                                a.cell_start, a.cell_faces);
        },
        py::arg("verts"), py::arg("faces"), py::arg("cell") = py::none(), py::arg("lo") = py::none());
  // the rays' first hit on the mesh: [t, face, bary]; accel = mesh_raycast_build's tuple, or None for the brute-force mode.
  // ValueError for rays outside the traversal's domain (origins more than 2^15 cells from the frame's origin)
  m.def("mesh_raycast",
        [](const Tensor& verts, const Tensor& faces, const py::object& accel, const Tensor& rays_o, const Tensor& rays_d,
           const c10::optional<Tensor>& bounds) {
          MeshRaycastAccel a;
          const bool have = !accel.is_none();
          if (have) {
            py::tuple t = accel.cast<py::tuple>();
            if (t.size() != 5) throw std::invalid_argument("accel must be mesh_raycast_build's (lo, cell, dims, cell_start, cell_faces)");
            const auto lo = t[0].cast<std::vector<float>>();
            const auto dims = t[2].cast<std::vector<int>>();
            if (lo.size() != 3 || dims.size() != 3) throw std::invalid_argument("accel: lo and dims must have three entries");
            for (int k = 0; k < 3; k++) {
              a.lo[k] = lo[k];
              a.dims[k] = dims[k];
            }
            a.cell = t[1].cast<float>();
            a.cell_start = t[3].cast<Tensor>();
            a.cell_faces = t[4].cast<Tensor>();
          }
          auto r = MeshRaycast(verts, faces, have ? &a : nullptr, rays_o, rays_d, bounds.has_value() ? *bounds : Tensor());
          return std::vector<Tensor>{std::get<0>(r), std::get<1>(r), std::get<2>(r)};
        },
        py::arg("verts"), py::arg("faces"), py::arg("accel"), py::arg("rays_o"), py::arg("rays_d"), py::arg("bounds") = py::none());
  // the points' closest point on the mesh: [dist (+inf: none within max_dist), face (-1: none), bary]; accel = mesh_raycast_build's
  // tuple, or None for the brute-force mode.  ValueError for a finite point outside the walk's domain (more than 2^15 cells from the
  // frame's origin)
  m.def("mesh_closest_point",
        [](const Tensor& verts, const Tensor& faces, const py::object& accel, const Tensor& points, float max_dist) {
          MeshRaycastAccel a;
          const bool have = !accel.is_none();
          if (have) {
            py::tuple t = accel.cast<py::tuple>();
            if (t.size() != 5) throw std::invalid_argument("accel must be mesh_raycast_build's (lo, cell, dims, cell_start, cell_faces)");
            const auto lo = t[0].cast<std::vector<float>>();
            const auto dims = t[2].cast<std::vector<int>>();
            if (lo.size() != 3 || dims.size() != 3) throw std::invalid_argument("accel: lo and dims must have three entries");
            for (int k = 0; k < 3; k++) {
              a.lo[k] = lo[k];
              a.dims[k] = dims[k];
            }
            a.cell = t[1].cast<float>();
            a.cell_start = t[3].cast<Tensor>();
            a.cell_faces = t[4].cast<Tensor>();
          }
          auto r = MeshClosestPoint(verts, faces, have ? &a : nullptr, points, max_dist);
          return std::vector<Tensor>{std::get<0>(r), std::get<1>(r), std::get<2>(r)};
        },
        py::arg("verts"), py::arg("faces"), py::arg("accel"), py::arg("points"),
        py::arg("max_dist") = std::numeric_limits<float>::infinity());
  // n area-uniform, stratified samples of the mesh's surface, a pure function of (mesh, n, seed): [points, face, bary]
  m.def("mesh_sample_surface",
        [](const Tensor& verts, const Tensor& faces, int64_t n, uint64_t seed) {
          auto r = MeshSampleSurface(verts, faces, n, seed);
          return std::vector<Tensor>{std::get<0>(r), std::get<1>(r), std::get<2>(r)};
        },
        py::arg("verts"), py::arg("faces"), py::arg("n"), py::arg("seed") = 0);
  // the texture atlas of a mesh: (uv [F,3,2], size, blocks, density_used); blocks = dict of the device tensors mesh_atlas_texels needs
  // (offsets [B+1] int64, block_log, block_faces, log_s, rot, slot).  ValueError: max_size no power of two, or the mesh cannot fit
  m.def("mesh_atlas",
        [](const Tensor& verts, const Tensor& faces, float density, int max_size, int max_log) {
          MeshAtlasResult a = MeshAtlas(verts, faces, density, max_size, max_log);
          py::dict b;
          b["offsets"] = a.offsets; b["block_log"] = a.block_log; b["block_faces"] = a.block_faces;
          b["log_s"] = a.log_s; b["rot"] = a.rot; b["slot"] = a.slot;
          return py::make_tuple(a.uv, a.size, b, a.density_used);
        },
        py::arg("verts"), py::arg("faces"), py::arg("density"), py::arg("max_size") = 8192, py::arg("max_log") = 7);
  // [tex_face [S,S] int32, tex_bary [S,S,3], tex_pos [S,S,3]] of mesh_atlas's blocks at its size
  m.def("mesh_atlas_texels",
        [](const Tensor& verts, const Tensor& faces, const py::dict& blocks, int size, bool clamp) {
          MeshAtlasResult a;
          a.size = size;
          a.offsets = blocks["offsets"].cast<Tensor>(); a.block_log = blocks["block_log"].cast<Tensor>();
          a.block_faces = blocks["block_faces"].cast<Tensor>(); a.rot = blocks["rot"].cast<Tensor>();
          auto r = MeshAtlasTexels(verts, faces, a, clamp);
          return std::vector<Tensor>{std::get<0>(r), std::get<1>(r), std::get<2>(r)};
        },
        py::arg("verts"), py::arg("faces"), py::arg("blocks"), py::arg("size"), py::arg("clamp") = true);
  m.def("texture_sample", [](const Tensor& tex, const Tensor& uv) { return TextureSample(tex, uv); }, py::arg("tex"), py::arg("uv"));
  m.def("image_ssim",
        [](const Tensor& a, const Tensor& b, double max_val, int filter_size, double filter_sigma, double k1, double k2, bool return_map) {
          auto r = ImageSSIM(a, b, max_val, filter_size, filter_sigma, k1, k2, return_map);
          return py::make_tuple(std::get<0>(r), std::get<1>(r), std::get<2>(r).defined() ? py::cast(std::get<2>(r)) : py::none());
        },
        py::arg("a"), py::arg("b"), py::arg("max_val") = 1.0, py::arg("filter_size") = 11, py::arg("filter_sigma") = 1.5, py::arg("k1") = 0.01,
        py::arg("k2") = 0.03, py::arg("return_map") = false);
  m.def("dp_set_table_buckets", [](int n) { DataParallel::table_buckets = n; });  // table all-reduce buckets of the next attach (A/B)
  // data-parallel replicas draw stream `rank` of every keyed purpose (KeyedDraws.h; the native attach sets it itself)
  m.def("dp_set_replica", [](int rank) { KeyedUniforms::SetReplica(rank); });
  m.def("keyed_draw_key", [](uint64_t seed, uint64_t purpose, int rank) {  // the Philox key of a purpose on a rank (no device needed)
    return KeyedUniforms::KeyOf(seed, purpose, KeyedUniforms::SaltOf(rank));
  });
  m.def("dp_new_unique_id", []() {  // rank 0: the id every rank passes to attach_data_parallel
    auto id = DataParallel::NewUniqueId();
    return py::bytes(reinterpret_cast<const char*>(id.data()), id.size());
  });
  // the schedules of ExpRunner::Train as a pure function (no device needed): tests pin them against the reference's own code
  m.def("schedule_at", [](float init_fineness, int fineness_decay_end, float lr, float lr_alpha, float lr_warm_up_end, int end_iter,
                          float gs_start, float gs_end, float var_w, int var_start, int var_end, int iter) {
    ExpRunner::ScheduleParams p{init_fineness, fineness_decay_end, lr, lr_alpha, lr_warm_up_end, end_iter, gs_start, gs_end, var_w,
                                var_start, var_end};
    auto v = ExpRunner::ScheduleAt(p, iter);
    return std::vector<float>{v.fineness, v.lr, v.gradient_scaling_progress, v.var_loss_weight};
  });
  // the step / exchange interleaving of ExpRunner::TrainStep on its own (no device): tests drive it with recording callbacks
  py::class_<GradSyncPipeline>(m, "GradSyncPipeline")
      .def(py::init<>())
      .def_readwrite("pipelined", &GradSyncPipeline::pipelined)
      .def("set_blocking", [](GradSyncPipeline& p, py::function f) { p.blocking = [f]() { f(); }; })
      .def("set_begin_end", [](GradSyncPipeline& p, py::function b, py::function e) { p.begin = [b]() { b(); }; p.end = [e]() { e(); }; })
      .def("set_apply", [](GradSyncPipeline& p, py::function f) { p.apply = [f](bool a, float lr) { f(a, lr); }; })
      .def("set_defer_flags", [](GradSyncPipeline& p, py::function f) { p.defer_flags = [f]() { f(); }; })
      .def("set_bucket", [](GradSyncPipeline& p, py::function f) { p.bucket = [f](int b, int n) { f(b, n); }; })
      .def("bucket_ready", &GradSyncPipeline::BucketReady)
      .def("set_small_exchange", [](GradSyncPipeline& p, py::function f) { p.small_exchange = [f](void*) { f(); }; })
      .def("small_grads_ready", [](GradSyncPipeline& p) { p.SmallGradsReady(nullptr); })
      .def_readwrite("small_first", &GradSyncPipeline::small_first)
      .def_property_readonly("small_sent", &GradSyncPipeline::small_sent)
      .def_property_readonly("buckets_sent", &GradSyncPipeline::buckets_sent)
      .def("installed", &GradSyncPipeline::Installed)
      .def("pending", &GradSyncPipeline::Pending)
      .def("begin_step", [](GradSyncPipeline& p, bool apply_optimizer, py::function presample) { p.BeginStep(apply_optimizer, [presample]() { presample(); }); })
      .def("gradients_ready", &GradSyncPipeline::GradientsReady)
      .def("finish_pending_step", &GradSyncPipeline::FinishPendingStep);
  py::class_<ExpRunner>(m, "ExpRunner")
      .def(py::init<const std::map<std::string, std::string>&, int>(), py::arg("flat_config"), py::arg("n_images"))
      .def("load_states", &ExpRunner::LoadStates)
      .def("states", &ExpRunner::States)
      .def("aux_states", &ExpRunner::AuxStates)
      .def("load_aux_states", &ExpRunner::LoadAuxStates)
      .def("train_step",
           [](ExpRunner& r, const Tensor& ro, const Tensor& rd, const Tensor& b, const Tensor& gt, const Tensor& emb, bool apply,
              const std::optional<Tensor>& nro, const std::optional<Tensor>& nrd, const std::optional<Tensor>& nb,
              const std::optional<Tensor>& n2ro, const std::optional<Tensor>& n2rd) {
             TrainStats s;
             {
               py::gil_scoped_release no_gil;  // hooks re-acquire the GIL themselves
               s = r.TrainStep(ro, rd, b, gt, emb, apply, nro.value_or(Tensor()), nrd.value_or(Tensor()), nb.value_or(Tensor()),
                               n2ro.value_or(Tensor()), n2rd.value_or(Tensor()));
             }
             return StatsToDict(s);
           },
           py::arg("rays_o"), py::arg("rays_d"), py::arg("bounds"), py::arg("gt_colors"), py::arg("emb_idx"),
           py::arg("apply_optimizer") = true, py::arg("next_rays_o") = py::none(), py::arg("next_rays_d") = py::none(),
           py::arg("next_bounds") = py::none(), py::arg("next2_rays_o") = py::none(), py::arg("next2_rays_d") = py::none())
      .def("train_step_autograd",
           [](ExpRunner& r, const Tensor& ro, const Tensor& rd, const Tensor& b, const Tensor& gt, const Tensor& emb, bool apply) {
             TrainStats s;
             {
               py::gil_scoped_release no_gil;  // the autograd engine must not be entered while holding the GIL
               s = r.TrainStepAutograd(ro, rd, b, gt, emb, apply);
             }
             return StatsToDict(s);
           },
           py::arg("rays_o"), py::arg("rays_d"), py::arg("bounds"), py::arg("gt_colors"), py::arg("emb_idx"),
           py::arg("apply_optimizer") = true)
      .def_readwrite("end_iter", &ExpRunner::end_iter_)
      .def_readwrite("forward_render", &ExpRunner::forward_render_)
      .def_readwrite("render_chunk_rays", &ExpRunner::render_chunk_rays_)
      .def_readwrite("dist_loss_weight", &ExpRunner::dist_loss_weight_)  // train.dist_loss_weight (0 = off; no reference counterpart)
      .def("last_losses", &ExpRunner::LastLosses)  // device [8] of the last training step: loss, colour, var, disp, tv, mse, dist, 0
      .def("ray_distortion",  // [N]: the distortion of any number of rays, rendered as render_rays renders them
           [](ExpRunner& r, const Tensor& ro, const Tensor& rd, const Tensor& b) {
             py::gil_scoped_release no_gil;
             return r.RayDistortion(ro, rd, b);
           },
           py::arg("rays_o"), py::arg("rays_d"), py::arg("bounds"))
      .def("render_rays", &ExpRunner::RenderRays)
      .def("render_whole_image", &ExpRunner::RenderWholeImage)
      .def("test_image_psnr", &ExpRunner::TestImagePSNR)
      .def("test_image_metrics",
           [](ExpRunner& r, Dataset& ds, int idx) {
             auto m = r.TestImageMetrics(ds, idx);
             py::dict d;
             d["psnr"] = m.psnr; d["ssim"] = m.ssim; d["pred"] = m.pred; d["disp"] = m.disp; d["oct_disp"] = m.oct_disp;
             return d;
           },
           py::arg("dataset"), py::arg("idx"))
      .def("test_images", &ExpRunner::TestImages)
      .def("visualize_image", &ExpRunner::VisualizeImage)
      .def("render_path_frame", &ExpRunner::RenderPathFrame, py::arg("dataset"), py::arg("pose"), py::arg("res_level") = 1)
      .def("render_path",
           [](ExpRunner& r, Dataset& ds, const Tensor& poses, py::function sink, int res_level) {
             r.RenderPath(ds, poses, [sink](int i, const Tensor& img) { sink(i, img); }, res_level);
           },
           py::arg("dataset"), py::arg("render_poses"), py::arg("sink"), py::arg("res_level") = 1)
      .def("save_checkpoint", &ExpRunner::SaveCheckpoint)
      .def("load_checkpoint", &ExpRunner::LoadCheckpoint)
      .def("train",
           [](ExpRunner& r, Dataset& ds, int until_iter, int sets) {
             int n;
             {
               py::gil_scoped_release no_gil;
               n = r.Train(ds, until_iter, sets);
             }
             py::dict d = StatsToDict(r.last_train_stats_);
             d["iterations"] = n;
             d["total_meaningful"] = r.last_train_meaningful_;
             d["total_marched"] = r.last_train_marched_;
             d["total_rays"] = r.last_train_rays_;
             return d;
           },
           py::arg("dataset"), py::arg("until_iter") = -1, py::arg("sets") = DATA_TRAIN_SET)
      .def("render_train",
           [](ExpRunner& r, const Tensor& ro, const Tensor& rd, const Tensor& b, const Tensor& emb) {
             r.global_data_pool_->mode_ = RunningMode::TRAIN;
             auto rr = r.renderer_->Render(ro, rd, b, emb);
             py::dict d;
             d["colors"] = rr.colors; d["first_oct_dis"] = rr.first_oct_dis; d["disparity"] = rr.disparity;
             d["edge_feats"] = rr.edge_feats; d["depth"] = rr.depth; d["weights"] = rr.weights;
             d["idx_start_end"] = rr.idx_start_end;
             d["dt"] = rr.dt;  // [M]: the survivors' warped step lengths
             return d;
           })
      .def("get_samples",
           [](ExpRunner& r, const Tensor& ro, const Tensor& rd, const Tensor& b) {
             auto s = r.renderer_->pts_sampler_->GetSamples(ro, rd, b);
             py::dict d;
             d["pts"] = s.pts; d["dirs"] = s.dirs; d["dt"] = s.dt; d["t"] = s.t; d["anchors"] = s.anchors;
             d["pts_idx_bounds"] = s.pts_idx_bounds; d["first_oct_dis"] = s.first_oct_dis;
             return d;
           })
      .def("anchored_query", [](ExpRunner& r, const Tensor& pts, const Tensor& anchors) { return r.renderer_->scene_field_->AnchoredQuery(pts, anchors); })
      .def("shader_query", [](ExpRunner& r, const Tensor& feats, const Tensor& dirs) { return r.renderer_->shader_->Query(feats, dirs); })
      .def("zero_grad", [](ExpRunner& r) { r.renderer_->ZeroGrad(); })
      .def("optim_step", [](ExpRunner& r) { r.OptimStep(nullptr); })
      .def("grads",
           [](ExpRunner& r) {
             py::dict d;
             d["feat_pool"] = FieldOf(r)->TableGradUnscaled();
             d["field_mlp"] = FieldOf(r)->mlp_->GradUnscaled();
             d["color_mlp"] = ShaderOf(r)->mlp_->GradUnscaled();
             d["app_emb"] = r.renderer_->app_emb_grad_.clone();
             return d;
           })
      .def("grad_buffers",  // raw buffers for the data-parallel all-reduce (RCCL): hash table (f16 x128), MLPs, app_emb
           [](ExpRunner& r) {
             return std::vector<Tensor>{FieldOf(r)->grad_h_, FieldOf(r)->mlp_->grad_scaled_, ShaderOf(r)->mlp_->grad_scaled_,
                                        r.renderer_->app_emb_grad_};
           })
      .def("flatten_small_grads", &ExpRunner::FlattenSmallGrads)
      .def("occupancy_buffers",
           [](ExpRunner& r) {
             auto& o = *SamplerOf(r)->pers_octree_;
             return std::vector<Tensor>{o.tree_weight_stats_, o.tree_alpha_stats_, o.tree_visit_cnt_};
           })
      .def("set_grad_sync_hook", [](ExpRunner& r, py::function f) { r.sync_.blocking = [f]() { py::gil_scoped_acquire g; f(); }; })
      .def("set_pipelined_grad_sync",
           [](ExpRunner& r, py::function begin, py::function end) {
             r.sync_.begin = [begin]() { py::gil_scoped_acquire g; begin(); };
             r.sync_.end = [end]() { py::gil_scoped_acquire g; end(); };
             r.sync_.pipelined = true;
           })
      .def("flush", [](ExpRunner& r) { py::gil_scoped_release no_gil; r.FinishPending(); })
      // world-space queries of the scene (Renderer::QueryDensity & co.): a streaming step is flushed first, as save_checkpoint does
      .def("locate_points",  // world [n,3] -> [warped [n,3], anchors [n,3] = (trans_idx, leaf, 0) or (-1, -1, 0)]
           [](ExpRunner& r, const Tensor& world) {
             py::gil_scoped_release no_gil;
             r.FinishPending();
             auto t = SamplerOf(r)->LocatePoints(world);
             return std::vector<Tensor>{std::get<0>(t), std::get<1>(t)};
           })
      .def("query_density",  // world [n,3] -> density [n] = exp(f0 - 3), exactly 0 where no leaf holds the point
           [](ExpRunner& r, const Tensor& world) {
             py::gil_scoped_release no_gil;
             r.FinishPending();
             return r.renderer_->QueryDensity(world);
           })
      // The field's pre-pass caches as a step's consumer would find them (tests of the queries' cache contract, PrepassCacheGuard):
      // density_prepass runs Hash3DAnchored::QueryDensityPreAct(keep_features = true, keep_outputs) on located points and returns f0;
      // prepass_caches returns [hash features h16 [n,32], field outputs h16 [n,16]], an empty tensor for a cache that is not held
      .def("density_prepass",
           [](ExpRunner& r, const Tensor& warped, const Tensor& anchors, bool keep_outputs) {
             py::gil_scoped_release no_gil;
             r.FinishPending();
             return FieldOf(r)->QueryDensityPreAct(warped, anchors, /*keep_features=*/true, keep_outputs);
           },
           py::arg("warped"), py::arg("anchors"), py::arg("keep_outputs") = true)
      .def("prepass_caches",
           [](ExpRunner& r) {
             auto* f = FieldOf(r);
             Tensor none = torch::empty({0}, torch::kFloat16);
             return std::vector<Tensor>{f->prepass_x_.defined() ? f->prepass_x_ : none, f->prepass_feat_h_.defined() ? f->prepass_feat_h_ : none};
           })
      // the third cache, which a streaming train step's pre-pass keeps in place of the rows: density_prepass_planes runs
      // QueryDensityPreAct(keep_features, keep_outputs, keep_planes), prepass_planes returns h16 [8,n,4] or an empty tensor
      .def("density_prepass_planes",
           [](ExpRunner& r, const Tensor& warped, const Tensor& anchors) {
             py::gil_scoped_release no_gil;
             r.FinishPending();
             return FieldOf(r)->QueryDensityPreAct(warped, anchors, /*keep_features=*/true, /*keep_outputs=*/true, /*keep_planes=*/true);
           },
           py::arg("warped"), py::arg("anchors"))
      .def("prepass_planes",
           [](ExpRunner& r) {
             auto* f = FieldOf(r);
             return f->prepass_planes_.defined() ? f->prepass_planes_ : torch::empty({0}, torch::kFloat16);
           })
      .def("density_grid",  // [nz, ny, nx] densities on the grid of grid_spec(lo, hi, res)
           [](ExpRunner& r, const std::vector<float>& lo, const std::vector<float>& hi, int res) {
             py::gil_scoped_release no_gil;
             r.FinishPending();
             return r.renderer_->DensityGrid(lo, hi, res);
           },
           py::arg("lo"), py::arg("hi"), py::arg("res"))
      .def("extract_mesh",  // (verts [V,3] f32 in the scene's normalised frame, faces [F,3] int32) of the density grid at `level`
           [](ExpRunner& r, const std::vector<float>& lo, const std::vector<float>& hi, int res, float level) {
             py::gil_scoped_release no_gil;
             r.FinishPending();
             auto t = r.renderer_->ExtractMesh(lo, hi, res, level);
             return std::vector<Tensor>{std::get<0>(t), std::get<1>(t)};
           },
           py::arg("lo"), py::arg("hi"), py::arg("res"), py::arg("level"))
      .def("extract_mesh_sparse",  // extract_mesh's bits from the bricks of brick^3 cells that can hold something; res up to 8192
           [sparse_stats](ExpRunner& r, const std::vector<float>& lo, const std::vector<float>& hi, int res, float level, int brick) {
             SparseMeshStats st;
             std::tuple<Tensor, Tensor> t;
             {
               py::gil_scoped_release no_gil;
               r.FinishPending();
               t = r.renderer_->ExtractMeshSparse(lo, hi, res, level, brick, &st);
             }
             py::dict d;
             d["verts"] = std::get<0>(t);
             d["faces"] = std::get<1>(t);
             d["stats"] = sparse_stats(st);
             return d;
           },
           py::arg("lo"), py::arg("hi"), py::arg("res"), py::arg("level"), py::arg("brick") = 8)
      .def("query_radiance",  // world [n,3], unit dirs [n,3] -> [density [n] (= query_density), rgb [n,3]]; zeros for empty points
           [](ExpRunner& r, const Tensor& world, const Tensor& dirs) {
             py::gil_scoped_release no_gil;
             r.FinishPending();
             auto t = r.renderer_->QueryRadiance(world, dirs);
             return std::vector<Tensor>{std::get<0>(t), std::get<1>(t)};
           },
           py::arg("world"), py::arg("dirs"))
      .def("extract_mesh_attrs",  // extract_mesh + floater removal, normals from the density grid, colours along the inward normal
           [sparse_stats](ExpRunner& r, const std::vector<float>& lo, const std::vector<float>& hi, int res, float level, int min_component_faces,
              bool normals, bool colors, const std::string& normal_source, int simplify, const py::object& refine, int sparse) {
             MeshRefineOptions ro;
             if (!refine.is_none()) {  // a dict of the stage's options; an unknown key is an error
               ro.on = true;
               for (auto item : refine.cast<py::dict>()) {
                 const std::string key = item.first.cast<std::string>();
                 if (key == "smooth_passes") ro.smooth_passes = item.second.cast<int>();
                 else if (key == "lam") ro.lam = item.second.cast<double>();
                 else if (key == "mu") ro.mu = item.second.cast<double>();
                 else if (key == "project") ro.project = item.second.cast<bool>();
                 else if (key == "iters") ro.iters = item.second.cast<int>();
                 else if (key == "max_step_steps") ro.max_step_steps = item.second.cast<float>();
                 else if (key == "max_move_steps") ro.max_move_steps = item.second.cast<float>();
                 else if (key == "tol") ro.tol = item.second.cast<float>();
                 else throw std::invalid_argument("extract_mesh_attrs: unknown refine option \"" + key + "\"");
               }
             }
             MeshAttrs a;
             {
               py::gil_scoped_release no_gil;
               r.FinishPending();
               InferenceMode mode(r, ro.on);  // (the projection refuses to run in training mode; without the stage nothing changes)
               a = r.renderer_->ExtractMeshAttrs(lo, hi, res, level, min_component_faces, normals, colors, normal_source, simplify, ro, sparse);
             }
             py::dict d;
             d["verts"] = a.verts;
             d["faces"] = a.faces;
             if (sparse != 0) d["sparse"] = sparse_stats(a.sparse);
             if (normals) d["normals"] = a.normals;
             if (colors) d["colors"] = a.colors;
             if (simplify >= 2) {  // the size of the mesh before the simplification
               d["verts_in"] = a.verts_in;
               d["faces_in"] = a.faces_in;
             }
             if (ro.on) {  // the stage's statistics: counts as ints, everything else as floats
               py::dict s;
               for (const auto& kv : a.refine) {
                 const bool real = kv.first.rfind("h_", 0) == 0 || kv.first.rfind("moved_", 0) == 0 || kv.first.rfind("quality_", 0) == 0 ||
                                   kv.first.rfind("max_", 0) == 0;
                 if (real) s[py::str(kv.first)] = kv.second;
                 else s[py::str(kv.first)] = (int64_t) kv.second;
               }
               d["refine"] = s;
             }
             return d;
           },
           py::arg("lo"), py::arg("hi"), py::arg("res"), py::arg("level"), py::arg("min_component_faces") = 0, py::arg("normals") = true,
           py::arg("colors") = true, py::arg("normal_source") = "grid",  // "field": normals (and colours) from the field's own gradient
           py::arg("simplify") = 0,  // k >= 2: mesh_simplify on clusters of k^3 grid cells before the attributes are computed
           // a dict (smooth_passes, lam, mu, project, iters, max_step_steps, max_move_steps, tol; {} = the defaults): Taubin smoothing and
           // the projection onto the level set after the simplification, before the attributes; the result gains a "refine" dict
           py::arg("refine") = py::none(),
           // 4, 8 or 16: the mesh from extract_mesh_sparse with that brick size (the same bits, no dense grid; needs normal_source="field"
           // for normals or colours); the result gains a "sparse" dict, extract_mesh_sparse's stats
           py::arg("sparse") = 0)
      .def("project_to_level",  // points [n,3] moved onto sigma = level: a dict of points, h_in, h_out (ln(sigma / level)), status, evals
           [](ExpRunner& r, const Tensor& points, float level, int iters, float max_step, float max_move, float tol,
              const c10::optional<Tensor>& origins) {
             LevelProjection p;
             {
               py::gil_scoped_release no_gil;
               r.FinishPending();
               InferenceMode mode(r, true);
               p = r.renderer_->ProjectToLevel(points, level, iters, max_step, max_move, tol, origins.has_value() ? *origins : Tensor());
             }
             py::dict d;
             d["points"] = p.points; d["h_in"] = p.h_in; d["h_out"] = p.h_out; d["status"] = p.status; d["evals"] = p.evals;
             return d;
           },
           py::arg("points"), py::arg("level"), py::arg("iters") = 8, py::arg("max_step") = std::numeric_limits<float>::infinity(),
           py::arg("max_move") = std::numeric_limits<float>::infinity(), py::arg("tol") = 1e-3f,
           py::arg("origins") = py::none())  // [n,3]: the centres of the max_move balls (None: the points themselves)
      .def("query_density_grad",  // world [n,3] -> [density [n] (= query_density), grad [n,3] = its analytic world-space gradient]
           [](ExpRunner& r, const Tensor& world) {
             py::gil_scoped_release no_gil;
             r.FinishPending();
             auto t = r.renderer_->QueryDensityGrad(world);
             return std::vector<Tensor>{std::get<0>(t), std::get<1>(t)};
           },
           py::arg("world"))
      .def("field_normals",  // world [n,3] -> unit normals [n,3] = -grad / |grad| of query_density_grad, 0 where that is 0 or not finite
           [](ExpRunner& r, const Tensor& world) {
             py::gil_scoped_release no_gil;
             r.FinishPending();
             return r.renderer_->FieldNormals(world);
           },
           py::arg("world"))
      .def("render_geometry",  // render_rays plus geometry buffers (f2n_composite_geometry): a dict, see README "world-space queries"
           [](ExpRunner& r, const Tensor& ro, const Tensor& rd, const Tensor& b, float tau, bool return_samples) {
             GeometryResult g;
             {
               py::gil_scoped_release no_gil;
               g = r.RenderGeometry(ro, rd, b, tau, return_samples);
             }
             py::dict d;
             d["colors"] = g.render.colors; d["disparity"] = g.render.disparity; d["depth"] = g.render.depth;
             d["opacity"] = g.opacity; d["normals"] = g.normals;
             d["surf_idx"] = g.surf_idx; d["surf_t"] = g.surf_t; d["surf_points"] = g.surf_points; d["surf_normals"] = g.surf_normals;
             if (return_samples) {
               const bool none = !g.render.weights.defined();  // (no ray met the scene)
               d["pts"] = g.pts; d["anchors"] = g.anchors; d["t"] = g.t; d["dt"] = g.dt;
               d["weights"] = none ? torch::empty({0}, DevF32()) : g.render.weights;
               d["idx_start_end"] = none ? torch::zeros({g.opacity.size(0), 2}, DevI32()) : g.render.idx_start_end;
               d["sample_grad"] = g.sample_grad; d["sample_normals"] = g.sample_normals;
             }
             return d;
           },
           py::arg("rays_o"), py::arg("rays_d"), py::arg("bounds"), py::arg("tau") = 0.5f, py::arg("return_samples") = false)
      .def_property("density_slab_points",  // points per z-slab of density_grid (bounds its workspaces)
                    [](ExpRunner& r) { return r.renderer_->density_slab_points_; },
                    [](ExpRunner& r, int64_t n) { r.renderer_->density_slab_points_ = std::max<int64_t>(1, n); })
      .def("attach_data_parallel",  // native RCCL exchanges, issued from C++ inside TrainStep (DataParallel.h); collective
           [](ExpRunner& r, int rank, int world, const py::bytes& unique_id, bool overlap, bool hooks_for_one_rank) {
             std::string s = unique_id;
             auto dp = std::make_shared<DataParallel>();
             {
               py::gil_scoped_release no_gil;
               dp->Attach(&r, rank, world, std::vector<uint8_t>(s.begin(), s.end()), overlap, hooks_for_one_rank);
             }
             r.data_parallel_ = dp;
           },
           py::arg("rank"), py::arg("world"), py::arg("unique_id"), py::arg("overlap") = true, py::arg("hooks_for_one_rank") = false)
      .def("dp_bucket_callbacks",  // table-gradient ranges the scatter reported while it ran (bucketed exchange, DataParallel.h)
           [](ExpRunner& r) { return r.data_parallel_ ? std::static_pointer_cast<DataParallel>(r.data_parallel_)->BucketCallbacks() : (int64_t) 0; })
      .def("dp_small_exchanges_early",  // steps whose small gradient buffers were exchanged beside the scatter (DataParallel::SmallGradsExchange)
           [](ExpRunner& r) { return r.data_parallel_ ? std::static_pointer_cast<DataParallel>(r.data_parallel_)->SmallExchangesEarly() : (int64_t) 0; })
      .def("dp_enable_timing",  // bracket every gradient exchange / every wait for it with timing events (DataParallel::EnableTiming)
           [](ExpRunner& r, bool on) { if (r.data_parallel_) std::static_pointer_cast<DataParallel>(r.data_parallel_)->EnableTiming(on); })
      .def("dp_collect_timing",  // [exchanges, exchange ms total, waits, exposed wait ms total] since the last call (synchronises)
           [](ExpRunner& r) { return r.data_parallel_ ? std::static_pointer_cast<DataParallel>(r.data_parallel_)->CollectTiming() : std::vector<double>{0, 0, 0, 0}; })
      .def("dp_comm_ranks",  // ranks of the native RCCL communicator as RCCL reports them (0: none attached)
           [](ExpRunner& r) { return r.data_parallel_ ? std::static_pointer_cast<DataParallel>(r.data_parallel_)->CommRanks() : 0; })
      .def("set_occupancy_sync_hook",  // all-reduce(MAX) of the per-node votes so that every replica prunes identically
           [](ExpRunner& r, py::function f) {
             SamplerOf(r)->occupancy_sync_hook_ = [f](Tensor occ) {
               py::gil_scoped_acquire g;
               f(occ);
             };
           })
      .def_static("host_profile",  // on=True: start (cleared); on=False: stop and return {region: (entries, seconds)} of the host thread
                  [](bool on) {
                    auto& hp = HostProf::Get();
                    py::dict d;
                    for (auto& kv : hp.acc) d[py::str(kv.first)] = py::make_tuple(kv.second.first, kv.second.second);
                    hp.acc.clear();
                    hp.on = on;
                    return d;
                  })
#if F2N_DEBUG_BUILD
      .def_static("debug_side_delay",  // spin kernels (us) in front of every period-th speculative begin / completion / step: a race amplifier
                  [](int begin_us, int complete_us, int main_us, int period, unsigned pollute) {
                    Renderer::SetDebugSideDelay(begin_us, complete_us, main_us, period, pollute);
                  },
                  py::arg("begin_us"), py::arg("complete_us"), py::arg("main_us"), py::arg("period"), py::arg("pollute") = 0u)
#endif
      .def_static("enable_kernel_timing", [](const std::vector<std::string>& names) { KernelTimers::Get().Enable(names); })
      .def_static("disable_kernel_timing", []() { KernelTimers::Get().Disable(); })
      .def_static("collect_kernel_timing",
                  []() {
                    py::dict d;
                    for (auto& kv : KernelTimers::Get().Collect()) d[py::str(kv.first)] = py::make_tuple(kv.second.first, kv.second.second);
                    return d;
                  })
      .def("install_octree", [](ExpRunner& r, const Tensor& n, const Tensor& t, const Tensor& e) { SamplerOf(r)->InstallOctree(n, t, e); })
      .def("set_edge_pool",[](ExpRunner& r, const Tensor& e) { SamplerOf(r)->SetEdgePool(e); })
      .def("set_train_cameras", [](ExpRunner& r, const Tensor& w2c, const Tensor& intri, const Tensor& b) { SamplerOf(r)->SetTrainCameras(w2c, intri, b); })
      .def("set_forced_randoms",
           [](ExpRunner& r, const Tensor& noise, const Tensor& bg, const Tensor& edge_idx, const Tensor& edge_coords) {
             SamplerOf(r)->forced_noise_ = noise;
             r.renderer_->forced_bg_ = bg;
             SamplerOf(r)->forced_edge_idx_ = edge_idx;
             SamplerOf(r)->forced_edge_coords_ = edge_coords;
           })
      .def("clear_forced_randoms",
           [](ExpRunner& r) {
             SamplerOf(r)->forced_noise_ = Tensor(); r.renderer_->forced_bg_ = Tensor();
             SamplerOf(r)->forced_edge_idx_ = Tensor(); SamplerOf(r)->forced_edge_coords_ = Tensor();
           })
      .def("n_nodes", [](ExpRunner& r) { return SamplerOf(r)->pers_octree_->n_nodes_; })
      .def("proc_octree", [](ExpRunner& r, bool compact, bool subdivide, bool brute) { SamplerOf(r)->pers_octree_->ProcOctree(compact, subdivide, brute); })
      .def("tree_nodes", [](ExpRunner& r) { return SamplerOf(r)->pers_octree_->tree_nodes_gpu_; })
      .def("cur_batch_size", &ExpRunner::CurBatchSize)
      .def("batch_size_for", &ExpRunner::BatchSizeFor)  // ray count of the batch with that sequence number (fixed-lag average)
      .def_property("step_seq",  // training steps taken = the sequence number the next step's draws are keyed by (KeyedDraws.h)
                    [](ExpRunner& r) { return r.step_seq_; }, [](ExpRunner& r, int64_t s) { r.ResetStepSequence(s); })
      .def_readwrite("digest_table", &ExpRunner::digest_table_)
      .def_property("digest_taps",  // per-step checksums of the step's intermediate arrays (Renderer::DigestTap; debugging)
                    [](ExpRunner& r) { return r.renderer_->digest_taps_; }, [](ExpRunner& r, bool on) { r.renderer_->digest_taps_ = on; })
      .def("step_taps",  // int64 [steps, 1 + N_TAPS]: seq, then the taps (pts, dt, anchors, f0, survivors, bg, edge, colours, table grad,
           [](ExpRunner& r) {  // small grads, table, field MLP, colour MLP, app_emb), oldest first
             r.FinishPending();
             std::vector<int64_t> seqs;
             for (auto& d : r.renderer_->digest_) if (d.seq >= 0) seqs.push_back(d.seq);
             std::sort(seqs.begin(), seqs.end());
             Tensor out = torch::zeros({(int64_t) seqs.size(), 1 + Renderer::N_TAPS}, torch::kInt64);
             if (!r.renderer_->digest_tap_sums_.defined()) return out;
             Tensor sums = r.renderer_->digest_tap_sums_.cpu();
             for (size_t i = 0; i < seqs.size(); i++) {
               out[i][0] = seqs[i];
               out[i].narrow(0, 1, Renderer::N_TAPS).copy_(sums[seqs[i] % Renderer::kDigestRing]);
             }
             return out;
           })
      .def("step_digest",  // the last steps' (seq, iter, rays, marched, kept[, table checksum]), oldest first (flushes)
           [](ExpRunner& r) {
             r.FinishPending();
             py::list out;
             auto& dg = r.renderer_->digest_;
             Tensor sums = r.digest_table_sums_.defined() ? r.digest_table_sums_.cpu() : Tensor();
             std::vector<Renderer::StepDigest> rows;
             for (auto& d : dg) if (d.seq >= 0) rows.push_back(d);
             std::sort(rows.begin(), rows.end(), [](const Renderer::StepDigest& a, const Renderer::StepDigest& b) { return a.seq < b.seq; });
             for (auto& d : rows) {
               py::list row;
               row.append(d.seq); row.append(d.iter); row.append(d.n_rays); row.append(d.n_marched); row.append(d.n_kept);
               if (sums.defined()) row.append(sums.data_ptr<int64_t>()[d.seq % Renderer::kDigestRing]);
               out.append(row);
             }
             return out;
           })
      .def_readwrite("iter_step", &ExpRunner::iter_step_)
      .def_readwrite("check_nan", &ExpRunner::check_nan_)
      .def_readwrite("async_counts", &ExpRunner::async_counts_)
      .def_property("speculative_sampling",  // 0 / False never, 1 / True always, 2 while no leaf has died lately (default)
                    [](ExpRunner& r) { return r.renderer_->speculative_sampling_; },
                    [](ExpRunner& r, int mode) { r.renderer_->speculative_sampling_ = mode; })
      .def_property("tail_repair",  // speculative batches repaired by list compaction + a march of the tail behind the first dead leaf (A/B knob)
                    [](ExpRunner& r) { return static_cast<PersSampler*>(r.renderer_->pts_sampler_.get())->tail_repair_; },
                    [](ExpRunner& r, bool on) { static_cast<PersSampler*>(r.renderer_->pts_sampler_.get())->tail_repair_ = on; })
      .def_readwrite("fused_tail", &ExpRunner::fused_tail_)
      .def_property("prepass_feat_reuse",  // streaming steps: grad pass from the pre-pass's field outputs, field backward on the cache rows (A/B: False = field_shade_fwd + field_x copy)
                    [](ExpRunner& r) { return r.renderer_->prepass_feat_reuse_; },
                    [](ExpRunner& r, bool on) { r.renderer_->prepass_feat_reuse_ = on; })
      .def_property("prepass_planes_cache",  // with reuse: the pre-pass keeps the gather's planes as its feature cache, no row copy (A/B: False = rows, the _rows calls)
                    [](ExpRunner& r) { return r.renderer_->prepass_planes_cache_; },
                    [](ExpRunner& r, bool on) { r.renderer_->prepass_planes_cache_ = on; })
      .def_property("votes_off_main",  // occupancy votes + stat update on the tail stream, early stop and survivor scan alone on the main queue: 0 never (the fused launches), 1 every eligible step, 2 eligible steps of the one-batch-ahead regime
                    [](ExpRunner& r) { return r.renderer_->votes_off_main_; },
                    [](ExpRunner& r, int mode) {
                      if (mode < 0 || mode > 2) throw std::invalid_argument("votes_off_main: 0, 1 or 2");
                      r.renderer_->votes_off_main_ = mode;
                    })
      .def_property_readonly("votes_off_main_steps", [](ExpRunner& r) { return r.renderer_->n_votes_off_main_steps_; })  // steps that took that route
      .def_property_readonly("prepass_reuse_steps", [](ExpRunner& r) { return r.renderer_->n_feat_reuse_steps_; })  // steps that took that path
      .def_property("scatter_producer",  // f2n_set_scatter_producer: 1 = hash constants in LDS (default), 0 = the non-staged instantiation (A/B knob; per process)
                    [](ExpRunner&) { return g_scatter_producer; },
                    [](ExpRunner&, int variant) {
                      if (f2n_set_scatter_producer(variant) != F2N_OK) throw std::invalid_argument("scatter_producer: 0 or 1");
                      g_scatter_producer = variant;
                    })
      .def_readwrite("spec_start_without_event", &ExpRunner::spec_start_without_event_)
      .def_readwrite("draws_off_main", &ExpRunner::draws_off_main_)  // ExpRunner::Train's batch draws on the tail stream (A/B: False = main queue)
      .def_readwrite("exact_flag_order", &ExpRunner::exact_flag_order_)  // the step's tail inside the field backward's call (A/B: False = separate launches)
      .def_property("march_block_waves",  // workgroup size of the persistent march, in waves (1..16)
                    [](ExpRunner& r) { return static_cast<PersSampler*>(r.renderer_->pts_sampler_.get())->march_block_waves_; },
                    [](ExpRunner& r, int n) { static_cast<PersSampler*>(r.renderer_->pts_sampler_.get())->march_block_waves_ = std::min(16, std::max(1, n)); })
      .def_property("march_blocks",  // > 0: speculative batches marched on that many persistent one-wave blocks (0: one block per 4 rays)
                    [](ExpRunner& r) { return static_cast<PersSampler*>(r.renderer_->pts_sampler_.get())->march_blocks_; },
                    [](ExpRunner& r, int n) { static_cast<PersSampler*>(r.renderer_->pts_sampler_.get())->march_blocks_ = std::max(0, n); })
      .def_property("speculation_depth",  // the batch after next is begun two steps ahead: 1 never, 2 once the octree has outgrown the LDS walk, 3 always
                    [](ExpRunner& r) { return r.renderer_->spec_depth_; },
                    [](ExpRunner& r, int d) { r.FinishPending(); r.renderer_->DropPendingSamples(); r.renderer_->spec_depth_ = std::max(1, std::min(3, d)); })
      .def("speculation_counters",  // batches sampled ahead of the stat update / behind it, rays repaired after a leaf died
           [](ExpRunner& r) {
             r.FinishPending();
             py::dict d;
             d["speculative"] = r.renderer_->n_speculative_;
             d["fallback"] = r.renderer_->n_spec_fallback_;
             d["dropped"] = r.renderer_->n_spec_dropped_;
             auto& o = *SamplerOf(r)->pers_octree_;
             d["rays_repaired"] = o.n_repaired_.defined() ? o.n_repaired_.item<int>() : 0;
             d["stat_updates"] = o.epoch_;
             return d;
           })
      .def("counters",  // running totals over training-mode steps; flushes (the last streaming step's count is still in flight)
           [](ExpRunner& r) {
             r.FinishPending();
             py::dict d;
             d["total_meaningful"] = r.renderer_->total_kept_pts_;
             d["total_marched"] = r.renderer_->total_all_pts_;
             return d;
           })
      .def_readonly("cur_lr", &ExpRunner::cur_lr_)
      .def_property("n_edge_pts", [](ExpRunner& r) { return r.renderer_->n_edge_pts_; }, [](ExpRunner& r, int n) { r.renderer_->n_edge_pts_ = n; })
      .def_property_readonly("fineness", [](ExpRunner& r) { return r.global_data_pool_->ray_march_fineness_; })
      .def_property_readonly("oct_per_ray", [](ExpRunner& r) { return r.global_data_pool_->sampled_oct_per_ray_; })
      .def_property_readonly("sampled_per_ray", [](ExpRunner& r) { return r.global_data_pool_->sampled_pts_per_ray_; })
      .def_property_readonly("meaningful_per_ray", [](ExpRunner& r) { return r.global_data_pool_->meaningful_sampled_pts_per_ray_; })
      .def_property_readonly("n_volumes", [](ExpRunner& r) { return r.global_data_pool_->n_volumes_; })
      .def("update_ada_params", &ExpRunner::UpdateAdaParams);
}
