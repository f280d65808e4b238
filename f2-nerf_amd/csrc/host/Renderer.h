// SHShader + Renderer host side (mirror src/Shader/SHShader.h, src/Renderer/Renderer.h).
#pragma once
#include "Hash3DAnchored.h"
#include "PersSampler.h"

namespace f2n {

class SHShader : public Shader {
 public:
  explicit SHShader(GlobalDataPool* global_data_pool);
  Tensor Query(const Tensor& feats, const Tensor& dirs) override;  // feats = the 16 shading features, dirs [n,3]
  // The Renderer's path: feats are the RAW field features [n,16]; the "[1 | feat[1:]] + app_emb[img]" assembly of
  // Renderer.cpp:181-187 happens inside the kernel.  sample_emb_idx/app_emb may be undefined.
  Tensor QueryFromField(const Tensor& field_feats, const Tensor& dirs, const Tensor& app_emb, const Tensor& sample_emb_idx,
                        Tensor* app_emb_grad);
  Tensor SHEncode(const Tensor& dirs);
  std::vector<Tensor> States() override;
  std::vector<ParamGroup> OptimParamGroups() override;
  int LoadStates(const std::vector<Tensor>& states, int idx) override;
  void Reset() override;

  std::unique_ptr<FusedMLP> mlp_;
  int d_hidden_, n_hiddens_, degree_;
  // the fused SH + colour-MLP kernels exist for the shipped shader (SH degree 4, 32 -> 64 -> 64 -> 3); any other
  // shader.degree / d_hidden / n_hiddens (confs/shader/sh_shader.yaml, SHShader.cu:51-102) runs op by op as SHShader.cpp:23-29
  bool fused_ok_ = true;
};

struct RenderResult {  // Renderer.h:18-27 of the reference
  Tensor colors;
  Tensor first_oct_dis;
  Tensor disparity;
  Tensor edge_feats;
  Tensor depth;
  Tensor weights;
  Tensor idx_start_end;
  Tensor dt;  // [M]: the warped step lengths of the surviving samples (what compositing integrates over; CustomOps::Distortion)
};

// Everything Render() knows after sampling, pre-pass, early stop, compaction and the occupancy update.
struct RenderFront {
  bool empty = false;        // no sample at all (Renderer.cpp:83-97)
  SampleResultFlex es;       // surviving samples
  Tensor pts_all, vol_all;   // [M + 2E] surviving samples followed by the edge (TV) samples
  Tensor src_rows;           // row of every surviving sample in the pre-pass feature cache
  Tensor bg_color, sample_emb_idx;
  int n_kept = 0, n_edge = 0;
  bool emb = false;
  // Streaming training steps do not wait for the survivor count: n_kept is then an UPPER BOUND (the marched count, which
  // sizes every buffer), the true count stays on the device (n_kept_dev, consumed by the f2n_*_dyn entry points) and the edge
  // samples come FIRST in pts_all / vol_all so that every row offset is known without it.
  bool dyn = false;
  Tensor n_kept_dev;
  // >= 0: the edge samples went through the density pre-pass; their hash features are rows [edge_cache_row, +2E) of its cache
  int64_t edge_cache_row = -1;
  int64_t sample_cache_row = 0;  // cache row of ray sample 0 (src_rows count from there)
  // pts_all / vol_all / bg_color came out of a side stream's allocator pool (Renderer::PreGenerateStepDraws) and are read by the
  // step's LAST kernels (compositing, the scatter): the device's `consumed` event is recorded once more behind those
  bool side_pool_buffers = false;
  // Streaming training steps (round 6, one event packet less on the main queue): the pre-early-stop sample buffers -- side-stream
  // pool memory as well -- stay alive in here until the step's last kernel has been queued, and ONE recording of the `consumed`
  // event behind that kernel covers them and the buffers above (an event recorded between two kernels of a stream costs the
  // command processor ~5 us: profiles/r06_event_cost.txt).
  SampleResultFlex presamples_keepalive;
  bool consumed_deferred = false;
  // Votes off the main queue (Renderer::votes_off_main_): the tail stream's vote walk reads the pre-early-stop bounds / anchors
  // (presamples_keepalive) and the early stop's weights / alphas, main-stream allocations held here.  TrainForwardBackward makes the
  // main stream wait for the tail stream's update before it records `consumed` and before any of these is released.
  Tensor votes_weights, votes_alphas;
  bool votes_deferred = false;
  // The same wait for a step that does not get that far (an exception between SampleAndFilter and TrainForwardBackward's join): its
  // deleter runs Renderer::JoinTailVotes().  Declared behind the tensors above, so destroyed -- and the main stream ordered -- first.
  std::shared_ptr<void> votes_join;
};

// The implicit grid of Renderer::DensityGrid: point (ix, iy, iz) = lo + step * i (f2n_oct_locate_warp_grid), n[k] points along axis k.
// step = (longest side of the box) / res, so that the longest side has res cells; n[k] = round(extent_k / step) + 1 (at least 2).
struct GridSpec {
  float lo[3];
  float step;
  int n[3];
};
// Iso-surface of any float32 grid [nz, ny, nx] (f2n_mesh_count / f2n_mesh_emit): (verts [V,3] f32, faces [F,3] int32)
std::tuple<Tensor, Tensor> MeshFromGrid(const Tensor& grid, float level, const float lo[3], float step);
// The same with a uint8 mask [nz, ny, nx] of the grid points that carry a value (f2n_mesh_count_masked): faces only from cells whose
// eight corners are valid, vertices only where a face uses them
std::tuple<Tensor, Tensor> MeshFromGridMasked(const Tensor& grid, const Tensor& valid, float level, const float lo[3], float step);
// Sparse meshing on bricks of B^3 cells of the virtual grid (lo, step, n = (nx, ny, nz)); include/f2n_abi.h, "Sparse mesh extraction
// on bricks".  std::invalid_argument: B outside {4, 8, 16}, a grid of 2^31 bricks or more, a brick id outside the grid or listed twice,
// a brick list that lacks the owner of a face's vertex, more than 2^31 - 1 vertices or faces.
// BrickMark: flags [nbz, nby, nbx] uint8 of f2n_brick_mark for the octree records tree_nodes (uint8, 64 B per node).
Tensor BrickMark(const Tensor& tree_nodes, const float lo[3], float step, const int n[3], int B);
// One batch of listed bricks through f2n_brick_mesh_count -> cumsum (int64) -> f2n_brick_mesh_emit: keyed vertices and faces
struct BrickMeshPart {
  Tensor vert_keys, verts, face_keys, face_vert_keys;  // [nv] int64, [nv,3] f32, [nf] int64, [nf,3] int64
  int64_t meshed_bricks = 0;                           // bricks of the batch that own a vertex or a face
};
// valid: undefined = f2n_brick_mesh_count / _emit, else the device uint8 rows [n_bricks, (B+1)^3] of the masked entry points
BrickMeshPart BrickMeshBatch(const Tensor& values, const Tensor& brick_ids, const int n[3], const float lo[3], float step, float level, int B,
                             const Tensor& valid = Tensor());
// The parts as one mesh in f2n_mesh_emit's order: vertices sorted by key, faces = searchsorted(sorted keys, face_vert_keys) as int32,
// sorted by face key.  drop_unreferenced (the masked mesher): the vertices no face names are compacted away, order kept, faces remapped
std::tuple<Tensor, Tensor> BrickMeshAssemble(const std::vector<BrickMeshPart>& parts, bool drop_unreferenced = false);
// (verts, faces) of values [n_bricks, (B+1)^3] for brick_ids [n_bricks] (any order, each id once); batch_bricks > 0: in batches of
// that many bricks (the same mesh)
std::tuple<Tensor, Tensor> MeshFromBricks(const Tensor& values, const Tensor& brick_ids, const int n[3], const float lo[3], float step,
                                          float level, int B, int64_t batch_bricks = 0);
// TSDF fusion on any grid (f2n_tsdf_integrate / f2n_tsdf_finalize).  TsdfIntegrate adds depth [V,h,w] (conf [V,h,w] or undefined) seen
// from poses [V,3,4] / intri [V,3,3] / dist [V,4] into the device tensors S, W [nz, ny, nx] IN PLACE; TsdfFinalize: (g, valid uint8).
void TsdfIntegrate(const Tensor& S, const Tensor& W, const float lo[3], float step, const Tensor& poses, const Tensor& intri,
                   const Tensor& dist, const Tensor& depth, const Tensor& conf, float trunc);
std::tuple<Tensor, Tensor> TsdfFinalize(const Tensor& S, const Tensor& W, float min_weight);
// Sparse TSDF fusion on bricks (include/f2n_abi.h, "Sparse TSDF fusion on bricks"); the views as TsdfIntegrate takes them.
// TsdfBrickMark: flags [nbz, nby, nbx] uint8 of f2n_tsdf_brick_mark (all zero without views).  TsdfIntegrateBricks: the device rows S, W
// [n_bricks, (B+1)^3] of brick_ids (checked as MeshFromBricks checks them) IN PLACE.  MeshFromBricksMasked: MeshFromBricks through the
// masked entry points, then without the vertices no face names -- MeshFromGridMasked's mesh when the list holds the owner of every face.
Tensor TsdfBrickMark(const float lo[3], float step, const int n[3], int B, const Tensor& poses, const Tensor& intri, const Tensor& dist,
                     const Tensor& depth, const Tensor& conf, float trunc);
void TsdfIntegrateBricks(const Tensor& S, const Tensor& W, const Tensor& brick_ids, const float lo[3], float step, const int n[3], int B,
                         const Tensor& poses, const Tensor& intri, const Tensor& dist, const Tensor& depth, const Tensor& conf, float trunc);
std::tuple<Tensor, Tensor> MeshFromBricksMasked(const Tensor& values, const Tensor& valid, const Tensor& brick_ids, const int n[3],
                                                const float lo[3], float step, float level, int B, int64_t batch_bricks = 0);
// View-colour fusion (f2n_view_colors_accumulate / f2n_view_colors_finalize); the views as TsdfIntegrate takes them, image [V,h,w,C] on
// the pixel grid of depth.  ViewColorsAccumulate adds the views' observations of points [n,3] (normals [n,3] or undefined) to the device
// tensors acc [n,C], wsum [n], count [n] int32 IN PLACE; ViewColorsFinalize: (rgb [n,C], known [n] uint8).
void ViewColorsAccumulate(const Tensor& acc, const Tensor& wsum, const Tensor& count, const Tensor& points, const Tensor& normals,
                          const Tensor& poses, const Tensor& intri, const Tensor& dist, const Tensor& depth, const Tensor& conf,
                          const Tensor& image, float tol, float cos_min);
std::tuple<Tensor, Tensor> ViewColorsFinalize(const Tensor& acc, const Tensor& wsum, const Tensor& count, int min_views);
// mark -> the flagged bricks in ascending order in batches of batch_bricks -> zeroed rows, TsdfIntegrateBricks over all views,
// TsdfFinalize, one masked mesh batch -> assemble: the mesh of TsdfIntegrate -> TsdfFinalize -> MeshFromGridMasked at level 0, bit for
// bit, with one batch of rows alive at a time
struct SparseTsdfStats {
  int64_t bricks = 0, active_bricks = 0, meshed_bricks = 0, points_evaluated = 0, points_known = 0, batches = 0;
  int grid[3] = {0, 0, 0};
};
std::tuple<Tensor, Tensor> TsdfMeshSparse(const float lo[3], float step, const int n[3], int B, const Tensor& poses, const Tensor& intri,
                                          const Tensor& dist, const Tensor& depth, const Tensor& conf, float trunc, float min_weight,
                                          int64_t batch_bricks, SparseTsdfStats* stats = nullptr);
// Unit normals [n,3] at pts [n,3] from the gradient of any float32 grid [nz, ny, nx] (f2n_grid_normals): -grad / |grad|, 0 where flat
Tensor GridNormals(const Tensor& grid, const Tensor& pts, const float lo[3], float step);
// labels [V] int32: the smallest vertex index of every vertex's connected component (f2n_mesh_components); *rounds: labelling rounds
Tensor MeshComponents(const Tensor& faces, int64_t n_verts, int* rounds = nullptr);
// The mesh without the components of fewer than min_faces faces, order kept (f2n_mesh_filter_count / _emit): (verts, faces re-indexed,
// vert_src [V'] int32 = the original index of every kept vertex).  min_faces <= 1: the input itself and the identity.
std::tuple<Tensor, Tensor, Tensor> MeshFilterComponents(const Tensor& verts, const Tensor& faces, int min_faces);
// Vertex clustering with quadric-error placement on the grid of origin lo (NULL: the minimum of the finite coordinates) and cell size
// `cell` (f2n_mesh_cluster_*): (verts, faces, vert_map [V] int32 = the output vertex of every input vertex or -1).  One output
// vertex per occupied cell, collapsed faces dropped, duplicates merged, faces sorted; lambda ties a vertex to its cluster's mean.
std::tuple<Tensor, Tensor, Tensor> MeshSimplify(const Tensor& verts, const Tensor& faces, float cell, const float* lo, double lambda);

// Ray casting against a triangle mesh (f2n_mesh_raycast*; include/f2n_abi.h states the test rounding by rounding).  The accel is a
// uniform grid of face lists that covers the mesh: lo (NULL: the minimum of the finite coordinates; given: it must not lie above it),
// cell (NaN: MeshRaycastDefaultCell), dims, cell_start [ncells + 1] and cell_faces [E] int32.  std::invalid_argument for a grid
// that does not cover the mesh, holds more than 2^27 cells or 2^31 entries, and for rays outside the traversal's domain.
struct MeshRaycastAccel {
  float lo[3] = {0.f, 0.f, 0.f}, cell = 1.f;
  int32_t dims[3] = {1, 1, 1};
  Tensor cell_start, cell_faces;
};
// The default cell: sqrt(10 A / F) with A the area of the vertices' bounding box -- about ten faces per occupied cell if the surface
// had the box's area -- and at least 1/500 of the box's longest side; 1 for an empty or flat box.  A heuristic, not measured on a
// trained scene.
float MeshRaycastDefaultCell(const float mn[3], const float mx[3], int64_t n_faces);
MeshRaycastAccel MeshRaycastBuild(const Tensor& verts, const Tensor& faces, float cell, const float* lo);
// (t [R], face [R] int32 (-1: none), bary [R,3]) of the rays' first hit inside their window bounds [R,2] (undefined: (0, inf));
// accel NULL: the brute-force mode, every ray against every face
std::tuple<Tensor, Tensor, Tensor> MeshRaycast(const Tensor& verts, const Tensor& faces, const MeshRaycastAccel* accel, const Tensor& rays_o,
                                               const Tensor& rays_d, const Tensor& bounds);

// Mesh-to-mesh distance (f2n_mesh_closest_point, f2n_mesh_face_weights, f2n_mesh_sample_surface; include/f2n_abi.h states both).
// (dist [N] (+inf: none within max_dist), face [N] int32 (-1: none), bary [N,3]) of the points' closest point on the mesh; accel NULL:
// the brute-force mode.  The accel is MeshRaycastBuild's, unchanged.  The points are processed in the caller's order (sorting them
// by grid cell first was measured and bought nothing: DESIGN.md section 3).  std::invalid_argument for a finite point more than 2^15
// cells from the frame's origin and for a max_dist that is negative or NaN.
std::tuple<Tensor, Tensor, Tensor> MeshClosestPoint(const Tensor& verts, const Tensor& faces, const MeshRaycastAccel* accel, const Tensor& points,
                                                    float max_dist);
// (points [n,3], face [n] int32, bary [n,3]): n area-uniform, stratified samples of the surface, a pure function of (mesh, n, seed).
// std::invalid_argument for a mesh without area and for n < 0.
constexpr uint64_t kMeshSamplePurpose = 0x8CB92BA72F3D8DD7ull;  // the key of the samples' Philox draws is seed ^ this (KeyedDraws.h)
std::tuple<Tensor, Tensor, Tensor> MeshSampleSurface(const Tensor& verts, const Tensor& faces, int64_t n, uint64_t seed);

// Texture atlas of a mesh (f2n_atlas_*; include/f2n_abi.h states the layout): one right-triangle chart per face, two to a power-of-two
// block, blocks placed by the Morton decode of the prefix sum of their areas.  density = texels per length unit; while the atlas is
// wider than max_size (a power of two) the density is halved, at most 32 times.  std::invalid_argument for a max_size that is no
// power of two and for a mesh that cannot fit.
struct MeshAtlasResult {
  Tensor uv;                              // [F,3,2] fp32, image convention, per face corner
  int size = 4;                           // the atlas side
  float density_used = 0.f;
  Tensor offsets, block_log, block_faces; // [B+1] int64, [B] int32, [B,2] int32 (lower, upper; -1: empty)
  Tensor log_s, rot, slot;                // [F] int32 each; slot = 2 block + upper; bit 2 of rot flags a degenerate face
};
MeshAtlasResult MeshAtlas(const Tensor& verts, const Tensor& faces, float density, int max_size, int max_log);
// (tex_face [S,S] int32 (-1: unowned), tex_bary [S,S,3], tex_pos [S,S,3]): the face, weights and position of every texel; clamp: gutter
// texels replicate the nearest edge instead of extrapolating.  Reads a's size, offsets, block_log, block_faces and rot.
std::tuple<Tensor, Tensor, Tensor> MeshAtlasTexels(const Tensor& verts, const Tensor& faces, const MeshAtlasResult& a, bool clamp);
// [N,C]: the bilinear lookup of tex [S,S,C] at uv [N,2] (texel centres at (i + 0.5) / S, clamped to the edge; f2n_texture_sample)
Tensor TextureSample(const Tensor& tex, const Tensor& uv);
// SSIM of two float32 [H,W,C] images (the reference's rgb_ssim, scripts/eval.py:29-75; f2n_ssim_window + f2n_image_ssim, include/f2n_abi.h
// states every rounding): c1 = (k1 max_val)^2, c2 = (k2 max_val)^2 in fp64; mean = sum_c stats[c][0] / (2^36 oh ow C) and per_channel [C]
// (fp64, on the host) = stats[c][0] / (2^36 oh ow), each NaN if a count of finite values falls short of oh ow (np.mean of the reference's
// map); map [oh,ow,C] fp64 on the device, undefined unless asked for.  Reads the statistics back: it synchronises the stream.
std::tuple<double, Tensor, Tensor> ImageSSIM(const Tensor& a, const Tensor& b, double max_val = 1.0, int filter_size = 11, double sigma = 1.5,
                                             double k1 = 0.01, double k2 = 0.03, bool return_map = false);

// Mesh refinement (f2n_mesh_ring_*, f2n_mesh_smooth, f2n_mesh_move_clamp, f2n_level_step, f2n_mesh_face_quality; include/f2n_abi.h
// states every rounding).  The one-ring of every vertex as a CSR: start_end [V,2] int32, ring [E] int32 (neighbours ascending, each
// once), pinned [V] uint8 (on a boundary or non-manifold edge, or used by no face), edge_counts [2] int32 on the device (edges used by
// one face, by three or more).  The sort of the directed-edge keys is a torch op; reads back one index.
struct MeshRingResult {
  Tensor start_end, ring, pinned, edge_counts;
};
MeshRingResult MeshRing(const Tensor& faces, int64_t n_verts);
// `passes` Taubin pairs (a pass with lam, a pass with mu) over the ring, pinned vertices copied through; then, for a finite max_move,
// the clamp of every vertex to the ball of that radius around its input position.  std::invalid_argument for passes < 0, a lam or mu
// that is not finite, max_move <= 0 or NaN.
Tensor MeshSmooth(const Tensor& verts, const Tensor& faces, int passes, double lam, double mu, float max_move);
Tensor MeshSmoothOnRing(const Tensor& verts, const MeshRingResult& ring, int passes, double lam, double mu, float max_move);
// [F] float64: 4 sqrt(3) area / (sum of the squared edge lengths); 0 for a degenerate or invalid face, NaN where a coordinate is not finite
Tensor MeshFaceQuality(const Tensor& verts, const Tensor& faces);
// f2n_level_step on the caller's device arrays, the state (cand .. evals) in place
void LevelStep(bool first, bool propose, const Tensor& p0, const Tensor& sigma, const Tensor& grad, const Tensor& h, float tol, float max_step,
               float max_move, const Tensor& cand, const Tensor& best, const Tensor& h_best, const Tensor& g_best, const Tensor& scale,
               const Tensor& status, const Tensor& evals);

// Renderer::ProjectToLevel: per point the position, ln(sigma / level) at the start and at the end, the status bits and the number of
// field evaluations it used
struct LevelProjection {
  Tensor points, h_in, h_out, status, evals;
};

// the refine stage of Renderer::ExtractMeshAttrs; max_*_steps in grid steps (times simplify when simplify >= 2)
struct MeshRefineOptions {
  bool on = false;
  int smooth_passes = 2;
  double lam = 0.5, mu = -0.53;
  bool project = true;
  int iters = 8;
  float max_step_steps = 0.5f, max_move_steps = 1.0f, tol = 1e-3f;
};

struct SparseMeshStats {  // Renderer::ExtractMeshSparse
  int64_t bricks = 0, active_bricks = 0, meshed_bricks = 0;  // of the grid; flagged by BrickMark; owning a vertex or a face
  int64_t points_evaluated = 0, points_nonempty = 0;         // existing corners of the active bricks' rows; those in a live leaf
  int64_t batches = 0;
  int grid[3] = {0, 0, 0};                                   // (nx, ny, nz) of the virtual grid
};

struct MeshAttrs {  // Renderer::ExtractMeshAttrs; normals / colors are undefined unless asked for
  Tensor verts, faces, normals, colors;
  SparseMeshStats sparse;  // sparse > 0 only
  int64_t verts_in = -1, faces_in = -1;  // simplify >= 2: the size of the mesh that went into MeshSimplify
  std::vector<std::pair<std::string, double>> refine;  // the refine stage's statistics, in order (empty: the stage was off)
};

// Renderer::RenderGeometry: RenderForward's result and the geometry buffers of f2n_composite_geometry
struct GeometryResult {
  RenderResult render;  // colors, disparity, depth, weights, idx_start_end: RenderForward's, bit for bit
  Tensor opacity, normals;                              // [R], [R,3]
  Tensor surf_idx, surf_t, surf_points, surf_normals;   // [R] int32 (-1: none), [R], [R,3], [R,3]
  // keep_samples only: the surviving samples ([M,3] warped, [M,3] int32, [M], [M]) and their J^T df0/dw / unit normals [M,3]
  Tensor pts, anchors, t, dt, sample_grad, sample_normals;
};

struct TrainOutputs {
  Tensor losses;  // device [8]: loss, color, var, disp, tv, mse, dist (0 unless dist_w > 0), 0 (f2n_train_loss, f2n_loss_add_mean)
  Tensor colors;
  bool has_samples = false;
};

class Renderer : public Pipe {
  enum BGColorType { white, black, rand_noise };

 public:
  Renderer(GlobalDataPool* global_data_pool, int n_images);
#if F2N_DEBUG_BUILD
  // debug variant only (see RendererPrefetch.cpp): spin kernels in front of every period-th speculative begin / completion / step
  static void SetDebugSideDelay(int begin_us, int complete_us, int main_us, int period, unsigned pollute = 0);
#endif
  static void DebugSkew(int which);  // 0 speculative begin, 1 completion, 2 step; a no-op in the product build
  RenderResult Render(const Tensor& rays_o, const Tensor& rays_d, const Tensor& bounds, const Tensor& emb_idx);
  RenderResult RenderForward(const Tensor& rays_o, const Tensor& rays_d, const Tensor& bounds);  // inference: no tape, no count read-back
  // issues the ray sampling of the next SampleAndFilter / TrainForwardBackward call ahead of time (same rays!)
  void PreSample(const Tensor& rays_o, const Tensor& rays_d, const Tensor& bounds);
  // The same on a SIDE stream that only waits for this step's octree update: the sampler kernels (latency-bound: few
  // waves, long dependent chains) then run underneath the remaining forward/backward kernels of the current step.
  void PreSampleAsync(const Tensor& rays_o, const Tensor& rays_d, const Tensor& bounds);
  // seq: the batch's sequence number in the training run (KeyedDraws.h: keys its march noise and its step's draws); < 0: unkeyed
  void PreSampleBegin(const Tensor& rays_o, const Tensor& rays_d, const Tensor& bounds, float fineness, int64_t seq = -1);
  // Batches whose sampling is in flight on a side stream: at most kPendingSlots of them (round 4: the batch the NEXT step
  // consumes, being repaired / packed, and the one behind it, being walked and marched -- see next2_batch_), each on its own
  // stream.  A batch is identified by the ray tensors it was begun for (held: see PresampleMatches).
  static constexpr int kPendingSlots = 2;
  struct PendingBatch {
    PendingSamples s;
    Tensor rays_o, rays_d;
    int64_t seq = -1;               // the batch's sequence number (keys its noise and the draws of the step that consumes it)
    bool step_draws_ready = false;  // PreGenerateStepDraws ran behind this batch's pack
    Tensor bg_color, pts_all, vol_all;
  };
  // the background colours and edge samples of the step that will consume pend_[slot], on that slot's side stream (behind its pack)
  void PreGenerateStepDraws(int slot);
  // The random draws a training step makes for itself (background colours, edge samples: Renderer.cpp:67-81, PersSampler.cu:456-457)
  // are keyed by the step's sequence number (KeyedDraws.h, as the march noise: PersSampler::BeginSamples): step k gets draw k
  // whether it is made at the top of that step or a step earlier on a side stream, once or -- after a dropped batch -- twice.
  KeyedUniforms step_draws_{0xD1B54A32D192ED03ull};
  Tensor DrawStepUniforms(int64_t n, int64_t seq) { return step_draws_.Draw(n, seq); }
  // The sequence number of the batch the running / next training-mode SampleAndFilter consumes: set by ExpRunner around every
  // step (its count of steps taken); -1: unkeyed (Render() called on its own: each call takes the next draw of every purpose).
  int64_t cur_seq_ = -1;
  PendingBatch pend_[kPendingSlots];
  int64_t n_spec_dropped_ = 0;  // batches begun ahead and thrown away (other rays asked for, tree replaced)
  int FindPending(const Tensor& rays_o, const Tensor& rays_d) const {
    for (int i = 0; i < kPendingSlots; i++)
      if (pend_[i].s.active && pend_[i].rays_o.defined() && pend_[i].rays_d.defined() && rays_o.defined() && rays_d.defined() &&
          rays_o.data_ptr() == pend_[i].rays_o.data_ptr() && rays_d.data_ptr() == pend_[i].rays_d.data_ptr() &&
          rays_o.sizes() == pend_[i].rays_o.sizes())
        return i;
    return -1;
  }
  int FreePendingSlot() const {
    for (int i = 0; i < kPendingSlots; i++)
      if (!pend_[i].s.active) return i;
    return -1;
  }
  void PreSampleFinish(int slot);
  bool PreSampleBegun() const { return pend_[0].s.active || pend_[1].s.active; }
  bool PendingMatches(const Tensor& rays_o, const Tensor& rays_d) const { return FindPending(rays_o, rays_d) >= 0; }
  void DropPendingSlot(int i) {
    if (!pend_[i].s.active) return;
    n_spec_dropped_++;
    pend_[i].s.counts_ready.synchronize();  // its kernels may still be running: keep the buffers until they are done
    if (!pend_[i].s.completed && side_[i]) side_[i]->synchronize();  // (a speculative batch has recorded no count event yet)
    pend_[i] = PendingBatch();
  }
  void DropPendingSamples() {
    for (int i = 0; i < kPendingSlots; i++) DropPendingSlot(i);
  }
  // drops every pending batch that was not begun for one of these ray pairs (undefined tensors match nothing)
  void KeepOnlyPending(const Tensor& o0, const Tensor& d0, const Tensor& o1, const Tensor& d1, const Tensor& o2, const Tensor& d2) {
    for (int i = 0; i < kPendingSlots; i++) {
      if (!pend_[i].s.active) continue;
      const int a = FindPending(o0, d0), b = FindPending(o1, d1), c = FindPending(o2, d2);
      if (i != a && i != b && i != c) DropPendingSlot(i);
    }
  }
  std::function<void()> after_octree_update_;  // one-shot: called in SampleAndFilter right after the occupancy update
  // Speculative sampling of the NEXT batch (streaming single-GPU steps): intersection and march are issued on the side stream
  // as soon as THIS batch's samples are packed -- against the octree as it stands, underneath this step's pre-pass -- and
  // repaired behind this step's stat update (PersSampler::CompleteSpeculative).  The sampler's two latency chains (~0.6 ms on
  // a converged scene) then no longer sit between one step's stat update and the next step's pre-pass.  Not used in the
  // iterations that run ProcOctree (node indices change: the batch is sampled after the update, as before).
  // MEASURED (profiles/r03_speculation_experiments.txt): it pays while no leaf dies -- fresh scene 1.254 -> 1.171 ms per step --
  // and costs where leaves die in most steps -- converged scene 0.917 -> 0.959 ms, 20 000 iterations 17.9 -> 19.7 s: the
  // repair's duration is the re-walk and re-march of the LONGEST invalidated ray (~85 us), and it sits on the cycle the
  // sampler left.  Hence mode 2 (the default): speculate only when no leaf has died for kSpecQuietEpochs stat updates, as far
  // as the host can tell from a pinned word the update kernel writes (a timing decision only: samples are identical).
  int speculative_sampling_ = 2;  // 0 never, 1 always (outside ProcOctree iterations), 2 while the octree is quiet
  static constexpr int kSpecQuietEpochs = 8;
  struct NextBatch {
    Tensor rays_o, rays_d;
    float fineness = 1.f;
    int64_t seq = -1;
    bool valid = false;
  } next_batch_, next2_batch_;  // the batch of the next step, and (two-deep pipeline) of the step after it
  // Two-deep pipeline (round 4).  With ONE batch in flight the sampler chain of batch k+1 -- walk, march, repair, scan, pack:
  // 0.65-0.75 ms of latency on a converged scene -- has exactly step k to finish in, and a converged step is no longer than that:
  // the main queue waits for it.  With next2_batch_ handed over as well, batch k+2 is walked and marched during step k (on the
  // other side stream) and repaired + packed behind step k+1's stat update against every death since: its chain has two steps,
  // and the only sampler work between a stat update and the next step's pre-pass is the tail repair + pack of the batch in front.
  // 1: never; 2: once the octree has outgrown the LDS-resident walk (PersSampler::LdsWalkMaxInterior: the chain is then as long
  // as a step); 3: always.
  int spec_depth_ = 2;
  int64_t n_speculative_ = 0, n_spec_fallback_ = 0;  // batches sampled speculatively / sampled after the update instead
  void PreSampleSpecBegin(int slot, const Tensor& rays_o, const Tensor& rays_d, float fineness, int64_t seq);
  // Small trees (one-step-ahead regime): the batch after next is begun when THIS step's backward has been queued, not at the top
  // of the next step -- its noise draw, prologue and LDS-resident walk then run underneath the step's Adam / reduction tail (an
  // HBM stream: the vector units are idle) instead of colliding with the next step's gather, whose long-lived blocks keep a
  // newly dispatched small kernel waiting for a wave slot (measured: 0.29 ms for the 9 k-element noise draw;
  // profiles/r04_fresh_timeline.txt).  The step's own stat update is in the stream already, so the batch is repaired against the
  // next one only, exactly like a batch begun at the top of the next step.
  void SpecBeginAtStepEnd();
  bool PreSampleSpecComplete(int slot);  // false: could not be repaired (tree re-numbered): dropped
  at::cuda::CUDAEvent spec_start_ev_;
  bool spec_start_recorded_ = false;
  // ExpRunner::Train's batch draws OFF the main queue (round 6): Dataset::RandRaysData's one kernel runs on the device's tail stream
  // -- idle at the top of a step -- out of that stream's pool; a batch's rays are read first by its sampling on a side stream (which
  // waits for draw_ev_ at its begin) and two steps later by the main stream, which is ordered behind the draw through that batch's
  // presample_done_ev_ or, when it samples the batch itself, waits for draw_ev_.  The pool's memory is protected like the sampler's:
  // the tail stream waits for `consumed` in front of every draw, and a step of such a loop records `consumed` whatever its path.
  c10::hip::HIPStreamMasqueradingAsCUDA* BeginDraw();
  void EndDraw();
  void ConsumedBehindStep(uint64_t seq_before);  // records `consumed` if the step that has just been queued did not
  uint64_t ConsumedSeq() { return side_shared_ ? side_shared_->seq : 0; }
  at::cuda::CUDAEvent draw_ev_;
  bool draw_ev_recorded_ = false;
  bool rays_off_main_ = false;          // set by ExpRunner::Train around its loop: the main stream starts a step with nothing queued since `consumed`
  bool spec_start_is_consumed_ = false;  // this step's "start" point for speculative begins is the previous step's `consumed` (no event of its own)
  RenderFront SampleAndFilter(const Tensor& rays_o, const Tensor& rays_d, const Tensor& bounds, const Tensor& emb_idx,
                              bool async_count = false);
  // The survivor count of an async SampleAndFilter arrives in pinned memory; the host-side bookkeeping that depends on it
  // (meaningful-samples EMA, counters) is applied here: at the start of the next step, or by ExpRunner::FinishPending.
  void ResolvePendingCount();
  // data-parallel runs (DataParallel.cpp): the survivor count behind the meaningful-samples EMA is summed over the ranks in
  // the occupancy exchange, so that every replica sizes its next ray batch from the same number
  int dp_world_ = 1;
  Tensor dp_count_, dp_count_host_;
  int dp_count_rays_ = 0, dp_sum_rays_ = 0;  // rays behind dp_count_ / behind the sum a scan has mirrored to the host
  bool dp_sum_mirrored_ = false;
  at::cuda::CUDAEvent dp_count_ev_;
  float KeptPerRayForEma(int n_kept_local, int n_rays);
  // The meaningful-samples average AFTER the count of step `seq` went into it, for the last kEmaRing steps: ExpRunner::Train
  // sizes batch j from the average after step j - kBatchSizeLag in EVERY mode (synchronous steps know their count at once,
  // streaming steps one step late, data-parallel streaming steps two: a fixed lag takes the schedule out of the batch sizes).
  static constexpr int kEmaRing = 32;
  struct EmaMark {
    int64_t seq = -1;
    float value = 0.f;
  } ema_ring_[kEmaRing];
  void RecordEma(int64_t seq) {
    if (seq >= 0) ema_ring_[seq % kEmaRing] = {seq, global_data_pool_->meaningful_sampled_pts_per_ray_};
  }
  bool EmaAfter(int64_t seq, float* value) const {
    if (seq < 0 || ema_ring_[seq % kEmaRing].seq != seq) return false;
    *value = ema_ring_[seq % kEmaRing].value;
    return true;
  }
  int64_t pending_count_seq_ = -1;  // the step the pending survivor count belongs to
  // Per-step digest (diagnostics: WHERE do two trainings part?): rays, marched and surviving samples of the last kDigestRing
  // training steps (a whole 20 000-iteration run), by sequence number; table_sum (when ExpRunner::digest_table_ is on): an order-free integer checksum of the
  // f16 table after the step's Adam, on the device until read.
  static constexpr int kDigestRing = 32768;
  struct StepDigest {
    int64_t seq = -1;
    int iter = 0, n_rays = 0, n_marched = 0, n_kept = -1;
  };
  std::vector<StepDigest> digest_;
  void DigestBegin(int n_rays, int n_marched) {
    if (cur_seq_ < 0) return;
    if (digest_.empty()) digest_.resize(kDigestRing);
    digest_[cur_seq_ % kDigestRing] = {cur_seq_, global_data_pool_->iter_step_, n_rays, n_marched, -1};
  }
  void DigestKept(int64_t seq, int n_kept) {
    if (seq >= 0 && !digest_.empty() && digest_[seq % kDigestRing].seq == seq) digest_[seq % kDigestRing].n_kept = n_kept;
  }
  // Debugging taps (ExpRunner::digest_taps): order-free integer checksums of a step's intermediate arrays -- sampler outputs,
  // pre-pass densities, survivor bounds, background, edge samples, colours, gradient buffers, parameters after Adam -- one
  // int64 per (step, tap), on the device until read (ExpRunner.step_digest).  Two trainings that part are bisected to the
  // first array that differs.  One small reduction launch per tap and step: off unless asked for.
  enum { TAP_PTS, TAP_DT, TAP_ANCHORS, TAP_F0, TAP_SURVIVORS, TAP_BG, TAP_EDGE, TAP_COLORS, TAP_TABLE_GRAD, TAP_SMALL_GRADS, TAP_TABLE,
         TAP_FIELD_MLP, TAP_COLOR_MLP, TAP_APP_EMB, TAP_GRAD_BEFORE, TAP_PTS_ALL_AFTER, TAP_VOL_ALL_AFTER, TAP_FIELD_X, TAP_DFEAT,
         // the same arrays IN FRONT of the kernel that consumes them: a tap pair that differs inside one run is an array that changed while
         // (or after) it was read -- a late write from another stream -- and needs no second run to compare with
         TAP_PTS_PRE, TAP_DT_PRE, TAP_ANCHORS_PRE, TAP_PTS_ALL_PRE, TAP_VOL_ALL_PRE, N_TAPS };
  bool digest_taps_ = false;
  Tensor digest_tap_sums_;  // int64 [kDigestRing, N_TAPS]
  void DigestTap(int tap, const Tensor& t);
  bool async_count_ = false;        // set by ExpRunner::TrainStep for streaming steps
  // A streaming train step's grad pass starts from the field outputs its own density pre-pass computed (same table, same weights,
  // same h16 features: the same bits) instead of evaluating the field network a second time, and its field backward reads the
  // pre-pass feature cache through the survivors' row index instead of a copy (ExpRunner.prepass_feat_reuse; false = the
  // field_shade_fwd / compact field_x path, bit-identical results).  Host-side and data-independent.
  bool prepass_feat_reuse_ = true;
  // With reuse, a large-batch pre-pass keeps its hash features as the gather's own planes (Hash3DAnchored::prepass_planes_) and
  // writes no row-major copy; the field backward reads the planes (f2n_field_bwd_*_planes).  ExpRunner.prepass_planes_cache;
  // false = the row cache and the _rows calls, bit-identical results.
  bool prepass_planes_cache_ = true;
  // Occupancy votes and stat update OFF the main queue (ExpRunner.votes_off_main, profiles/votes_off_main.txt).  They feed only the
  // repair and pack of the NEXT batch, yet sat on the main queue in front of compaction (the fused f2n_early_stop_votes /
  // f2n_oct_update_stats_scan launches).  On an eligible step -- streaming, single GPU, no exchange hook, no octree maintenance due,
  // no digest taps -- the main stream runs f2n_early_stop and f2n_segment_scan_ex, records ONE event (early_stop_ev_: the tail stream and the host's
  // count read wait for it) and goes on with compaction; the device's tail stream casts the votes (f2n_oct_mark_visit), runs the stat
  // update and records octree_ready_ev_.  0 = never (the fused launches), 1 = every eligible step, 2 = eligible steps of the
  // one-batch-ahead regime only (not two_deep: there the cycle stat update -> next sampling bounds the step).  Same bytes either way.
  // Ordering: (a) the tail stream is in order, so the next step's votes follow this step's stat update, which re-arms the vote rows;
  // (b) the main stream waits for octree_ready_ev_ at the end of the step (TrainForwardBackward) -- before `consumed` is recorded and
  // before the tensors the votes read are released (RenderFront) -- and at the top of the next SampleAndFilter if that did not happen
  // (tail_votes_pending_), so whatever replaces the octree or the vote buffer on the main stream later (ProcOctree in a fused step,
  // LoadStates, InstallOctree, a VoteBuffer() rebuild) is ordered behind the tail stream's last update; (c) the batch draws on the
  // tail stream keep their `consumed` wait in front (BeginDraw) and queue behind the update.
  // Default 2: the fresh fox step gains 9 us (1.087 -> 1.078 ms); the two-deep regime keeps its program.
  int votes_off_main_ = 2;
  int64_t n_votes_off_main_steps_ = 0;  // steps that took that route
  at::cuda::CUDAEvent early_stop_ev_;
  bool tail_votes_pending_ = false;  // the tail stream holds an update the main stream has not been ordered behind yet
  void JoinTailVotes();              // ... orders it (one wait on octree_ready_ev_)
  bool keep_prepass_outputs_ = false;  // TrainForwardBackward -> SampleAndFilter: this pre-pass is a streaming train step's
  int64_t n_feat_reuse_steps_ = 0;     // steps that took the reuse path (tests: the knob is inert where it must be)
  bool count_pending_ = false;
  int pending_count_rays_ = 0;
  int64_t total_kept_pts_ = 0, total_all_pts_ = 0;  // running totals over training-mode calls (resolved counts only)
  // forward + ExpRunner::Train's loss + backward into the gradient buffers, without the autograd tape
  TrainOutputs TrainForwardBackward(const Tensor& rays_o, const Tensor& rays_d, const Tensor& bounds, const Tensor& gt_colors,
                                    const Tensor& emb_idx, float var_w, float disp_w, float tv_w, float dist_w = 0.f);

  // World-space density (RendererQuery.cpp): exp(f0 - 3) at world points [n,3], exactly 0 where no listed leaf holds the point;
  // on the grid of MakeGridSpec as [nz, ny, nx] (x fastest), in z-slabs of at most density_slab_points_ points; and the
  // iso-surface of that grid at `level`.  Free of side effects on training (no keyed draws, no occupancy votes, the pre-pass
  // feature cache kept); the caller flushes a streaming step first (ExpRunner::FinishPending).
  // Every point query below is the same four steps (helpers at the top of RendererQuery.cpp): locate; LocatedRows = the non-empty
  // points compacted into rows, whose count is the query's one read-back; the query's own field calls on the rows, under a
  // PrepassCacheGuard that puts Hash3DAnchored's three pre-pass caches back on every exit path, an exception included; its own scatter kernel.
  Tensor QueryDensity(const Tensor& world);
  Tensor DensityGrid(const std::vector<float>& lo, const std::vector<float>& hi, int res);
  std::tuple<Tensor, Tensor> ExtractMesh(const std::vector<float>& lo, const std::vector<float>& hi, int res, float level);
  static GridSpec MakeGridSpec(const std::vector<float>& lo, const std::vector<float>& hi, int res, int max_res = 1024);
  Tensor DensityOfLocated(const Tensor& warped, const Tensor& anchors);
  // ExtractMesh's mesh, bit for bit, without the dense grid (res up to 8192): BrickMark, then the flagged bricks in ascending order in
  // batches of max(1, density_slab_points_ / (brick + 1)^3) bricks through f2n_oct_locate_warp_bricks -> DensityOfLocated ->
  // BrickMeshBatch, then BrickMeshAssemble.  Exact for level >= 0 (a crossing edge then has a non-empty endpoint, and every
  // non-empty point lies in flagged bricks only); std::invalid_argument for level < 0.  The side-effect contract of QueryDensity.
  std::tuple<Tensor, Tensor> ExtractMeshSparse(const std::vector<float>& lo, const std::vector<float>& hi, int res, float level, int brick,
                                               SparseMeshStats* stats = nullptr);
  // (density [n], rgb [n,3]) at world points seen from the UNIT directions dirs [n,3] (not normalised here): the density of
  // QueryDensity, bit for bit, and the shader's colour for the point's field features without appearance embedding -- what
  // RenderForward computes per sample; zeros where no listed leaf holds the point.  The same side-effect contract as QueryDensity.
  std::tuple<Tensor, Tensor> QueryRadiance(const Tensor& world, const Tensor& dirs);
  // ExtractMesh, then: the components of fewer than min_component_faces faces removed, normals of the surviving vertices from
  // the same density grid, colours = the radiance at each vertex seen along its inward normal ((0, 0, -1) where the normal is 0)
  // normal_source "field": the normals are FieldNormals at the kept vertices (a vertex whose field normal is the zero vector takes
  // its grid normal) and the colours follow them; "grid" (the default): the density grid's normals
  // sparse in {4, 8, 16}: the mesh comes from ExtractMeshSparse with that brick size (the same bits) and no dense grid exists -- the
  // normals are FieldNormals alone ((0, 0, 0) where that vanishes); normal_source "grid" with normals or colours: std::invalid_argument
  MeshAttrs ExtractMeshAttrs(const std::vector<float>& lo, const std::vector<float>& hi, int res, float level, int min_component_faces,
                             bool normals, bool colors, const std::string& normal_source = "grid", int simplify = 0,
                             const MeshRefineOptions& refine = MeshRefineOptions(), int sparse = 0);
  // Points moved onto the level set sigma = level by a damped Newton iteration on h = ln(sigma) - ln(level) along grad sigma / sigma:
  // `iters` rounds of QueryDensityGrad at the candidates (DensityGradChunk, in slabs), a torch log, f2n_level_step.  A step is at most
  // max_step long and no candidate leaves the ball of radius max_move around its origin (origins undefined: the point's own start).
  // A point where the field cannot be evaluated (an empty leaf, sigma = 0) keeps its bits.  Inference only; the side-effect contract
  // of QueryDensity.  std::invalid_argument for level <= 0, iters < 1, max_step <= 0, max_move <= 0, tol < 0.
  LevelProjection ProjectToLevel(const Tensor& points, float level, int iters, float max_step, float max_move, float tol,
                                 const Tensor& origins = Tensor());
  // (density [n], grad [n,3]) at world points: the density of QueryDensity, bit for bit, and its analytic gradient with respect to the
  // world position, sigma J^T df0/dw (f2n_field_density_grad / f2n_density_grad_scatter: the hash table's trilinear blend, the
  // density MLP and the leaf's warp differentiated exactly, fp32); zeros where no listed leaf holds the point.  Field shapes
  // without the fused kernels take df0/dx from f2n_mlp_bwd (its h16 roundings) and f2n_hash_pos_grad: both routes are Df0Dw of
  // RendererQuery.cpp, which RenderGeometry shares.  The same side-effect contract as QueryDensity; reads back only the row count.
  std::tuple<Tensor, Tensor> QueryDensityGrad(const Tensor& world);
  // -grad / |grad| of QueryDensityGrad (the sign of GridNormals); 0 where |grad| is 0 or not finite, or the point is empty
  Tensor FieldNormals(const Tensor& world);
  // The slab loop both share: world [n,3] in chunks of at most density_slab_points_ points, each through DensityGradChunk; whichever
  // of density [n], grad [n,3], normals [n,3] is defined is filled (an undefined density / grad gets a scratch buffer per chunk).
  void DensityGradSlabs(const Tensor& world, const Tensor& density, const Tensor& grad, const Tensor& normals);
  // density, grad and (where defined) unit normals of one chunk, written in place
  void DensityGradChunk(const Tensor& world, const Tensor& density, const Tensor& grad, const Tensor& normals);
  // RenderForward plus geometry buffers (f2n_composite_geometry): per ray the opacity (sum of the weights), the weight-composited
  // unit normal, and the surface = the first sample at which the accumulated weight reaches tau (index, t, world point, normal; -1 and
  // zeros where none does).  The samples' normals are -J^T df0/dw / |.| at o + t d: f2n_field_density_grad on the survivors' rows of
  // the pre-pass cache (f2n_mlp_bwd + f2n_hash_pos_grad for field shapes without the fused kernels).  Colours, disparity, depth and
  // weights are RenderForward's bit for bit.  Inference mode only; the side-effect contract of RenderForward.  Unlike RenderForward
  // this path reads the survivor count back, once per call (the gradient kernels take their row count from the host).
  GeometryResult RenderGeometry(const Tensor& rays_o, const Tensor& rays_d, const Tensor& bounds, float tau, bool keep_samples);
  int64_t density_slab_points_ = int64_t(1) << 22;

  int LoadStates(const std::vector<Tensor>& states, int idx) override;
  std::vector<Tensor> States() override;
  std::vector<ParamGroup> OptimParamGroups() override;
  void ZeroGrad();
  // both networks have the shapes the fused (untaped, streaming) training step and the forward-only render are built for
  bool FusedPathOk() const;

  GlobalDataPool* global_data_pool_;
  std::unique_ptr<PtsSampler> pts_sampler_;
  std::unique_ptr<Field> scene_field_;
  std::unique_ptr<Shader> shader_;
  bool use_app_emb_;
  Tensor app_emb_;       // [n_images, 16]
  Tensor app_emb_grad_;  // fp32, unscaled
  Tensor small_grads_flat_;  // when defined: the flat home of the three small gradient buffers (ExpRunner::FlattenSmallGrads)
  BGColorType bg_color_type_ = BGColorType::rand_noise;
  SampleResultFlex sample_result_, presampled_;
  bool has_presample_ = false, presample_async_ = false;
  int presample_slot_ = 0;  // the side stream (pending slot) an asynchronous presample was produced on
  Tensor presample_rays_o_, presample_rays_d_;  // the rays the presample belongs to (held: see PresampleMatches)
  bool PresampleMatches(const Tensor& rays_o, const Tensor& rays_d) const;
  at::cuda::CUDAEvent octree_ready_ev_, presample_done_ev_[kPendingSlots], n_kept_ev_;
  // which event the pending survivor count hides behind: n_kept_ev_, or -- streaming steps, whose survivor scan rides in the stat
  // update's launch -- the octree event recorded behind that very launch (one packet instead of two)
  at::cuda::CUDAEvent* kept_wait_ev_ = &n_kept_ev_;
  // The two side streams -- and so their allocator pools -- are per DEVICE (EnsureSideStream), and so is the protocol that stands in
  // for record_stream on the sample buffers that cross from a side stream's pool to the main stream: `consumed` is recorded on the
  // main stream once the last reader of such buffers has been queued and awaited by a side stream before its next kernels, once
  // per recording (seq counts the recordings, waited[slot] what each stream has waited for).  One event per device, not per
  // Renderer: memory one Renderer returns to a shared pool may be handed to another Renderer's side-stream kernels (round-4 advisor).
  struct SideShared {
    std::shared_ptr<c10::hip::HIPStreamMasqueradingAsCUDA> stream[kPendingSlots];
    std::shared_ptr<c10::hip::HIPStreamMasqueradingAsCUDA> tail;  // (created with the first fused step tail)
    at::cuda::CUDAEvent consumed;
    uint64_t seq = 0, waited[kPendingSlots] = {0, 0};
  };
  std::shared_ptr<SideShared> side_shared_;
  bool consumed_side_samples_ = false;
  void SideWaitConsumed(int slot);
  bool small_grads_clean_ = false;  // set by ExpRunner::OptimStep (fused zero_grad), consumed by the next ZeroGrad()
  std::function<void()> after_count_readback_;  // ExpRunner: reads the previous step's finiteness flags here (no extra wait)
  // ExpRunner: the step's tail -- finiteness flags, Adam -- as arguments of the field backward's call (f2n_field_bwd_step_tail);
  // false: this step keeps the separate launches.  step_tail_done_: the call has queued them (ExpRunner::EnqueueApply's cue).
  std::function<bool(F2nStepTail*)> step_tail_builder_;
  // two batches in flight (the walk + march of the batch after next begin at the TOP of a step): see spec_depth_
  bool TwoDeepRegime();
  // ExpRunner: called once the step's forward has been queued and before anything of its backward is (loss scales, the step count
  // and the schedule the backward and the optimiser read are settled there: the previous step's finiteness flags)
  std::function<void()> before_backward_;
  bool step_tail_done_ = false;
  c10::hip::HIPStreamMasqueradingAsCUDA* TailStream();  // the device's third side stream (flags + small Adam beside the scatter)
  MappedWords n_kept_words_;  // [1]: the surviving-sample count, written by the survivor scan itself, read behind n_kept_ev_
  std::shared_ptr<c10::hip::HIPStreamMasqueradingAsCUDA> side_[kPendingSlots];  // (shared by every Renderer of the device)
  void EnsureSideStream(int slot);
  Tensor forced_bg_;  // explicit background colours for parity tests (undefined = as the reference)
  int n_edge_pts_ = 8192;
  int last_n_all_pts_ = 0, last_n_kept_pts_ = 0;
};

namespace CustomOps {
Tensor WeightVar(Tensor weights, Tensor idx_start_end);  // CustomOps.cu:12-66 via f2n_weight_var_*
// [R]: the distortion loss of every ray on its warped intervals via f2n_distortion_* (no reference counterpart); differentiable in weights
Tensor Distortion(Tensor weights, Tensor dt, Tensor idx_start_end);
}

}  // namespace f2n
