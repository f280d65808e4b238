// World-space density and radiance queries, iso-surface extraction and mesh attributes (csrc/octree.hip; include/f2n_abi.h, "World-space queries and meshes").
// None of this is on the training path: the queries draw nothing from the keyed streams, touch no occupancy statistics and leave
// the pre-pass feature cache of Hash3DAnchored (prepass_x_) as they found it.  Callers flush a streaming step first
// (ExpRunner::FinishPending, as SaveCheckpoint does).
// Shared by the drivers, defined first: Points3, LocatedRows (locate -> compact: the non-empty points as rows, the one read-back),
// PrepassCacheGuard (the cache contract on every exit path), Df0Dw (df0/dw of rows, fused or op by op), TwoTotals.  A point query
// is: locate, rows, its own field calls under the guard, its own scatter kernel.
#include <cmath>
#include <limits>

#include "Renderer.h"

namespace f2n {

namespace {

// [n,3] float32 on the device, of at most INT32_MAX rows (the kernels count in int)
Tensor Points3(const Tensor& t) {
  Tensor p = t.to(torch::kCUDA, torch::kFloat32).contiguous().view({-1, 3});
  TORCH_CHECK(p.size(0) <= INT32_MAX, "too many points");
  return p;
}

// The non-empty points of a located set as rows of their own (f2n_located_compact): se [n,2] = every point's row range (what the
// scatter kernels read), total = the row count on the device, pts / vol (/ src: the point each row came from, on request) = the m rows.
// The field kernels take their row count from the host: m is the one read-back of a query.
struct LocatedRows {
  Tensor se, total, pts, vol, src;
  int m = 0;
  LocatedRows(const Tensor& warped, const Tensor& anchors, bool want_src) {
    const int64_t n = anchors.size(0);
    Tensor counts = torch::empty({n}, DevI32());
    se = torch::empty({n, 2}, DevI32());
    total = torch::empty({1}, DevI32());
    Tensor cpts = torch::empty({n, 3}, DevF32()), cvol = torch::empty({n}, DevI32()), csrc;
    if (want_src) csrc = torch::empty({n}, DevI32());
    F2N_CALL(f2n_located_compact(CurStream(), (int) n, I32P(anchors), F32P(warped), I32P(counts), I32P(se), I32P(total), F32P(cpts),
                                 I32P(cvol), want_src ? I32P(csrc) : nullptr));
    m = total.item<int>();
    pts = cpts.narrow(0, 0, m);
    vol = cvol.narrow(0, 0, m);
    if (want_src) src = csrc.narrow(0, 0, m);
  }
};

// The side-effect contract of every query: a batch sampled ahead may still be served from the pre-pass feature cache, so whatever a
// query's field calls make of Hash3DAnchored::prepass_x_ -- and of prepass_feat_h_, the field outputs of the same rows that a
// streaming train step keeps beside it, and of prepass_planes_, the form that step keeps the features in -- is undone when the guard goes out of scope -- by return or by exception.
struct PrepassCacheGuard {
  Hash3DAnchored* field;
  Tensor kept, kept_feat_h, kept_planes;
  explicit PrepassCacheGuard(Hash3DAnchored* f) : field(f), kept(f->prepass_x_), kept_feat_h(f->prepass_feat_h_), kept_planes(f->prepass_planes_) {}
  ~PrepassCacheGuard() {
    field->prepass_x_ = kept;
    field->prepass_feat_h_ = kept_feat_h;
    field->prepass_planes_ = kept_planes;
  }
};

// df0/dw [m,3] of the rows (p [m,3] warped, v [m]) into g.  x_h defined: their h16 hash features, the fused route
// (f2n_field_density_grad).  Undefined -- field shapes without the fused kernels --: df0/dx from the general MLP backward (its h16
// roundings) with dy = e_0 and no loss scale, then f2n_hash_pos_grad.
void Df0Dw(Hash3DAnchored* field, const Tensor& p, const Tensor& v, const Tensor& x_h, Tensor& g) {
  if (x_h.defined()) return field->DensityGrad(p, v, x_h, g);
  auto& mlp = *field->mlp_;
  const int m = (int) p.size(0);
  Tensor x = field->HashEncode(p, v).to(torch::kFloat32).contiguous();
  Tensor dy = torch::zeros({m, F2N_MLP_OUT_PAD}, DevF32());
  dy.select(1, 0).fill_(1.f);
  Tensor dparams = torch::zeros({mlp.n_params_}, DevF32()), dx = torch::empty({m, mlp.d_in_}, DevF32());
  F2N_CALL(f2n_mlp_bwd(CurStream(), m, mlp.d_in_, mlp.d_hidden_, mlp.n_hidden_layers_, 1.f, VoidP(mlp.params_h_), F32P(x), F32P(dy),
                       F32P(dparams), F32P(dx)));
  field->PosGrad(p, v, dx, g);
}

// the two totals a count kernel left on the device: the one read-back of a mesher (they size its outputs)
std::pair<int64_t, int64_t> TwoTotals(const Tensor& totals) {
  Tensor t = totals.cpu();
  return {t.data_ptr<int32_t>()[0], t.data_ptr<int32_t>()[1]};
}

}  // namespace

std::tuple<Tensor, Tensor> PersSampler::LocatePoints(const Tensor& world) {
  torch::NoGradGuard g;
  Tensor w = Points3(world);
  const int64_t n = w.size(0);
  Tensor warped = torch::empty({n, 3}, DevF32()), anchors = torch::empty({n, 3}, DevI32());
  auto& o = *pers_octree_;
  F2N_CALL(f2n_oct_locate_warp(CurStream(), (int) n, F32P(w), VoidP(o.tree_nodes_gpu_), VoidP(o.pers_trans_gpu_), F32P(warped),
                               I32P(anchors)));
  return {warped, anchors};
}

Tensor Renderer::DensityOfLocated(const Tensor& warped, const Tensor& anchors) {
  torch::NoGradGuard g;
  auto* field = static_cast<Hash3DAnchored*>(scene_field_.get());
  const int64_t n = anchors.size(0);
  Tensor density = torch::empty({n}, DevF32());
  if (n == 0) return density;
  LocatedRows rows(warped, anchors, /*want_src=*/false);
  Tensor f0 = torch::zeros({1}, DevF32());
  if (rows.m > 0) {
    PrepassCacheGuard cache(field);
    f0 = field->QueryDensityPreAct(rows.pts, rows.vol, /*keep_features=*/false);
  }
  F2N_CALL(f2n_density_scatter(CurStream(), (int) n, I32P(anchors), I32P(rows.se), F32P(f0), F32P(density)));
  return density;
}

Tensor Renderer::QueryDensity(const Tensor& world) {
  auto* sampler = static_cast<PersSampler*>(pts_sampler_.get());
  auto located = sampler->LocatePoints(world);
  return DensityOfLocated(std::get<0>(located), std::get<1>(located));
}

std::tuple<Tensor, Tensor> Renderer::QueryRadiance(const Tensor& world, const Tensor& dirs) {
  torch::NoGradGuard g;
  auto* sampler = static_cast<PersSampler*>(pts_sampler_.get());
  auto* field = static_cast<Hash3DAnchored*>(scene_field_.get());
  auto* shader = static_cast<SHShader*>(shader_.get());
  auto located = sampler->LocatePoints(world);
  const Tensor& warped = std::get<0>(located);
  const Tensor& anchors = std::get<1>(located);
  const int64_t n = anchors.size(0);
  Tensor d = Points3(dirs);
  TORCH_CHECK(d.size(0) == n, "one view direction per point");
  Tensor density = torch::empty({n}, DevF32()), rgb = torch::empty({n, 3}, DevF32());
  if (n == 0) return {density, rgb};
  LocatedRows rows(warped, anchors, /*want_src=*/true);
  const int m = rows.m;
  Tensor f0 = torch::zeros({1}, DevF32()), crgb = torch::zeros({1, 3}, DevF32());
  if (m > 0) {
    PrepassCacheGuard cache(field);
    Tensor cdirs = d.index_select(0, rows.src).contiguous();  // the directions travel with their points
    if (FusedPathOk()) {
      f0 = field->QueryDensityPreAct(rows.pts, rows.vol, /*keep_features=*/true);
      TORCH_CHECK(field->prepass_x_.defined(), "no pre-pass feature cache for this query");
      crgb = torch::empty({m, 3}, DevF32());
      Tensor f0_again = torch::empty({m}, DevF32());  // (the fused launch writes its own copy; the density comes from the pre-pass)
      F2N_CALL(f2n_field_shade_fwd_dyn(CurStream(), m, I32P(rows.total), nullptr, VoidP(field->prepass_x_), VoidP(field->mlp_->params_h_),
                                       F32P(cdirs), nullptr, nullptr, VoidP(shader->mlp_->params_h_), F32P(f0_again), nullptr, nullptr,
                                       F32P(crgb)));
    } else {  // network shapes without fused kernels: op by op, as Render()
      f0 = field->QueryDensityPreAct(rows.pts, rows.vol, /*keep_features=*/false);
      Tensor feat = field->AnchoredQuery(rows.pts, rows.vol);
      Tensor none = torch::empty({0}, DevF32());
      crgb = shader->QueryFromField(feat, cdirs, none, torch::empty({0}, DevI32()), nullptr).to(torch::kFloat32).contiguous();
    }
  }
  F2N_CALL(f2n_radiance_scatter(CurStream(), (int) n, I32P(anchors), I32P(rows.se), F32P(f0), F32P(crgb), F32P(density), F32P(rgb)));
  return {density, rgb};
}

void Renderer::DensityGradChunk(const Tensor& w, const Tensor& density, const Tensor& grad, const Tensor& normals) {
  auto* sampler = static_cast<PersSampler*>(pts_sampler_.get());
  auto* field = static_cast<Hash3DAnchored*>(scene_field_.get());
  auto located = sampler->LocatePoints(w);
  const Tensor& warped = std::get<0>(located);
  const Tensor& anchors = std::get<1>(located);
  const int64_t n = anchors.size(0);
  if (n == 0) return;
  LocatedRows rows(warped, anchors, /*want_src=*/false);
  Tensor f0 = torch::zeros({1}, DevF32()), g = torch::zeros({1, 3}, DevF32());
  if (rows.m > 0) {
    PrepassCacheGuard cache(field);
    g = torch::empty({rows.m, 3}, DevF32());
    f0 = field->QueryDensityPreAct(rows.pts, rows.vol, /*keep_features=*/field->fused_ok_);
    TORCH_CHECK(!field->fused_ok_ || field->prepass_x_.defined(), "no pre-pass feature cache for this query");
    Df0Dw(field, rows.pts, rows.vol, field->prepass_x_, g);  // (field shapes without the fused kernels keep no features)
  }
  auto& o = *sampler->pers_octree_;
  F2N_CALL(f2n_density_grad_scatter(CurStream(), (int) n, F32P(w), I32P(anchors), I32P(rows.se), VoidP(o.pers_trans_gpu_), F32P(f0), F32P(g),
                                    F32P(density), F32P(grad), normals.defined() ? F32P(normals) : nullptr));
}

void Renderer::DensityGradSlabs(const Tensor& w, const Tensor& density, const Tensor& grad, const Tensor& normals) {
  const int64_t n = w.size(0);
  for (int64_t i0 = 0; i0 < n; i0 += density_slab_points_) {  // (bounded workspaces, as DensityGrid's slabs)
    const int64_t c = std::min(density_slab_points_, n - i0);
    DensityGradChunk(w.narrow(0, i0, c), density.defined() ? density.narrow(0, i0, c) : torch::empty({c}, DevF32()),
                     grad.defined() ? grad.narrow(0, i0, c) : torch::empty({c, 3}, DevF32()),
                     normals.defined() ? normals.narrow(0, i0, c) : Tensor());
  }
}

std::tuple<Tensor, Tensor> Renderer::QueryDensityGrad(const Tensor& world) {
  torch::NoGradGuard g;
  Tensor w = Points3(world);
  Tensor density = torch::empty({w.size(0)}, DevF32()), grad = torch::empty({w.size(0), 3}, DevF32());
  DensityGradSlabs(w, density, grad, Tensor());
  return {density, grad};
}

Tensor Renderer::FieldNormals(const Tensor& world) {
  torch::NoGradGuard g;
  Tensor w = Points3(world);
  Tensor normals = torch::empty({w.size(0), 3}, DevF32());
  DensityGradSlabs(w, Tensor(), Tensor(), normals);
  return normals;
}

// RenderForward step by step (SampleAndFilter -> f2n_field_shade_fwd_dyn -> f2n_composite_fwd: the same launches on the same inputs,
// so colours, disparity, depth and weights are its bits), then the survivors' df0/dw (Df0Dw) and f2n_composite_geometry.  The gradient
// kernels take their row count from the host and want the survivors' h16 features as rows of their own, so this path -- unlike
// RenderForward, which leaves the count on the device -- reads the survivor count back, once per call (= per chunk of
// ExpRunner::RenderGeometry), and takes the rows out of the pre-pass cache through src_rows before the cache is dropped.
GeometryResult Renderer::RenderGeometry(const Tensor& rays_o_in, const Tensor& rays_d_in, const Tensor& bounds, float tau, bool keep_samples) {
  auto* gdp = global_data_pool_;
  auto* sampler = static_cast<PersSampler*>(pts_sampler_.get());
  auto* field = static_cast<Hash3DAnchored*>(scene_field_.get());
  auto* shader = static_cast<SHShader*>(shader_.get());
  TORCH_CHECK(gdp->mode_ != RunningMode::TRAIN, "RenderGeometry is an inference path");
  TORCH_CHECK(tau > 0.f && tau <= 1.f, "tau must lie in (0, 1], got ", tau);
  torch::NoGradGuard no_grad;
  Tensor rays_o = rays_o_in.contiguous(), rays_d = rays_d_in.contiguous();
  CheckDev(rays_o, torch::kFloat32, "rays_o");
  CheckDev(rays_d, torch::kFloat32, "rays_d");
  const int n_rays = rays_o.size(0);
  const bool fused = FusedPathOk();
  void* st = CurStream();
  GeometryResult out;
  out.opacity = torch::zeros({n_rays}, DevF32());
  out.normals = torch::zeros({n_rays, 3}, DevF32());
  out.surf_idx = torch::full({n_rays}, -1, DevI32());
  out.surf_t = torch::zeros({n_rays}, DevF32());
  out.surf_points = torch::zeros({n_rays, 3}, DevF32());
  out.surf_normals = torch::zeros({n_rays, 3}, DevF32());
  // keep_samples: the per-sample outputs are the first m rows of the samples' arrays and of the gradient / normal buffers
  auto kept_samples = [&](const Tensor& pts, const Tensor& anchors, const Tensor& t, const Tensor& dt, int64_t m) {
    if (!keep_samples) return;
    out.pts = pts.narrow(0, 0, m);
    out.anchors = anchors.narrow(0, 0, m);
    out.t = t.narrow(0, 0, m);
    out.dt = dt.narrow(0, 0, m);
    out.sample_grad = out.sample_grad.narrow(0, 0, m);
    out.sample_normals = out.sample_normals.narrow(0, 0, m);
  };
  // (field shapes without the fused kernels render op by op, as RenderForward does through Render(): the synchronous count)
  RenderFront fr = SampleAndFilter(rays_o, rays_d, bounds, Tensor(), /*async_count=*/fused);
  if (fr.empty) {  // RenderForward's empty result
    out.render = {fr.bg_color, torch::zeros({n_rays, 1}, DevF32()), torch::zeros({n_rays}, DevF32()), Tensor(),
                  torch::full({n_rays}, 512.f, DevF32()), Tensor(), Tensor()};
    if (keep_samples) {  // (no rows of anything)
      out.sample_grad = torch::empty({0, 3}, DevF32());
      out.sample_normals = torch::empty({0, 3}, DevF32());
    }
    kept_samples(torch::empty({0, 3}, DevF32()), torch::empty({0, 3}, DevI32()), torch::empty({0}, DevF32()), torch::empty({0}, DevF32()), 0);
    return out;
  }
  SampleResultFlex& es = fr.es;
  const int n_cap = std::max(fr.n_kept, 1);
  int m = fr.n_kept;
  // the two routes differ in where the density pre-activations lie (sigma, its row stride) and in how rgb was made
  Tensor sigma, rgb;
  int sigma_stride = 1;
  if (fused) {
    TORCH_CHECK(field->prepass_x_.defined(), "no pre-pass feature cache for this query");
    sigma = torch::empty({n_cap}, DevF32());
    rgb = torch::empty({n_cap, 3}, DevF32());
    const at::Half* cache = field->prepass_x_.data_ptr<at::Half>() + (int64_t) N_LEVELS * N_CHANNELS * fr.sample_cache_row;
    F2N_TIMED_CALL("field_shade_fwd", f2n_field_shade_fwd_dyn(st, fr.n_kept, I32P(fr.n_kept_dev), I32P(fr.src_rows),
                           static_cast<const void*>(cache), VoidP(field->mlp_->params_h_), F32P(es.dirs), nullptr, nullptr,
                           VoidP(shader->mlp_->params_h_), F32P(sigma), nullptr, nullptr, F32P(rgb)));
  } else {  // op by op, the launches of Render() in VALIDATE mode
    Tensor feat = field->AnchoredQueryReuse(fr.pts_all, fr.vol_all, fr.src_rows, m).slice(0, 0, m);
    rgb = shader->QueryFromField(feat, es.dirs, torch::empty({0}, DevF32()), fr.sample_emb_idx, nullptr).contiguous();
    sigma = feat.contiguous();
    sigma_stride = F2N_MLP_OUT_PAD;
  }
  Tensor colors = torch::empty({n_rays, 3}, DevF32()), disparity = torch::empty({n_rays}, DevF32()), depth = torch::empty({n_rays}, DevF32());
  Tensor weights = torch::empty({n_cap}, DevF32());
  Tensor bg = fr.bg_color.contiguous();
  F2N_TIMED_CALL("composite_fwd", f2n_composite_fwd(st, n_rays, I32P(es.pts_idx_bounds), F32P(sigma), sigma_stride, F32P(es.dt), F32P(es.t),
                             F32P(rgb), F32P(bg), F32P(colors), F32P(disparity), F32P(depth), F32P(weights), nullptr));
  if (fused) {
    m = fr.n_kept_dev.item<int>();  // the read-back RenderForward avoids: everything above has been queued by now
    TORCH_CHECK(m >= 0 && m <= fr.n_kept, "survivor count out of range");
  }
  Tensor g = torch::zeros({std::max(m, 1), 3}, DevF32());  // df0/dw of the survivors [m,3]
  if (m > 0) {
    Tensor x_h;  // fused: the survivors' rows of the pre-pass cache
    if (fused) {
      const int64_t row = (int64_t) N_LEVELS * N_CHANNELS;
      Tensor cache_rows = field->prepass_x_.view({-1, row}).narrow(0, fr.sample_cache_row, field->prepass_x_.numel() / row - fr.sample_cache_row);
      x_h = cache_rows.index_select(0, fr.src_rows.narrow(0, 0, m).to(torch::kInt64)).contiguous();
    }
    Tensor p = es.pts.narrow(0, 0, m).contiguous(), v = es.anchors.narrow(0, 0, m).select(1, 0).contiguous();
    Df0Dw(field, p, v, x_h, g);
  }
  if (fused) field->DropPrepassCache();  // (as RenderForward: the cache served its render)
  out.render = {colors, es.first_oct_dis, disparity, Tensor(), depth, weights, es.pts_idx_bounds};
  Tensor dirs = torch::empty_like(rays_d);  // the unit directions the march walked along (the sampler's own normalisation)
  F2N_CALL(f2n_normalize_dirs(st, n_rays, F32P(rays_d), F32P(dirs)));
  if (keep_samples) {
    out.sample_grad = torch::empty({std::max(m, 1), 3}, DevF32());
    out.sample_normals = torch::empty({std::max(m, 1), 3}, DevF32());
  }
  Tensor anchors = es.anchors.contiguous(), tt = es.t.contiguous();
  F2N_TIMED_CALL("composite_geometry", f2n_composite_geometry(st, n_rays, I32P(es.pts_idx_bounds), F32P(weights), F32P(tt), F32P(rays_o), F32P(dirs),
                                  I32P(anchors), VoidP(sampler->pers_octree_->pers_trans_gpu_), F32P(g), tau, F32P(out.opacity),
                                  F32P(out.normals), I32P(out.surf_idx), F32P(out.surf_t), F32P(out.surf_points), F32P(out.surf_normals),
                                  keep_samples ? F32P(out.sample_grad) : nullptr, keep_samples ? F32P(out.sample_normals) : nullptr));
  if (keep_samples) out.render.weights = weights.narrow(0, 0, m);
  kept_samples(es.pts, es.anchors, es.t, es.dt, m);
  return out;
}

GridSpec Renderer::MakeGridSpec(const std::vector<float>& lo, const std::vector<float>& hi, int res, int max_res) {
  TORCH_CHECK(lo.size() == 3 && hi.size() == 3, "lo / hi must have three coordinates");
  TORCH_CHECK(res >= 1 && res <= max_res, "resolution must be in [1, ", max_res, "]");
  GridSpec s;
  float ext[3], longest = 0.f;
  for (int k = 0; k < 3; k++) {
    ext[k] = hi[k] - lo[k];
    TORCH_CHECK(ext[k] > 0.f && std::isfinite(ext[k]), "empty or invalid box");
    longest = std::max(longest, ext[k]);
    s.lo[k] = lo[k];
  }
  s.step = longest / (float) res;
  for (int k = 0; k < 3; k++) s.n[k] = std::max(2, (int) std::lround(ext[k] / s.step) + 1);
  return s;
}

Tensor Renderer::DensityGrid(const std::vector<float>& lo, const std::vector<float>& hi, int res) {
  torch::NoGradGuard g;
  const GridSpec s = MakeGridSpec(lo, hi, res);
  const int nx = s.n[0], ny = s.n[1], nz = s.n[2];
  const int64_t plane = (int64_t) nx * ny;
  // z-slabs of at most density_slab_points_ points: the gather's plane workspace ([8][n][4] h16, 64 B per point) and the
  // compaction buffers stay bounded at any resolution
  const int slab_z = (int) std::max<int64_t>(1, std::min<int64_t>(nz, density_slab_points_ / plane));
  Tensor out = torch::empty({nz, ny, nx}, DevF32());
  auto& o = *static_cast<PersSampler*>(pts_sampler_.get())->pers_octree_;
  const int64_t cap = plane * slab_z;
  Tensor warped = torch::empty({cap, 3}, DevF32()), anchors = torch::empty({cap, 3}, DevI32());
  for (int z0 = 0; z0 < nz; z0 += slab_z) {
    const int n_z = std::min(slab_z, nz - z0);
    const int64_t n = plane * n_z;
    Tensor w = warped.narrow(0, 0, n), a = anchors.narrow(0, 0, n);
    F2N_CALL(f2n_oct_locate_warp_grid(CurStream(), s.lo, s.step, nx, ny, nz, z0, n_z, VoidP(o.tree_nodes_gpu_), VoidP(o.pers_trans_gpu_),
                                      F32P(w), I32P(a)));
    out.narrow(0, z0, n_z).view({-1}).copy_(DensityOfLocated(w, a));
  }
  return out;
}

namespace {
// valid: undefined = every corner carries a value (f2n_mesh_count), else the uint8 mask of f2n_mesh_count_masked
std::tuple<Tensor, Tensor> MeshFromGridImpl(const Tensor& grid, const Tensor& valid, float level, const float lo[3], float step) {
  torch::NoGradGuard g;
  Tensor gr = grid.to(torch::kCUDA, torch::kFloat32).contiguous();
  TORCH_CHECK(gr.dim() == 3, "grid must be [nz, ny, nx]");
  const int nz = (int) gr.size(0), ny = (int) gr.size(1), nx = (int) gr.size(2);
  Tensor va;
  if (valid.defined()) {
    va = valid.to(torch::kCUDA, torch::kUInt8).contiguous();
    TORCH_CHECK(va.numel() == gr.numel(), "valid must have one entry per grid point");
  }
  if (nx < 2 || ny < 2 || nz < 2) return {torch::empty({0, 3}, DevF32()), torch::empty({0, 3}, DevI32())};
  const int64_t n_corners = (int64_t) nx * ny * nz, n_cells = (int64_t) (nx - 1) * (ny - 1) * (nz - 1);
  Tensor mask = torch::empty({n_corners}, torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA));
  Tensor vc = torch::empty({n_corners}, DevI32()), vse = torch::empty({n_corners, 2}, DevI32());
  Tensor fc = torch::empty({n_cells}, DevI32()), fse = torch::empty({n_cells, 2}, DevI32()), totals = torch::empty({2}, DevI32());
  if (va.defined())
    F2N_CALL(f2n_mesh_count_masked(CurStream(), nx, ny, nz, F32P(gr), level, va.data_ptr<uint8_t>(), mask.data_ptr<uint8_t>(), I32P(vc),
                                   I32P(vse), I32P(fc), I32P(fse), I32P(totals)));
  else
    F2N_CALL(f2n_mesh_count(CurStream(), nx, ny, nz, F32P(gr), level, mask.data_ptr<uint8_t>(), I32P(vc), I32P(vse), I32P(fc), I32P(fse),
                            I32P(totals)));
  const auto [nv, nf] = TwoTotals(totals);
  Tensor verts = torch::empty({nv, 3}, DevF32()), faces = torch::empty({nf, 3}, DevI32());
  if (nv > 0 || nf > 0)
    F2N_CALL(f2n_mesh_emit(CurStream(), nx, ny, nz, F32P(gr), level, lo, step, mask.data_ptr<uint8_t>(), I32P(vse), I32P(fse),
                           F32P(verts), I32P(faces)));
  return {verts, faces};
}
}  // namespace

std::tuple<Tensor, Tensor> MeshFromGrid(const Tensor& grid, float level, const float lo[3], float step) {
  return MeshFromGridImpl(grid, Tensor(), level, lo, step);
}

std::tuple<Tensor, Tensor> MeshFromGridMasked(const Tensor& grid, const Tensor& valid, float level, const float lo[3], float step) {
  TORCH_CHECK(valid.defined(), "valid is required");
  return MeshFromGridImpl(grid, valid, level, lo, step);
}

// ---- sparse meshing on bricks (include/f2n_abi.h, "Sparse mesh extraction on bricks") ----------------------------------------
namespace {
constexpr int kSparseMaxRes = 8192;

torch::TensorOptions DevI64() { return DevI32().dtype(torch::kInt64); }

// bricks per axis and their number; std::invalid_argument for what f2n_brick_mark refuses
int64_t BrickCounts(const int n[3], int B, int nb[3]) {
  if (B != 4 && B != 8 && B != 16) throw std::invalid_argument("brick size must be 4, 8 or 16, got " + std::to_string(B));
  int64_t total = 1;
  for (int k = 0; k < 3; k++) {
    if (n[k] < 2 || n[k] > F2N_BRICK_MAX_POINTS) throw std::invalid_argument("the grid must have 2 .. 2^19 points per axis");
    nb[k] = (n[k] - 1 + B - 1) / B;
    total *= nb[k];
  }
  if (total > INT32_MAX) throw std::invalid_argument("the grid has " + std::to_string(total) + " bricks; at most 2^31 - 1 are supported");
  return total;
}

// brick_ids as a device int32 list, every id inside the grid and listed once
Tensor CheckedBrickIds(const Tensor& brick_ids, int64_t total) {
  Tensor ids = brick_ids.to(torch::kCUDA, torch::kInt64).contiguous().view({-1});
  if (ids.numel() > 0) {
    Tensor sorted = std::get<0>(torch::sort(ids));
    Tensor ends = torch::stack({sorted[0], sorted[-1]}).cpu();
    if (ends.data_ptr<int64_t>()[0] < 0 || ends.data_ptr<int64_t>()[1] >= total)
      throw std::invalid_argument("a brick id lies outside the grid's " + std::to_string(total) + " bricks");
    if (ids.numel() > 1 && (sorted.narrow(0, 1, ids.numel() - 1) == sorted.narrow(0, 0, ids.numel() - 1)).any().item<bool>())
      throw std::invalid_argument("a brick id is listed twice");
  }
  return ids.to(torch::kInt32).contiguous();
}
}  // namespace

Tensor BrickMark(const Tensor& tree_nodes, const float lo[3], float step, const int n[3], int B) {
  torch::NoGradGuard g;
  int nb[3];
  BrickCounts(n, B, nb);
  Tensor nodes = tree_nodes.to(torch::kCUDA).contiguous();
  TORCH_CHECK(nodes.scalar_type() == torch::kUInt8 && nodes.numel() >= 64 && nodes.numel() % 64 == 0, "tree_nodes must be uint8, 64 B per node");
  Tensor flags = torch::empty({nb[2], nb[1], nb[0]}, torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA));
  F2N_CALL(f2n_brick_mark(CurStream(), VoidP(nodes), lo, step, n[0], n[1], n[2], B, flags.data_ptr<uint8_t>()));
  return flags;
}

BrickMeshPart BrickMeshBatch(const Tensor& values, const Tensor& brick_ids, const int n[3], const float lo[3], float step, float level, int B,
                             const Tensor& valid) {
  torch::NoGradGuard g;
  const int64_t nbr = brick_ids.numel(), P = (int64_t) (B + 1) * (B + 1) * (B + 1);
  TORCH_CHECK(brick_ids.is_cuda() && brick_ids.scalar_type() == torch::kInt32 && brick_ids.is_contiguous(), "brick_ids must be device int32");
  TORCH_CHECK(values.is_cuda() && values.scalar_type() == torch::kFloat32 && values.is_contiguous() && values.numel() == nbr * P,
              "values must be device float32 [n_bricks, (B+1)^3]");
  TORCH_CHECK(!valid.defined() || (valid.is_cuda() && valid.scalar_type() == torch::kUInt8 && valid.is_contiguous() && valid.numel() == nbr * P),
              "valid must be device uint8 [n_bricks, (B+1)^3]");
  TORCH_CHECK(nbr <= INT32_MAX, "too many bricks in one batch");
  BrickMeshPart part;
  part.vert_keys = torch::empty({0}, DevI64());
  part.verts = torch::empty({0, 3}, DevF32());
  part.face_keys = torch::empty({0}, DevI64());
  part.face_vert_keys = torch::empty({0, 3}, DevI64());
  if (nbr == 0) return part;
  Tensor vc = torch::empty({nbr}, DevI32()), fc = torch::empty({nbr}, DevI32());
  if (valid.defined())
    F2N_CALL(f2n_brick_mesh_count_masked(CurStream(), n[0], n[1], n[2], B, (int) nbr, I32P(brick_ids), F32P(values), valid.data_ptr<uint8_t>(),
                                         level, I32P(vc), I32P(fc)));
  else
    F2N_CALL(f2n_brick_mesh_count(CurStream(), n[0], n[1], n[2], B, (int) nbr, I32P(brick_ids), F32P(values), level, I32P(vc), I32P(fc)));
  Tensor vend = torch::cumsum(vc, 0, torch::kInt64), fend = torch::cumsum(fc, 0, torch::kInt64);
  Tensor tot = torch::stack({vend[-1], fend[-1], ((vc > 0) | (fc > 0)).sum()}).cpu();  // the one read-back: the totals size the outputs
  const int64_t nv = tot.data_ptr<int64_t>()[0], nf = tot.data_ptr<int64_t>()[1];
  part.meshed_bricks = tot.data_ptr<int64_t>()[2];
  if (nv == 0 && nf == 0) return part;
  Tensor vstart = (vend - vc).contiguous(), fstart = (fend - fc).contiguous();
  // (at least one row each: the emit wants its four outputs, and a batch may own vertices but no face or the other way round)
  Tensor vk = torch::empty({std::max<int64_t>(nv, 1)}, DevI64()), v = torch::empty({std::max<int64_t>(nv, 1), 3}, DevF32());
  Tensor fk = torch::empty({std::max<int64_t>(nf, 1)}, DevI64()), fvk = torch::empty({std::max<int64_t>(nf, 1), 3}, DevI64());
  if (valid.defined())
    F2N_CALL(f2n_brick_mesh_emit_masked(CurStream(), n[0], n[1], n[2], B, (int) nbr, I32P(brick_ids), F32P(values), valid.data_ptr<uint8_t>(),
                                        level, lo, step, vstart.data_ptr<int64_t>(), fstart.data_ptr<int64_t>(), vk.data_ptr<int64_t>(), F32P(v),
                                        fk.data_ptr<int64_t>(), fvk.data_ptr<int64_t>()));
  else
    F2N_CALL(f2n_brick_mesh_emit(CurStream(), n[0], n[1], n[2], B, (int) nbr, I32P(brick_ids), F32P(values), level, lo, step,
                                 vstart.data_ptr<int64_t>(), fstart.data_ptr<int64_t>(), vk.data_ptr<int64_t>(), F32P(v), fk.data_ptr<int64_t>(),
                                 fvk.data_ptr<int64_t>()));
  part.vert_keys = vk.narrow(0, 0, nv);
  part.verts = v.narrow(0, 0, nv);
  part.face_keys = fk.narrow(0, 0, nf);
  part.face_vert_keys = fvk.narrow(0, 0, nf);
  return part;
}

std::tuple<Tensor, Tensor> BrickMeshAssemble(const std::vector<BrickMeshPart>& parts, bool drop_unreferenced) {
  torch::NoGradGuard g;
  std::vector<Tensor> vk, v, fk, fvk;
  for (const auto& p : parts) {
    vk.push_back(p.vert_keys);
    v.push_back(p.verts);
    fk.push_back(p.face_keys);
    fvk.push_back(p.face_vert_keys);
  }
  if (parts.empty()) return {torch::empty({0, 3}, DevF32()), torch::empty({0, 3}, DevI32())};
  Tensor keys = torch::cat(vk), verts = torch::cat(v), fkeys = torch::cat(fk), fverts = torch::cat(fvk);
  const int64_t nv = keys.size(0), nf = fkeys.size(0);
  if (nv > INT32_MAX || nf > INT32_MAX)
    throw std::invalid_argument("the mesh has " + std::to_string(nv) + " vertices and " + std::to_string(nf) + " faces; at most 2^31 - 1 of each are supported");
  auto sorted = torch::sort(keys);
  const Tensor& skeys = std::get<0>(sorted);
  verts = verts.index_select(0, std::get<1>(sorted)).contiguous();
  if (nf == 0) return {drop_unreferenced ? torch::empty({0, 3}, DevF32()) : verts, torch::empty({0, 3}, DevI32())};
  if (nv == 0) throw std::invalid_argument("the brick list lacks the owner of a face's vertex");
  Tensor want = fverts.view({-1});
  Tensor at = torch::searchsorted(skeys, want).clamp_max(nv - 1);
  if (!(skeys.index_select(0, at) == want).all().item<bool>()) throw std::invalid_argument("the brick list lacks the owner of a face's vertex");
  if (drop_unreferenced) {  // the vertices some face names, in key order; a face's index = the number of kept vertices in front of it
    Tensor used = torch::zeros({nv}, DevI64());
    used.index_fill_(0, at, 1);
    Tensor rank = torch::cumsum(used, 0) - used;
    verts = verts.index_select(0, torch::nonzero(used).view({-1})).contiguous();
    at = rank.index_select(0, at);
  }
  Tensor faces = at.to(torch::kInt32).view({-1, 3}).index_select(0, torch::argsort(fkeys)).contiguous();
  return {verts, faces};
}

namespace {
// valid: undefined = MeshFromBricks, else MeshFromBricksMasked
std::tuple<Tensor, Tensor> MeshFromBricksImpl(const Tensor& values, const Tensor& valid, const Tensor& brick_ids, const int n[3],
                                              const float lo[3], float step, float level, int B, int64_t batch_bricks) {
  torch::NoGradGuard g;
  int nb[3];
  const int64_t total = BrickCounts(n, B, nb);
  Tensor ids = CheckedBrickIds(brick_ids, total);
  const int64_t nbr = ids.numel(), P = (int64_t) (B + 1) * (B + 1) * (B + 1);
  Tensor vals = values.to(torch::kCUDA, torch::kFloat32).contiguous();
  TORCH_CHECK(vals.numel() == nbr * P, "values must be [n_bricks, (B+1)^3]");
  vals = vals.view({nbr, P});
  Tensor ok;
  if (valid.defined()) {
    ok = valid.to(torch::kCUDA, torch::kUInt8).contiguous();
    TORCH_CHECK(ok.numel() == nbr * P, "valid must be [n_bricks, (B+1)^3]");
    ok = ok.view({nbr, P});
  }
  const int64_t per = batch_bricks > 0 ? batch_bricks : std::max<int64_t>(nbr, 1);
  std::vector<BrickMeshPart> parts;
  for (int64_t j0 = 0; j0 < nbr; j0 += per) {
    const int64_t c = std::min(per, nbr - j0);
    parts.push_back(BrickMeshBatch(vals.narrow(0, j0, c), ids.narrow(0, j0, c), n, lo, step, level, B,
                                   ok.defined() ? ok.narrow(0, j0, c) : Tensor()));
  }
  return BrickMeshAssemble(parts, ok.defined());
}
}  // namespace

std::tuple<Tensor, Tensor> MeshFromBricks(const Tensor& values, const Tensor& brick_ids, const int n[3], const float lo[3], float step,
                                          float level, int B, int64_t batch_bricks) {
  return MeshFromBricksImpl(values, Tensor(), brick_ids, n, lo, step, level, B, batch_bricks);
}

std::tuple<Tensor, Tensor> MeshFromBricksMasked(const Tensor& values, const Tensor& valid, const Tensor& brick_ids, const int n[3],
                                                const float lo[3], float step, float level, int B, int64_t batch_bricks) {
  TORCH_CHECK(valid.defined(), "valid is required");
  return MeshFromBricksImpl(values, valid, brick_ids, n, lo, step, level, B, batch_bricks);
}

std::tuple<Tensor, Tensor> Renderer::ExtractMeshSparse(const std::vector<float>& lo, const std::vector<float>& hi, int res, float level,
                                                       int brick, SparseMeshStats* stats) {
  torch::NoGradGuard g;
  if (!(level >= 0.f)) throw std::invalid_argument("extract_mesh_sparse: level must be >= 0 (the cull of empty bricks is exact only then)");
  const GridSpec s = MakeGridSpec(lo, hi, res, kSparseMaxRes);
  int nb[3];
  const int64_t total = BrickCounts(s.n, brick, nb);
  auto& o = *static_cast<PersSampler*>(pts_sampler_.get())->pers_octree_;
  Tensor flags = BrickMark(o.tree_nodes_gpu_, s.lo, s.step, s.n, brick);
  Tensor ids = torch::nonzero(flags.view({-1})).view({-1}).to(torch::kInt32).contiguous();  // ascending
  const int64_t n_active = ids.numel(), S = brick + 1, P = S * S * S;
  const int64_t per = std::max<int64_t>(1, density_slab_points_ / P);
  SparseMeshStats st;
  st.bricks = total;
  st.active_bricks = n_active;
  for (int k = 0; k < 3; k++) st.grid[k] = s.n[k];
  if (n_active > 0) {  // the corners of the listed bricks that exist: per axis min(B + 1, n - b B)
    Tensor b = ids.to(torch::kInt64), cnt = torch::ones_like(b);
    Tensor bc[3] = {b % nb[0], torch::floor_divide(b, nb[0]) % nb[1], torch::floor_divide(b, (int64_t) nb[0] * nb[1])};
    for (int k = 0; k < 3; k++) cnt = cnt * torch::clamp_max(s.n[k] - bc[k] * brick, S);
    st.points_evaluated = cnt.sum().item<int64_t>();
  }
  std::vector<BrickMeshPart> parts;
  Tensor nonempty = torch::zeros({1}, DevI64());
  const int64_t cap = std::min(per, std::max<int64_t>(n_active, 1)) * P;
  Tensor warped = torch::empty({cap, 3}, DevF32()), anchors = torch::empty({cap, 3}, DevI32());
  for (int64_t j0 = 0; j0 < n_active; j0 += per) {
    const int64_t c = std::min(per, n_active - j0);
    Tensor batch = ids.narrow(0, j0, c);
    Tensor w = warped.narrow(0, 0, c * P), a = anchors.narrow(0, 0, c * P);
    F2N_CALL(f2n_oct_locate_warp_bricks(CurStream(), s.lo, s.step, s.n[0], s.n[1], s.n[2], brick, (int) c, I32P(batch), VoidP(o.tree_nodes_gpu_),
                                        VoidP(o.pers_trans_gpu_), F32P(w), I32P(a)));
    nonempty += (a.select(1, 0) >= 0).sum();
    Tensor values = DensityOfLocated(w, a);
    parts.push_back(BrickMeshBatch(values, batch, s.n, s.lo, s.step, level, brick));
    st.meshed_bricks += parts.back().meshed_bricks;
    st.batches++;
  }
  st.points_nonempty = nonempty.item<int64_t>();
  if (stats != nullptr) *stats = st;
  return BrickMeshAssemble(parts);
}

namespace {
const Tensor& DevArg(const Tensor& t, torch::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous(), name, " must be a contiguous device tensor of its type");
  return t;
}
}  // namespace

void TsdfIntegrate(const Tensor& S, const Tensor& W, const float lo[3], float step, const Tensor& poses, const Tensor& intri,
                   const Tensor& dist, const Tensor& depth, const Tensor& conf, float trunc) {
  torch::NoGradGuard g;
  // (S and W are updated in place: no copy may stand in for them)
  DevArg(S, torch::kFloat32, "S");
  DevArg(W, torch::kFloat32, "W");
  TORCH_CHECK(S.dim() == 3 && W.sizes() == S.sizes(), "S and W must be [nz, ny, nx]");
  Tensor po = poses.to(torch::kCUDA, torch::kFloat32).contiguous(), in = intri.to(torch::kCUDA, torch::kFloat32).contiguous();
  Tensor di = dist.to(torch::kCUDA, torch::kFloat32).contiguous(), de = depth.to(torch::kCUDA, torch::kFloat32).contiguous();
  TORCH_CHECK(de.dim() == 3, "depth must be [V, h, w]");
  const int64_t V = de.size(0);
  TORCH_CHECK(V <= INT32_MAX && po.numel() == V * 12 && in.numel() == V * 9 && di.numel() == V * 4,
              "poses [V,3,4], intri [V,3,3] and dist_params [V,4] must match depth [V,h,w]");
  Tensor co;
  if (conf.defined()) {
    co = conf.to(torch::kCUDA, torch::kFloat32).contiguous();
    TORCH_CHECK(co.sizes() == de.sizes(), "conf must have the shape of depth");
  }
  F2N_CALL(f2n_tsdf_integrate(CurStream(), lo, step, (int) S.size(2), (int) S.size(1), (int) S.size(0), (int) V, F32P(po), F32P(in), F32P(di),
                              F32P(de), co.defined() ? F32P(co) : nullptr, (int) de.size(1), (int) de.size(2), trunc, F32P(S), F32P(W)));
}

std::tuple<Tensor, Tensor> TsdfFinalize(const Tensor& S, const Tensor& W, float min_weight) {
  torch::NoGradGuard g;
  DevArg(S, torch::kFloat32, "S");
  DevArg(W, torch::kFloat32, "W");
  TORCH_CHECK(W.sizes() == S.sizes(), "S and W must have the same shape");
  Tensor out = torch::empty_like(S), valid = torch::empty(S.sizes(), torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA));
  F2N_CALL(f2n_tsdf_finalize(CurStream(), S.numel(), F32P(S), F32P(W), min_weight, F32P(out), valid.data_ptr<uint8_t>()));
  return {out, valid};
}

// ---- sparse TSDF fusion on bricks (include/f2n_abi.h, "Sparse TSDF fusion on bricks") -----------------------------------------
namespace {
// the views of TsdfIntegrate as contiguous device float32 tensors: {poses, intri, dist, depth, conf or undefined}
struct TsdfViews {
  Tensor po, in, di, de, co;
  int V = 0, h = 0, w = 0;
};
TsdfViews CheckedViews(const Tensor& poses, const Tensor& intri, const Tensor& dist, const Tensor& depth, const Tensor& conf) {
  TsdfViews v;
  v.po = poses.to(torch::kCUDA, torch::kFloat32).contiguous(), v.in = intri.to(torch::kCUDA, torch::kFloat32).contiguous();
  v.di = dist.to(torch::kCUDA, torch::kFloat32).contiguous(), v.de = depth.to(torch::kCUDA, torch::kFloat32).contiguous();
  TORCH_CHECK(v.de.dim() == 3, "depth must be [V, h, w]");
  const int64_t V = v.de.size(0);
  TORCH_CHECK(V <= INT32_MAX && v.po.numel() == V * 12 && v.in.numel() == V * 9 && v.di.numel() == V * 4,
              "poses [V,3,4], intri [V,3,3] and dist_params [V,4] must match depth [V,h,w]");
  if (conf.defined()) {
    v.co = conf.to(torch::kCUDA, torch::kFloat32).contiguous();
    TORCH_CHECK(v.co.sizes() == v.de.sizes(), "conf must have the shape of depth");
  }
  v.V = (int) V, v.h = (int) v.de.size(1), v.w = (int) v.de.size(2);
  return v;
}
void CheckTrunc(float trunc) {
  if (!(trunc > 0.f) || !std::isfinite(trunc)) throw std::invalid_argument("trunc must be positive and finite");
}

Tensor TsdfBrickMarkViews(const float lo[3], float step, const int n[3], int B, const TsdfViews& v, float trunc) {
  int nb[3];
  BrickCounts(n, B, nb);
  CheckTrunc(trunc);
  Tensor flags = torch::zeros({nb[2], nb[1], nb[0]}, torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA));
  F2N_CALL(f2n_tsdf_brick_mark(CurStream(), lo, step, n[0], n[1], n[2], B, v.V, F32P(v.po), F32P(v.in), F32P(v.di), F32P(v.de),
                               v.co.defined() ? F32P(v.co) : nullptr, v.h, v.w, trunc, flags.data_ptr<uint8_t>()));
  return flags;
}

// ids: device int32, checked
void TsdfIntegrateBrickRows(const Tensor& S, const Tensor& W, const Tensor& ids, const float lo[3], float step, const int n[3], int B,
                            const TsdfViews& v, float trunc) {
  const int64_t P = (int64_t) (B + 1) * (B + 1) * (B + 1);
  DevArg(S, torch::kFloat32, "S");
  DevArg(W, torch::kFloat32, "W");
  TORCH_CHECK(S.numel() == ids.numel() * P && W.numel() == S.numel(), "S and W must be [n_bricks, (B+1)^3]");
  TORCH_CHECK(S.numel() <= INT32_MAX, "too many bricks in one batch");
  F2N_CALL(f2n_tsdf_integrate_bricks(CurStream(), lo, step, n[0], n[1], n[2], B, (int) ids.numel(), I32P(ids), v.V, F32P(v.po), F32P(v.in),
                                     F32P(v.di), F32P(v.de), v.co.defined() ? F32P(v.co) : nullptr, v.h, v.w, trunc, F32P(S), F32P(W)));
}
}  // namespace

Tensor TsdfBrickMark(const float lo[3], float step, const int n[3], int B, const Tensor& poses, const Tensor& intri, const Tensor& dist,
                     const Tensor& depth, const Tensor& conf, float trunc) {
  torch::NoGradGuard g;
  return TsdfBrickMarkViews(lo, step, n, B, CheckedViews(poses, intri, dist, depth, conf), trunc);
}

void TsdfIntegrateBricks(const Tensor& S, const Tensor& W, const Tensor& brick_ids, const float lo[3], float step, const int n[3], int B,
                         const Tensor& poses, const Tensor& intri, const Tensor& dist, const Tensor& depth, const Tensor& conf, float trunc) {
  torch::NoGradGuard g;
  int nb[3];
  const int64_t total = BrickCounts(n, B, nb);
  CheckTrunc(trunc);
  TsdfIntegrateBrickRows(S, W, CheckedBrickIds(brick_ids, total), lo, step, n, B, CheckedViews(poses, intri, dist, depth, conf), trunc);
}

std::tuple<Tensor, Tensor> TsdfMeshSparse(const float lo[3], float step, const int n[3], int B, const Tensor& poses, const Tensor& intri,
                                          const Tensor& dist, const Tensor& depth, const Tensor& conf, float trunc, float min_weight,
                                          int64_t batch_bricks, SparseTsdfStats* stats) {
  torch::NoGradGuard g;
  int nb[3];
  const int64_t total = BrickCounts(n, B, nb);
  const TsdfViews v = CheckedViews(poses, intri, dist, depth, conf);
  Tensor flags = TsdfBrickMarkViews(lo, step, n, B, v, trunc);
  Tensor ids = torch::nonzero(flags.view({-1})).view({-1}).to(torch::kInt32).contiguous();  // ascending
  const int64_t n_active = ids.numel(), S1 = B + 1, P = S1 * S1 * S1;
  const int64_t per = std::max<int64_t>(1, batch_bricks);
  SparseTsdfStats st;
  st.bricks = total;
  st.active_bricks = n_active;
  for (int k = 0; k < 3; k++) st.grid[k] = n[k];
  if (n_active > 0) {  // the corners of the listed bricks that exist: per axis min(B + 1, n - b B)
    Tensor b = ids.to(torch::kInt64), cnt = torch::ones_like(b);
    Tensor bc[3] = {b % nb[0], torch::floor_divide(b, nb[0]) % nb[1], torch::floor_divide(b, (int64_t) nb[0] * nb[1])};
    for (int k = 0; k < 3; k++) cnt = cnt * torch::clamp_max(n[k] - bc[k] * B, S1);
    st.points_evaluated = cnt.sum().item<int64_t>();
  }
  std::vector<BrickMeshPart> parts;
  Tensor known = torch::zeros({1}, DevI64());
  for (int64_t j0 = 0; j0 < n_active; j0 += per) {  // one batch of rows alive at a time
    const int64_t c = std::min(per, n_active - j0);
    Tensor batch = ids.narrow(0, j0, c);
    Tensor S = torch::zeros({c, P}, DevF32()), W = torch::zeros({c, P}, DevF32());
    TsdfIntegrateBrickRows(S, W, batch, lo, step, n, B, v, trunc);
    auto [gv, valid] = TsdfFinalize(S, W, min_weight);
    known += (valid != 0).sum();  // (a corner that does not exist keeps W = 0: never valid)
    parts.push_back(BrickMeshBatch(gv, batch, n, lo, step, 0.f, B, valid));
    st.meshed_bricks += parts.back().meshed_bricks;
    st.batches++;
  }
  st.points_known = known.item<int64_t>();
  if (stats != nullptr) *stats = st;
  return BrickMeshAssemble(parts, true);
}

// ---- view-colour fusion (include/f2n_abi.h, "View-colour fusion") -------------------------------------------------------------
void ViewColorsAccumulate(const Tensor& acc, const Tensor& wsum, const Tensor& count, const Tensor& points, const Tensor& normals,
                          const Tensor& poses, const Tensor& intri, const Tensor& dist, const Tensor& depth, const Tensor& conf,
                          const Tensor& image, float tol, float cos_min) {
  torch::NoGradGuard g;
  // (the sums are updated in place: no copy may stand in for them)
  DevArg(acc, torch::kFloat32, "acc");
  DevArg(wsum, torch::kFloat32, "wsum");
  DevArg(count, torch::kInt32, "count");
  Tensor p = Points3(points);
  const int64_t n = p.size(0);
  TORCH_CHECK(acc.dim() == 2 && acc.size(0) == n && acc.size(1) >= 1 && acc.size(1) <= 4 && wsum.numel() == n && count.numel() == n,
              "acc must be [n, C] with C in [1, 4], wsum and count [n] for points [n, 3]");
  const int C = (int) acc.size(1);
  Tensor nr;
  if (normals.defined()) {
    nr = Points3(normals);
    TORCH_CHECK(nr.size(0) == n, "normals must have the shape of points");
  }
  const TsdfViews v = CheckedViews(poses, intri, dist, depth, conf);
  Tensor im = image.to(torch::kCUDA, torch::kFloat32).contiguous();
  TORCH_CHECK(im.dim() == 4 && im.size(0) == v.V && im.size(1) == v.h && im.size(2) == v.w && im.size(3) == C,
              "image must be [V, h, w, C] on the pixel grid of depth");
  F2N_CALL(f2n_view_colors_accumulate(CurStream(), n, F32P(p), nr.defined() ? F32P(nr) : nullptr, v.V, F32P(v.po), F32P(v.in), F32P(v.di),
                                      F32P(v.de), v.co.defined() ? F32P(v.co) : nullptr, F32P(im), C, v.h, v.w, tol, cos_min, F32P(acc),
                                      F32P(wsum), I32P(count)));
}

std::tuple<Tensor, Tensor> ViewColorsFinalize(const Tensor& acc, const Tensor& wsum, const Tensor& count, int min_views) {
  torch::NoGradGuard g;
  DevArg(acc, torch::kFloat32, "acc");
  DevArg(wsum, torch::kFloat32, "wsum");
  DevArg(count, torch::kInt32, "count");
  TORCH_CHECK(acc.dim() == 2 && acc.size(1) >= 1 && acc.size(1) <= 4 && wsum.numel() == acc.size(0) && count.numel() == acc.size(0),
              "acc must be [n, C] with C in [1, 4], wsum and count [n]");
  const int64_t n = acc.size(0);
  Tensor rgb = torch::empty_like(acc), known = torch::empty({n}, torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA));
  F2N_CALL(f2n_view_colors_finalize(CurStream(), n, (int) acc.size(1), F32P(acc), F32P(wsum), I32P(count), min_views, F32P(rgb),
                                    known.data_ptr<uint8_t>()));
  return {rgb, known};
}

std::tuple<Tensor, Tensor> Renderer::ExtractMesh(const std::vector<float>& lo, const std::vector<float>& hi, int res, float level) {
  const GridSpec s = MakeGridSpec(lo, hi, res);
  Tensor grid = DensityGrid(lo, hi, res);
  return MeshFromGrid(grid, level, s.lo, s.step);
}

Tensor GridNormals(const Tensor& grid, const Tensor& pts, const float lo[3], float step) {
  torch::NoGradGuard g;
  Tensor gr = grid.to(torch::kCUDA, torch::kFloat32).contiguous();
  TORCH_CHECK(gr.dim() == 3 && gr.size(0) >= 2 && gr.size(1) >= 2 && gr.size(2) >= 2, "grid must be [nz, ny, nx] with at least 2 points per axis");
  TORCH_CHECK(gr.numel() <= INT32_MAX && step > 0.f, "grid too large or step not positive");
  Tensor p = Points3(pts);
  const int64_t n = p.size(0);
  Tensor out = torch::empty({n, 3}, DevF32());
  F2N_CALL(f2n_grid_normals(CurStream(), (int) n, F32P(p), F32P(gr), (int) gr.size(2), (int) gr.size(1), (int) gr.size(0), lo, step,
                            F32P(out)));
  return out;
}

Tensor MeshComponents(const Tensor& faces, int64_t n_verts, int* rounds) {
  torch::NoGradGuard g;
  Tensor f = faces.to(torch::kCUDA, torch::kInt32).contiguous().view({-1, 3});
  TORCH_CHECK(n_verts >= 0 && n_verts <= INT32_MAX && f.size(0) <= INT32_MAX, "mesh too large");
  Tensor labels = torch::empty({n_verts}, DevI32()), changed = torch::zeros({1}, DevI32());
  F2N_CALL(f2n_mesh_components(CurStream(), (int) n_verts, (int) f.size(0), I32P(f), I32P(labels), I32P(changed), rounds));
  return labels;
}

std::tuple<Tensor, Tensor, Tensor> MeshFilterComponents(const Tensor& verts, const Tensor& faces, int min_faces) {
  torch::NoGradGuard g;
  Tensor v = Points3(verts);
  Tensor f = faces.to(torch::kCUDA, torch::kInt32).contiguous().view({-1, 3});
  const int64_t nv = v.size(0), nf = f.size(0);
  TORCH_CHECK(nf <= INT32_MAX, "mesh too large");
  if (min_faces <= 1) return {v, f, torch::arange(nv, DevI32())};
  Tensor labels = MeshComponents(f, nv);
  Tensor comp = torch::empty({nv}, DevI32()), vkeep = torch::empty({nv}, DevI32()), vse = torch::empty({nv, 2}, DevI32());
  Tensor fkeep = torch::empty({nf}, DevI32()), fse = torch::empty({nf, 2}, DevI32()), totals = torch::empty({2}, DevI32());
  F2N_CALL(f2n_mesh_filter_count(CurStream(), (int) nv, (int) nf, I32P(f), I32P(labels), min_faces, I32P(comp), I32P(vkeep), I32P(vse),
                                 I32P(fkeep), I32P(fse), I32P(totals)));
  const auto [kv, kf] = TwoTotals(totals);
  Tensor ov = torch::empty({kv, 3}, DevF32()), src = torch::empty({kv}, DevI32()), of = torch::empty({kf, 3}, DevI32());
  if (kv > 0 || kf > 0)
    F2N_CALL(f2n_mesh_filter_emit(CurStream(), (int) nv, (int) nf, F32P(v), I32P(f), I32P(vkeep), I32P(vse), I32P(fkeep), I32P(fse),
                                  F32P(ov), I32P(src), I32P(of)));
  return {ov, of, src};
}

namespace {
// a stretch of MeshSimplify between two kernels (sorted uniques, selections: torch ops) under a name of its own in the kernel timers
struct TimedSpan {
  const char* name;
  explicit TimedSpan(const char* n) : name(n) { KernelTimers::Get().Begin(name); }
  ~TimedSpan() { KernelTimers::Get().End(name); }
};
}  // namespace

std::tuple<Tensor, Tensor, Tensor> MeshSimplify(const Tensor& verts, const Tensor& faces, float cell, const float* lo_in, double lambda) {
  torch::NoGradGuard g;
  Tensor v = Points3(verts);
  Tensor f = faces.to(torch::kCUDA, torch::kInt32).contiguous().view({-1, 3});
  const int64_t nv = v.size(0), nf = f.size(0);
  TORCH_CHECK(nf <= INT32_MAX, "mesh too large");
  float lo[3] = {0.f, 0.f, 0.f};
  int32_t dims[3] = {1, 1, 1};
  if (lo_in != nullptr)
    for (int k = 0; k < 3; k++) lo[k] = lo_in[k];
  Tensor keys = torch::empty({nv}, DevI32().dtype(torch::kInt64));
  Tensor none_v = torch::empty({0, 3}, DevF32()), none_f = torch::empty({0, 3}, DevI32());
  if (nv > 0 && cell > 0.f && std::isfinite(cell)) {  // (any other cell: the kernels' own F2N_ERR_INVALID_ARG below)
    // the bounding box of the vertices' finite coordinates gives lo (unless given) and dims; the keys' clamp then only guards the upper border
    TimedSpan span("mesh_simplify_bounds");
    // (per coordinate, over its finite values; three full reductions over a column each -- a reduction of [V,3] over V is slow)
    Tensor fin = torch::isfinite(v);
    const float inf = std::numeric_limits<float>::infinity();
    Tensor lows = torch::where(fin, v, torch::full({1}, inf, DevF32())), highs = torch::where(fin, v, torch::full({1}, -inf, DevF32()));
    std::vector<Tensor> ends;
    for (int k = 0; k < 3; k++) ends.push_back(lows.select(1, k).min());
    for (int k = 0; k < 3; k++) ends.push_back(highs.select(1, k).max());
    Tensor box = torch::stack(ends).cpu();
    const float *mn = box.data_ptr<float>(), *mx = mn + 3;
    for (int k = 0; k < 3; k++) {
      if (mn[k] <= mx[k]) {  // (the coordinate has a finite value)
        if (lo_in == nullptr) lo[k] = mn[k];
        const float u = (mx[k] - lo[k]) / cell;  // (two fp32 roundings, as the keys' u)
        TORCH_CHECK(!(u >= 1048575.f), "cell ", cell, " is too small for the extent of the mesh (at most 2^20 cells per axis)");
        dims[k] = u >= 0.f ? (int) std::floor(u) + 1 : 1;
      }
    }
  }
  F2N_TIMED_CALL("mesh_cluster_keys", f2n_mesh_cluster_keys(CurStream(), (int) nv, F32P(v), lo, cell, dims, keys.data_ptr<int64_t>()));
  Tensor cluster_of, ckeys;
  int64_t nc = 0;
  {
    TimedSpan span("mesh_simplify_unique_keys");
    auto uq = at::_unique2(keys, /*sorted=*/true, /*return_inverse=*/true);
    const Tensor& uk = std::get<0>(uq);
    const int64_t bad = uk.size(0) > 0 && uk[0].item<int64_t>() < 0 ? 1 : 0;  // key -1 sorts first
    ckeys = uk.narrow(0, bad, uk.size(0) - bad).contiguous();
    cluster_of = (std::get<1>(uq) - bad).to(torch::kInt32).contiguous();
    nc = ckeys.size(0);
  }
  TORCH_CHECK(nc <= INT32_MAX, "mesh too large");
  Tensor vert_map = torch::full({nv}, -1, DevI32());
  if (nc == 0) return {none_v, none_f, vert_map};
  Tensor acc = torch::zeros({nc, 16}, DevI32().dtype(torch::kInt64)), flag = torch::empty({1}, DevI32());
  F2N_TIMED_CALL("mesh_cluster_accumulate",
                 f2n_mesh_cluster_accumulate(CurStream(), (int) nv, (int) nf, F32P(v), I32P(f), I32P(cluster_of), (int) nc, lo, cell, dims,
                                             acc.data_ptr<int64_t>(), I32P(flag)));
  Tensor cverts = torch::empty({nc, 3}, DevF32());
  F2N_TIMED_CALL("mesh_cluster_place", f2n_mesh_cluster_place(CurStream(), (int) nc, acc.data_ptr<int64_t>(), ckeys.data_ptr<int64_t>(), lo,
                                                              cell, dims, lambda, F32P(cverts)));
  if (nf == 0) return {none_v, none_f, vert_map};
  Tensor rows = torch::empty({nf, 3}, DevI32());
  F2N_TIMED_CALL("mesh_cluster_faces", f2n_mesh_cluster_faces(CurStream(), (int) nv, (int) nf, I32P(f), I32P(cluster_of), I32P(rows)));
  Tensor uf;
  {
    TimedSpan span("mesh_simplify_unique_faces");
    uf = std::get<0>(at::unique_dim(rows, 0, /*sorted=*/true));
    if (uf.size(0) > 0 && uf[0][0].item<int>() < 0) uf = uf.narrow(0, 1, uf.size(0) - 1);  // the dropped faces' row sorts first
    uf = uf.contiguous();
  }
  const int64_t kf0 = uf.size(0);
  if (kf0 == 0) return {none_v, none_f, vert_map};
  // the clusters no face uses leave, order kept: the component filter with one label and a threshold every face passes
  Tensor labels = torch::zeros({nc}, DevI32());
  Tensor comp = torch::empty({nc}, DevI32()), vkeep = torch::empty({nc}, DevI32()), vse = torch::empty({nc, 2}, DevI32());
  Tensor fkeep = torch::empty({kf0}, DevI32()), fse = torch::empty({kf0, 2}, DevI32()), totals = torch::empty({2}, DevI32());
  F2N_TIMED_CALL("mesh_simplify_compact", f2n_mesh_filter_count(CurStream(), (int) nc, (int) kf0, I32P(uf), I32P(labels), 1, I32P(comp),
                                                                I32P(vkeep), I32P(vse), I32P(fkeep), I32P(fse), I32P(totals)));
  const auto [kv, kf] = TwoTotals(totals);
  Tensor ov = torch::empty({kv, 3}, DevF32()), src = torch::empty({kv}, DevI32()), of = torch::empty({kf, 3}, DevI32());
  F2N_TIMED_CALL("mesh_simplify_compact", f2n_mesh_filter_emit(CurStream(), (int) nc, (int) kf0, F32P(cverts), I32P(uf), I32P(vkeep), I32P(vse),
                                                               I32P(fkeep), I32P(fse), F32P(ov), I32P(src), I32P(of)));
  Tensor new_of_cluster = torch::where(vkeep != 0, vse.select(1, 0), torch::full({1}, -1, DevI32()));
  vert_map = torch::where(cluster_of >= 0, new_of_cluster.index_select(0, cluster_of.clamp_min(0).to(torch::kInt64)), vert_map).contiguous();
  return {ov, of, vert_map};
}

MeshRingResult MeshRing(const Tensor& faces, int64_t n_verts) {
  torch::NoGradGuard g;
  Tensor f = faces.to(torch::kCUDA, torch::kInt32).contiguous().view({-1, 3});
  const int64_t nf = f.size(0);
  TORCH_CHECK(n_verts >= 0 && n_verts <= INT32_MAX && nf <= INT32_MAX / 6, "mesh too large");
  const auto i64 = DevI32().dtype(torch::kInt64);
  Tensor ek = torch::empty({0}, i64), uses = torch::empty({0}, i64);
  if (nf > 0) {
    Tensor keys = torch::empty({nf, 6}, i64);
    F2N_TIMED_CALL("mesh_ring_keys", f2n_mesh_ring_keys(CurStream(), (int) n_verts, (int) nf, I32P(f), keys.data_ptr<int64_t>()));
    TimedSpan span("mesh_ring_sort");
    Tensor sorted = std::get<0>(torch::sort(keys.view({-1})));
    const int64_t first = torch::searchsorted(sorted, torch::zeros({1}, i64)).item<int64_t>();  // the invalid faces' -1 sort first
    auto u = at::unique_consecutive(sorted.narrow(0, first, sorted.size(0) - first), /*return_inverse=*/false, /*return_counts=*/true);
    ek = std::get<0>(u).contiguous();
    uses = std::get<2>(u).to(torch::kInt64).contiguous();
  }
  const int64_t ne = ek.size(0);
  MeshRingResult r;
  r.start_end = torch::empty({n_verts, 2}, DevI32());
  r.ring = torch::empty({ne}, DevI32());
  r.pinned = torch::empty({n_verts}, DevI32().dtype(torch::kUInt8));
  r.edge_counts = torch::zeros({2}, DevI32());
  F2N_TIMED_CALL("mesh_ring_fill", f2n_mesh_ring_fill(CurStream(), (int) n_verts, (int) ne, ne > 0 ? ek.data_ptr<int64_t>() : nullptr,
                                                      ne > 0 ? uses.data_ptr<int64_t>() : nullptr, n_verts > 0 ? I32P(r.start_end) : nullptr,
                                                      ne > 0 ? I32P(r.ring) : nullptr, n_verts > 0 ? r.pinned.data_ptr<uint8_t>() : nullptr,
                                                      I32P(r.edge_counts)));
  return r;
}

Tensor MeshSmoothOnRing(const Tensor& verts, const MeshRingResult& ring, int passes, double lam, double mu, float max_move) {
  torch::NoGradGuard g;
  if (passes < 0) throw std::invalid_argument("mesh_smooth: passes must be >= 0");
  if (!std::isfinite(lam) || !std::isfinite(mu)) throw std::invalid_argument("mesh_smooth: lam and mu must be finite");
  if (!(max_move > 0.f)) throw std::invalid_argument("mesh_smooth: max_move must be > 0 (inf: no clamp)");
  Tensor v = Points3(verts);
  const int64_t nv = v.size(0), ne = ring.ring.size(0);
  TORCH_CHECK(ring.start_end.size(0) == nv && ring.pinned.size(0) == nv, "mesh_smooth: the ring does not belong to these vertices");
  Tensor a = v.clone();
  if (nv == 0 || passes == 0) return a;
  Tensor b = torch::empty_like(a);
  auto pass = [&](const Tensor& src, const Tensor& dst, double factor) {
    F2N_TIMED_CALL("mesh_smooth", f2n_mesh_smooth(CurStream(), (int) nv, (int) ne, F32P(src), I32P(ring.start_end),
                                                  ne > 0 ? I32P(ring.ring) : nullptr, ring.pinned.data_ptr<uint8_t>(), factor, F32P(dst)));
  };
  for (int p = 0; p < passes; p++) {
    pass(a, b, lam);
    pass(b, a, mu);
  }
  if (std::isfinite(max_move)) F2N_TIMED_CALL("mesh_move_clamp", f2n_mesh_move_clamp(CurStream(), (int) nv, F32P(v), max_move, F32P(a)));
  return a;
}

Tensor MeshSmooth(const Tensor& verts, const Tensor& faces, int passes, double lam, double mu, float max_move) {
  Tensor v = Points3(verts);
  return MeshSmoothOnRing(v, MeshRing(faces, v.size(0)), passes, lam, mu, max_move);
}

Tensor MeshFaceQuality(const Tensor& verts, const Tensor& faces) {
  torch::NoGradGuard g;
  Tensor v = Points3(verts);
  Tensor f = faces.to(torch::kCUDA, torch::kInt32).contiguous().view({-1, 3});
  const int64_t nv = v.size(0), nf = f.size(0);
  TORCH_CHECK(nf <= INT32_MAX, "mesh too large");
  Tensor q = torch::empty({nf}, DevF32().dtype(torch::kFloat64));
  if (nf > 0)
    F2N_TIMED_CALL("mesh_face_quality", f2n_mesh_face_quality(CurStream(), (int) nv, (int) nf, nv > 0 ? F32P(v) : nullptr, I32P(f),
                                                              q.data_ptr<double>()));
  return q;
}

void LevelStep(bool first, bool propose, const Tensor& p0, const Tensor& sigma, const Tensor& grad, const Tensor& h, float tol, float max_step,
               float max_move, const Tensor& cand, const Tensor& best, const Tensor& h_best, const Tensor& g_best, const Tensor& scale,
               const Tensor& status, const Tensor& evals) {
  torch::NoGradGuard g;
  if (!(tol >= 0.f) || !(max_step > 0.f) || !(max_move > 0.f))
    throw std::invalid_argument("level_step: tol must be >= 0, max_step and max_move > 0");
  const int64_t n = DevArg(p0, torch::kFloat32, "p0").numel() / 3;
  TORCH_CHECK(n <= INT32_MAX, "too many points");
  for (const Tensor* t : {&p0, &grad, &cand, &best, &g_best})
    TORCH_CHECK(DevArg(*t, torch::kFloat32, "a [n,3] array").dim() == 2 && t->size(0) == n && t->size(1) == 3, "level_step: p0, grad, cand, best and g_best must be [n,3]");
  for (const Tensor* t : {&sigma, &h, &h_best, &scale})
    TORCH_CHECK(DevArg(*t, torch::kFloat32, "a [n] array").dim() == 1 && t->size(0) == n, "level_step: sigma, h, h_best and scale must be [n]");
  for (const Tensor* t : {&status, &evals})
    TORCH_CHECK(DevArg(*t, torch::kInt32, "status / evals").dim() == 1 && t->size(0) == n, "level_step: status and evals must be [n] int32");
  if (n == 0) return;
  F2N_TIMED_CALL("level_step", f2n_level_step(CurStream(), (int) n, first ? 1 : 0, propose ? 1 : 0, F32P(p0), F32P(sigma), F32P(grad), F32P(h), tol,
                                              max_step, max_move, F32P(cand), F32P(best), F32P(h_best), F32P(g_best), F32P(scale), I32P(status),
                                              I32P(evals)));
}

namespace {
// per coordinate, over its finite values: (min [3], max [3]) on the host; min > max for a coordinate without a finite value
void FiniteBox(const Tensor& v, float mn[3], float mx[3]) {
  Tensor fin = torch::isfinite(v);
  const float inf = std::numeric_limits<float>::infinity();
  Tensor lows = torch::where(fin, v, torch::full({1}, inf, DevF32())), highs = torch::where(fin, v, torch::full({1}, -inf, DevF32()));
  std::vector<Tensor> ends;
  for (int k = 0; k < 3; k++) ends.push_back(lows.select(1, k).min());
  for (int k = 0; k < 3; k++) ends.push_back(highs.select(1, k).max());
  Tensor box = torch::stack(ends).cpu();
  for (int k = 0; k < 3; k++) {
    mn[k] = box.data_ptr<float>()[k];
    mx[k] = box.data_ptr<float>()[3 + k];
  }
}
}  // namespace

float MeshRaycastDefaultCell(const float mn[3], const float mx[3], int64_t n_faces) {
  double e[3], longest = 0.0;
  for (int k = 0; k < 3; k++) {
    e[k] = mn[k] <= mx[k] ? (double) mx[k] - (double) mn[k] : 0.0;
    longest = std::max(longest, e[k]);
  }
  const double area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0]);
  const double cell = std::max(std::sqrt(10.0 * area / (double) std::max<int64_t>(n_faces, 1)), longest / 500.0);
  return cell > 0.0 && std::isfinite(cell) && (float) cell > 0.f && std::isfinite((float) cell) ? (float) cell : 1.f;
}

MeshRaycastAccel MeshRaycastBuild(const Tensor& verts, const Tensor& faces, float cell_in, const float* lo_in) {
  torch::NoGradGuard g;
  Tensor v = Points3(verts);
  Tensor f = faces.to(torch::kCUDA, torch::kInt32).contiguous().view({-1, 3});
  const int64_t nv = v.size(0), nf = f.size(0);
  TORCH_CHECK(nf <= INT32_MAX, "mesh too large");
  MeshRaycastAccel a;
  float mn[3] = {1.f, 1.f, 1.f}, mx[3] = {0.f, 0.f, 0.f};
  if (nv > 0) FiniteBox(v, mn, mx);
  const bool given = !std::isnan(cell_in);  // (NaN: the default)
  a.cell = given ? cell_in : MeshRaycastDefaultCell(mn, mx, nf);
  if (!(a.cell > 0.f) || !std::isfinite(a.cell)) throw std::invalid_argument("mesh_raycast_build: cell must be positive and finite");
  double ncells = 1.0;
  for (int k = 0; k < 3; k++) {
    a.lo[k] = lo_in != nullptr ? lo_in[k] : 0.f;
    a.dims[k] = 1;
    if (!std::isfinite(a.lo[k])) throw std::invalid_argument("mesh_raycast_build: lo must be finite");
    if (mn[k] <= mx[k]) {  // (the coordinate has a finite value)
      if (lo_in == nullptr) a.lo[k] = mn[k];
      if (a.lo[k] > mn[k]) throw std::invalid_argument("mesh_raycast_build: the grid must cover the mesh (lo above a vertex)");
      const float u = (mx[k] - a.lo[k]) / a.cell;  // (two fp32 roundings, as the cell index's u)
      if (!(u < 1048575.f)) throw std::invalid_argument("mesh_raycast_build: cell is too small for the extent of the mesh");
      a.dims[k] = (int) std::floor(u) + 1;
    }
    ncells *= (double) a.dims[k];
  }
  if (ncells > (double) (1 << 27)) throw std::invalid_argument("mesh_raycast_build: more than 2^27 cells (cell is too small for the mesh)");
  const int64_t nc = (int64_t) ncells;
  Tensor counts = torch::zeros({nf}, DevI32()), flag = torch::empty({1}, DevI32());
  F2N_TIMED_CALL("mesh_raycast_count", f2n_mesh_raycast_count(CurStream(), (int) nv, (int) nf, F32P(v), I32P(f), a.lo, a.cell, a.dims,
                                                              I32P(counts), I32P(flag)));
  Tensor keys;
  {
    TimedSpan span("mesh_raycast_sort");
    Tensor ends = counts.cumsum(0, torch::kInt64);
    const int64_t total = nf > 0 ? ends[nf - 1].item<int64_t>() : 0;
    if (total > INT32_MAX) throw std::invalid_argument("mesh_raycast_build: more than 2^31 list entries (cell is too small for the mesh)");
    Tensor offsets = (ends - counts).contiguous();
    keys = torch::empty({total}, DevI32().dtype(torch::kInt64));
    if (total > 0)
      F2N_CALL(f2n_mesh_raycast_fill(CurStream(), (int) nv, (int) nf, F32P(v), I32P(f), a.lo, a.cell, a.dims, offsets.data_ptr<int64_t>(),
                                     keys.data_ptr<int64_t>()));
    keys = std::get<0>(torch::sort(keys));
    const int64_t m = std::max<int64_t>(nf, 1);
    Tensor firsts = torch::arange(nc + 1, DevI32().dtype(torch::kInt64)) * m;
    a.cell_start = torch::searchsorted(keys, firsts).to(torch::kInt32).contiguous();
    a.cell_faces = torch::remainder(keys, m).to(torch::kInt32).contiguous();
  }
  return a;
}

std::tuple<Tensor, Tensor, Tensor> MeshRaycast(const Tensor& verts, const Tensor& faces, const MeshRaycastAccel* accel, const Tensor& rays_o,
                                               const Tensor& rays_d, const Tensor& bounds) {
  torch::NoGradGuard g;
  Tensor v = Points3(verts), o = Points3(rays_o), d = Points3(rays_d);
  Tensor f = faces.to(torch::kCUDA, torch::kInt32).contiguous().view({-1, 3});
  const int64_t nv = v.size(0), nf = f.size(0), R = o.size(0);
  TORCH_CHECK(nf <= INT32_MAX && d.size(0) == R, "mesh too large, or rays_o and rays_d differ in size");
  Tensor b;
  if (bounds.defined()) {
    b = bounds.to(torch::kCUDA, torch::kFloat32).contiguous().view({-1, 2});
    TORCH_CHECK(b.size(0) == R, "bounds must be [R,2]");
  }
  Tensor t = torch::zeros({R}, DevF32()), face = torch::full({R}, -1, DevI32()), bary = torch::zeros({R, 3}, DevF32());
  if (accel != nullptr) {
    TORCH_CHECK(accel->cell_start.defined() && accel->cell_faces.defined(), "mesh_raycast: the accel has no cell lists");
    const int64_t nc = (int64_t) accel->dims[0] * accel->dims[1] * accel->dims[2];
    if (accel->cell_start.numel() != nc + 1) throw std::invalid_argument("mesh_raycast: cell_start does not match dims");
    // the traversal's domain (include/f2n_abi.h): every coordinate of the box and of the origins within 2^15 cells of the frame's origin
    float far = 0.f;
    for (int k = 0; k < 3; k++)
      far = std::max(far, std::max(std::fabs(accel->lo[k]), std::fabs(accel->lo[k] + (float) accel->dims[k] * accel->cell)));
    if (R > 0) {
      const float fo = o.abs().max().item<float>();  // (NaN propagates: an origin that is not finite is outside the domain)
      far = std::isnan(fo) ? fo : std::max(far, fo);
    }
    if (!(far <= 32768.f * accel->cell))
      throw std::invalid_argument("mesh_raycast: a ray origin (or the grid) lies more than 2^15 cells from the frame's origin: outside the "
                                  "domain in which the grid traversal is exact; use a larger cell or accel=None");
  }
  Tensor cs = accel != nullptr ? DevArg(accel->cell_start, torch::kInt32, "cell_start") : Tensor();
  Tensor cf = accel != nullptr ? DevArg(accel->cell_faces, torch::kInt32, "cell_faces") : Tensor();
  F2N_TIMED_CALL(accel != nullptr ? "mesh_raycast" : "mesh_raycast_brute",
                 f2n_mesh_raycast(CurStream(), (int) nv, (int) nf, F32P(v), I32P(f), accel != nullptr ? accel->lo : nullptr,
                                  accel != nullptr ? accel->cell : 0.f, accel != nullptr ? accel->dims : nullptr,
                                  accel != nullptr ? I32P(cs) : nullptr, accel != nullptr && cf.numel() > 0 ? I32P(cf) : nullptr, (int) R,
                                  F32P(o), F32P(d), b.defined() ? F32P(b) : nullptr, F32P(t), I32P(face), F32P(bary)));
  return {t, face, bary};
}

std::tuple<Tensor, Tensor, Tensor> MeshClosestPoint(const Tensor& verts, const Tensor& faces, const MeshRaycastAccel* accel, const Tensor& points,
                                                    float max_dist) {
  torch::NoGradGuard g;
  Tensor v = Points3(verts), p = Points3(points);
  Tensor f = faces.to(torch::kCUDA, torch::kInt32).contiguous().view({-1, 3});
  const int64_t nv = v.size(0), nf = f.size(0), N = p.size(0);
  TORCH_CHECK(nf <= INT32_MAX && N <= INT32_MAX, "mesh or point set too large");
  if (!(max_dist >= 0.f)) throw std::invalid_argument("mesh_closest_point: max_dist must be >= 0 (inf: no cut-off)");
  const float inf = std::numeric_limits<float>::infinity();
  Tensor dist = torch::full({N}, inf, DevF32()), face = torch::full({N}, -1, DevI32()), bary = torch::zeros({N, 3}, DevF32());
  if (accel != nullptr) {
    TORCH_CHECK(accel->cell_start.defined() && accel->cell_faces.defined(), "mesh_closest_point: the accel has no cell lists");
    const int64_t nc = (int64_t) accel->dims[0] * accel->dims[1] * accel->dims[2];
    if (accel->cell_start.numel() != nc + 1) throw std::invalid_argument("mesh_closest_point: cell_start does not match dims");
    // the walk's domain (include/f2n_abi.h): every coordinate of the box and of the finite points within 2^15 cells of the frame's origin
    float far = 0.f;
    for (int k = 0; k < 3; k++)
      far = std::max(far, std::max(std::fabs(accel->lo[k]), std::fabs(accel->lo[k] + (float) accel->dims[k] * accel->cell)));
    if (N > 0) far = std::max(far, torch::where(torch::isfinite(p), p.abs(), torch::zeros({1}, DevF32())).max().item<float>());
    if (!(far <= 32768.f * accel->cell))
      throw std::invalid_argument("mesh_closest_point: a point (or the grid) lies more than 2^15 cells from the frame's origin: outside the "
                                  "domain in which the grid walk is exact; use a larger cell or accel=None");
  }
  Tensor cs = accel != nullptr ? DevArg(accel->cell_start, torch::kInt32, "cell_start") : Tensor();
  Tensor cf = accel != nullptr ? DevArg(accel->cell_faces, torch::kInt32, "cell_faces") : Tensor();
  F2N_TIMED_CALL(accel != nullptr ? "mesh_closest_point" : "mesh_closest_point_brute",
                 f2n_mesh_closest_point(CurStream(), (int) nv, (int) nf, F32P(v), I32P(f), accel != nullptr ? accel->lo : nullptr,
                                        accel != nullptr ? accel->cell : 0.f, accel != nullptr ? accel->dims : nullptr,
                                        accel != nullptr ? I32P(cs) : nullptr, accel != nullptr && cf.numel() > 0 ? I32P(cf) : nullptr, (int) N,
                                        F32P(p), max_dist, F32P(dist), I32P(face), F32P(bary)));
  return {dist, face, bary};
}

std::tuple<Tensor, Tensor, Tensor> MeshSampleSurface(const Tensor& verts, const Tensor& faces, int64_t n, uint64_t seed) {
  torch::NoGradGuard g;
  Tensor v = Points3(verts);
  Tensor f = faces.to(torch::kCUDA, torch::kInt32).contiguous().view({-1, 3});
  const int64_t nv = v.size(0), nf = f.size(0);
  TORCH_CHECK(nf <= INT32_MAX, "mesh too large");
  if (n < 0 || n > INT32_MAX) throw std::invalid_argument("mesh_sample_surface: n must lie in [0, 2^31)");
  const auto f64 = DevF32().dtype(torch::kFloat64), i64 = DevI32().dtype(torch::kInt64);
  Tensor area2 = torch::zeros({nf}, f64), weights = torch::zeros({nf}, i64);
  if (nf > 0)
    F2N_TIMED_CALL("mesh_face_weights", f2n_mesh_face_weights(CurStream(), (int) nv, (int) nf, F32P(v), I32P(f), 0.0, area2.data_ptr<double>(),
                                                              nullptr));
  const double largest = nf > 0 ? area2.max().item<double>() : 0.0;
  if (!(largest > 0.0)) throw std::invalid_argument("mesh_sample_surface: the mesh has no face with an area");
  F2N_TIMED_CALL("mesh_face_weights", f2n_mesh_face_weights(CurStream(), (int) nv, (int) nf, F32P(v), I32P(f), largest * 0x1p-31, nullptr,
                                                            weights.data_ptr<int64_t>()));
  Tensor cum = weights.cumsum(0).contiguous();
  Tensor pts = torch::empty({n, 3}, DevF32()), face = torch::empty({n}, DevI32()), bary = torch::empty({n, 3}, DevF32());
  F2N_TIMED_CALL("mesh_sample_surface", f2n_mesh_sample_surface(CurStream(), (int) nv, (int) nf, F32P(v), I32P(f), cum.data_ptr<int64_t>(), (int) n,
                                                                seed ^ kMeshSamplePurpose, F32P(pts), I32P(face), F32P(bary)));
  return {pts, face, bary};
}

MeshAtlasResult MeshAtlas(const Tensor& verts, const Tensor& faces, float density, int max_size, int max_log) {
  torch::NoGradGuard g;
  Tensor v = Points3(verts);
  Tensor f = faces.to(torch::kCUDA, torch::kInt32).contiguous().view({-1, 3});
  const int64_t nv = v.size(0), nf = f.size(0);
  TORCH_CHECK(nf <= INT32_MAX, "mesh too large");
  if (max_size < 4 || (max_size & (max_size - 1)) != 0) throw std::invalid_argument("mesh_atlas: max_size must be a power of two, at least 4");
  if (max_log < 2 || max_log > 13) throw std::invalid_argument("mesh_atlas: max_log must lie in [2, 13]");
  if (!(density > 0.f) || !std::isfinite(density)) throw std::invalid_argument("mesh_atlas: density must be positive and finite");
  {  // the layout with every block at its minimum of 4 x 4 texels: two faces to a block
    int64_t least = 4;
    while (least * least < 16 * ((nf + 1) / 2)) least *= 2;
    if (least > max_size) throw std::invalid_argument("mesh_atlas: the mesh does not fit max_size even at the smallest block size");
  }
  const auto i64 = DevI32().dtype(torch::kInt64);
  const int64_t m = std::max<int64_t>(nf, 1), ncls = max_log - 1;
  MeshAtlasResult a;
  a.log_s = torch::empty({nf}, DevI32());
  a.rot = torch::empty({nf}, DevI32());
  for (int round = 0; round <= 32; round++, density *= 0.5f) {
    if (!(density > 0.f)) break;
    F2N_TIMED_CALL("atlas_classify", f2n_atlas_classify(CurStream(), (int) nv, (int) nf, F32P(v), I32P(f), density, max_log, I32P(a.log_s),
                                                        I32P(a.rot)));
    TimedSpan span("atlas_layout");
    // classes descending, faces ascending within a class; positions 2j and 2j + 1 of a class share its block j
    Tensor keys = std::get<0>(torch::sort((max_log - a.log_s.to(torch::kInt64)) * m + torch::arange(nf, i64)));
    Tensor order = torch::remainder(keys, m), cls = torch::floor_divide(keys, m);
    Tensor n_c = torch::bincount(cls, {}, ncls);
    Tensor nb_c = torch::floor_divide(n_c + 1, 2);
    Tensor c0 = n_c.cumsum(0) - n_c, b0 = nb_c.cumsum(0) - nb_c;
    Tensor q = torch::arange(nf, i64) - c0.index_select(0, cls);
    Tensor sl = (b0.index_select(0, cls) + torch::floor_divide(q, 2)) * 2 + torch::remainder(q, 2);
    const int64_t B = nb_c.sum().item<int64_t>();
    a.block_log = (max_log - torch::repeat_interleave(torch::arange(ncls, i64), nb_c)).to(torch::kInt32).contiguous();
    Tensor areas = torch::bitwise_left_shift(torch::ones({B}, i64), a.block_log.to(torch::kInt64) * 2);
    a.offsets = torch::cat({torch::zeros({1}, i64), areas.cumsum(0)}).contiguous();
    const int64_t total = a.offsets[B].item<int64_t>();
    int64_t size = 4;
    while (size * size < total) size *= 2;
    if (size > max_size) continue;
    a.slot = torch::zeros({nf}, DevI32());
    a.slot.index_put_({order}, sl.to(torch::kInt32));
    Tensor bf = torch::full({B * 2}, -1, DevI32());
    bf.index_put_({sl}, order.to(torch::kInt32));
    a.block_faces = bf.view({B, 2});
    a.size = (int) size;
    a.density_used = density;
    a.uv = torch::zeros({nf, 3, 2}, DevF32());
    F2N_TIMED_CALL("atlas_place", f2n_atlas_place(CurStream(), (int) nf, (int) B, a.size, I32P(a.log_s), I32P(a.rot), I32P(a.slot),
                                                  a.offsets.data_ptr<int64_t>(), F32P(a.uv)));
    return a;
  }
  throw std::invalid_argument("mesh_atlas: the mesh does not fit max_size after 32 halvings of the density");
}

std::tuple<Tensor, Tensor, Tensor> MeshAtlasTexels(const Tensor& verts, const Tensor& faces, const MeshAtlasResult& a, bool clamp) {
  torch::NoGradGuard g;
  Tensor v = Points3(verts);
  Tensor f = faces.to(torch::kCUDA, torch::kInt32).contiguous().view({-1, 3});
  const int64_t nv = v.size(0), nf = f.size(0), S = a.size;
  DevArg(a.offsets, torch::kInt64, "offsets");
  DevArg(a.block_log, torch::kInt32, "block_log");
  DevArg(a.block_faces, torch::kInt32, "block_faces");
  DevArg(a.rot, torch::kInt32, "rot");
  const int64_t B = a.block_log.numel();
  if (S < 4 || S > 8192 || (S & (S - 1)) != 0) throw std::invalid_argument("mesh_atlas_texels: size must be a power of two in [4, 8192]");
  if (a.offsets.numel() != B + 1 || a.block_faces.numel() != 2 * B || a.rot.numel() != nf)
    throw std::invalid_argument("mesh_atlas_texels: blocks do not match (offsets [B+1], block_faces [B,2], rot [F])");
  Tensor tex_face = torch::empty({S, S}, DevI32()), tex_bary = torch::empty({S, S, 3}, DevF32()), tex_pos = torch::empty({S, S, 3}, DevF32());
  // above 4096^2 texels in row bands (16 M lanes a launch); the kernel writes the outputs in place, so there is no workspace
  const int64_t band = std::max<int64_t>(16, (int64_t) 4096 * 4096 / S);
  for (int64_t y = 0; y < S; y += band)
    F2N_TIMED_CALL("atlas_texels", f2n_atlas_texels(CurStream(), (int) nv, (int) nf, F32P(v), I32P(f), (int) B, (int) S,
                                                    a.offsets.data_ptr<int64_t>(), B > 0 ? I32P(a.block_log) : nullptr,
                                                    B > 0 ? I32P(a.block_faces) : nullptr, I32P(a.rot), clamp ? 1 : 0, (int) y,
                                                    (int) std::min(S, y + band), I32P(tex_face), F32P(tex_bary), F32P(tex_pos)));
  return {tex_face, tex_bary, tex_pos};
}

Tensor TextureSample(const Tensor& tex, const Tensor& uv) {
  torch::NoGradGuard g;
  Tensor t = tex.to(torch::kCUDA, torch::kFloat32).contiguous();
  Tensor u = uv.to(torch::kCUDA, torch::kFloat32).contiguous().view({-1, 2});
  if (t.dim() != 3 || t.size(0) != t.size(1) || t.size(0) < 1 || t.size(0) > 32768 || t.size(2) < 1 || t.size(2) > 64)
    throw std::invalid_argument("texture_sample: tex must be [S,S,C] with S in [1, 32768] and C in [1, 64]");
  Tensor out = torch::empty({u.size(0), t.size(2)}, DevF32());
  F2N_TIMED_CALL("texture_sample", f2n_texture_sample(CurStream(), (int) t.size(0), (int) t.size(2), F32P(t), u.size(0), F32P(u), F32P(out)));
  return out;
}

std::tuple<double, Tensor, Tensor> ImageSSIM(const Tensor& a, const Tensor& b, double max_val, int filter_size, double sigma, double k1, double k2,
                                             bool return_map) {
  torch::NoGradGuard g;
  static const char* rules =
      "image_ssim: a and b must be float32 [H,W,C] of one shape with C in [1, 4], filter_size in [1, 33] and at most min(H, W), "
      "(H - filter_size + 1) (W - filter_size + 1) <= 2^26, filter_sigma > 0 and finite";
  if (a.dim() != 3 || a.sizes() != b.sizes() || a.scalar_type() != torch::kFloat32 || b.scalar_type() != torch::kFloat32)
    throw std::invalid_argument(rules);
  const int64_t H = a.size(0), W = a.size(1), C = a.size(2);
  if (C < 1 || C > 4 || filter_size < 1 || filter_size > 33 || filter_size > std::min(H, W) || !(sigma > 0.0) || !std::isfinite(sigma) ||
      (H - filter_size + 1) * (W - filter_size + 1) > ((int64_t) 1 << 26))
    throw std::invalid_argument(rules);
  Tensor x = a.to(torch::kCUDA).contiguous(), y = b.to(torch::kCUDA).contiguous();
  double window[33];
  if (f2n_ssim_window(filter_size, sigma, window) != F2N_OK) throw std::invalid_argument(rules);
  const double c1 = (k1 * max_val) * (k1 * max_val), c2 = (k2 * max_val) * (k2 * max_val);
  const int64_t oh = H - filter_size + 1, ow = W - filter_size + 1;
  Tensor stats = torch::empty({C, 2}, torch::TensorOptions().dtype(torch::kInt64).device(torch::kCUDA));
  Tensor map;
  if (return_map) map = torch::empty({oh, ow, C}, torch::TensorOptions().dtype(torch::kFloat64).device(torch::kCUDA));
  F2N_TIMED_CALL("image_ssim", f2n_image_ssim(CurStream(), (int) H, (int) W, (int) C, F32P(x), F32P(y), window, filter_size, c1, c2,
                                              return_map ? map.data_ptr<double>() : nullptr, stats.data_ptr<int64_t>()));
  Tensor st = stats.cpu();
  const int64_t* s = st.data_ptr<int64_t>();
  const double n = (double) (oh * ow), nan = std::numeric_limits<double>::quiet_NaN();
  Tensor per = torch::empty({C}, torch::kFloat64);
  int64_t total = 0;
  bool all = true;
  for (int64_t c = 0; c < C; c++) {
    const bool full = s[2 * c + 1] == oh * ow;
    per.data_ptr<double>()[c] = full ? (double) s[2 * c] / (68719476736.0 * n) : nan;
    total += s[2 * c];
    all = all && full;
  }
  return {all ? (double) total / (68719476736.0 * (n * (double) C)) : nan, per, map};
}

LevelProjection Renderer::ProjectToLevel(const Tensor& points, float level, int iters, float max_step, float max_move, float tol,
                                         const Tensor& origins) {
  torch::NoGradGuard g;
  TORCH_CHECK(global_data_pool_->mode_ != RunningMode::TRAIN, "ProjectToLevel is an inference path");
  if (!(level > 0.f) || !std::isfinite(level)) throw std::invalid_argument("project_to_level: level must be positive and finite");
  if (iters < 1) throw std::invalid_argument("project_to_level: iters must be >= 1 (it counts field evaluations)");
  if (!(max_step > 0.f) || !(max_move > 0.f) || !(tol >= 0.f))
    throw std::invalid_argument("project_to_level: max_step and max_move must be > 0, tol >= 0");
  Tensor start = Points3(points);
  Tensor p0 = origins.defined() ? Points3(origins) : start;
  const int64_t n = start.size(0);
  TORCH_CHECK(p0.size(0) == n, "project_to_level: one origin per point");
  LevelProjection out;
  out.points = torch::empty({n, 3}, DevF32());
  out.h_in = torch::empty({n}, DevF32());
  out.h_out = torch::empty({n}, DevF32());
  out.status = torch::empty({n}, DevI32());
  out.evals = torch::empty({n}, DevI32());
  const Tensor log_level = torch::log(torch::full({1}, level, DevF32()));
  for (int64_t i0 = 0; i0 < n; i0 += density_slab_points_) {  // (bounded workspaces, as DensityGradSlabs)
    const int64_t c = std::min(density_slab_points_, n - i0);
    Tensor cand = start.narrow(0, i0, c).clone(), origin = p0.narrow(0, i0, c);
    Tensor best = out.points.narrow(0, i0, c), h_best = out.h_out.narrow(0, i0, c), status = out.status.narrow(0, i0, c);
    Tensor evals = out.evals.narrow(0, i0, c);
    Tensor g_best = torch::empty({c, 3}, DevF32()), scale = torch::empty({c}, DevF32());
    Tensor sigma = torch::empty({c}, DevF32()), grad = torch::empty({c, 3}, DevF32());
    for (int k = 0; k < iters; k++) {
      DensityGradChunk(cand, sigma, grad, Tensor());
      Tensor h = (torch::log(sigma) - log_level).contiguous();
      if (k == 0) out.h_in.narrow(0, i0, c).copy_(h);
      LevelStep(k == 0, k + 1 < iters, origin, sigma, grad, h, tol, max_step, max_move, cand, best, h_best, g_best, scale, status, evals);
    }
  }
  return out;
}

namespace {
// the values of the sorted 1-d tensor at the given fractions of its length ("lower": index floor(q (n - 1))); NaN for an empty tensor
std::vector<double> SortedAt(const Tensor& x, const std::vector<double>& qs) {
  std::vector<double> out;
  const int64_t n = x.numel();
  Tensor s = n > 0 ? std::get<0>(torch::sort(x.to(torch::kFloat64).view({-1}))) : x;
  std::vector<int64_t> at;
  for (double q : qs) at.push_back(n > 0 ? (int64_t) std::floor(q * (double) (n - 1)) : 0);
  Tensor picked = n > 0 ? s.index_select(0, torch::tensor(at, torch::kInt64).to(s.device())).cpu() : Tensor();
  for (size_t k = 0; k < qs.size(); k++) out.push_back(n > 0 ? picked.data_ptr<double>()[k] : std::numeric_limits<double>::quiet_NaN());
  return out;
}

Tensor FaceNormalsF64(const Tensor& verts, const Tensor& faces) {
  Tensor v = verts.to(torch::kFloat64), f = faces.to(torch::kInt64);
  Tensor a = v.index_select(0, f.select(1, 0)), b = v.index_select(0, f.select(1, 1)), c = v.index_select(0, f.select(1, 2));
  return torch::cross(b - a, c - a, 1);
}
}  // namespace

MeshAttrs Renderer::ExtractMeshAttrs(const std::vector<float>& lo, const std::vector<float>& hi, int res, float level,
                                     int min_component_faces, bool normals, bool colors, const std::string& normal_source, int simplify,
                                     const MeshRefineOptions& refine, int sparse) {
  torch::NoGradGuard g;
  const bool from_field = normal_source == "field";
  TORCH_CHECK(from_field || normal_source == "grid", "normal_source must be \"grid\" or \"field\", got \"", normal_source, "\"");
  if (sparse != 0 && !from_field && (normals || colors))
    throw std::invalid_argument("extract_mesh_attrs: sparse extraction builds no dense grid; normals and colours need normal_source=\"field\"");
  const GridSpec s = MakeGridSpec(lo, hi, res, sparse != 0 ? kSparseMaxRes : 1024);
  Tensor grid;  // (stays undefined in sparse mode)
  MeshAttrs out;
  if (sparse != 0) {
    std::tie(out.verts, out.faces) = ExtractMeshSparse(lo, hi, res, level, sparse, &out.sparse);
  } else {
    grid = DensityGrid(lo, hi, res);
    std::tie(out.verts, out.faces) = MeshFromGrid(grid, level, s.lo, s.step);
  }
  if (min_component_faces > 1) {
    auto kept = MeshFilterComponents(out.verts, out.faces, min_component_faces);
    out.verts = std::get<0>(kept);
    out.faces = std::get<1>(kept);
  }
  if (simplify >= 2) {  // clusters of simplify^3 grid cells; the attributes below are computed at the new vertices
    out.verts_in = out.verts.size(0);
    out.faces_in = out.faces.size(0);
    auto simple = MeshSimplify(out.verts, out.faces, (float) simplify * s.step, s.lo, 1e-3);
    out.verts = std::get<0>(simple);
    out.faces = std::get<1>(simple);
  }
  if (refine.on) {  // smooth, then project onto the level set; the attributes below are computed at the refined vertices
    const float unit = simplify >= 2 ? (float) simplify * s.step : s.step;
    const float max_step = refine.max_step_steps * unit, max_move = refine.max_move_steps * unit;
    if (!(max_step > 0.f) || !(max_move > 0.f)) throw std::invalid_argument("refine: max_step_steps and max_move_steps must be > 0");
    if (refine.smooth_passes < 0) throw std::invalid_argument("refine: smooth_passes must be >= 0");
    auto& st = out.refine;
    const Tensor v0 = out.verts;
    const int64_t nv = v0.size(0);
    MeshRingResult ring = MeshRing(out.faces, nv);
    Tensor q0 = MeshFaceQuality(v0, out.faces);
    Tensor v = refine.smooth_passes > 0 ? MeshSmoothOnRing(v0, ring, refine.smooth_passes, refine.lam, refine.mu, max_move) : v0;
    st.emplace_back("smooth_passes", refine.smooth_passes);
    st.emplace_back("project", refine.project ? 1 : 0);
    st.emplace_back("max_step", max_step);
    st.emplace_back("max_move", max_move);
    st.emplace_back("points", (double) nv);
    if (refine.project) {
      LevelProjection pr = ProjectToLevel(v, level, refine.iters, max_step, max_move, refine.tol, v0);
      v = pr.points;
      Tensor live = (pr.status.bitwise_and(F2N_LEVEL_EMPTY) == 0);
      const char* names[4] = {"empty", "converged", "step_clamped", "move_clamped"};
      const int bits[4] = {F2N_LEVEL_EMPTY, F2N_LEVEL_CONVERGED, F2N_LEVEL_STEP_CLAMPED, F2N_LEVEL_MOVE_CLAMPED};
      for (int k = 0; k < 4; k++) st.emplace_back(names[k], (double) (pr.status.bitwise_and(bits[k]) != 0).sum().item<int64_t>());
      st.emplace_back("evals", (double) pr.evals.sum(torch::kInt64).item<int64_t>());
      const auto before = SortedAt(pr.h_in.masked_select(live).abs(), {0.5, 0.9});
      const auto after = SortedAt(pr.h_out.masked_select(live).abs(), {0.5, 0.9});
      st.emplace_back("h_median_before", before[0]);
      st.emplace_back("h_p90_before", before[1]);
      st.emplace_back("h_median_after", after[0]);
      st.emplace_back("h_p90_after", after[1]);
    }
    const auto moved = SortedAt((v.to(torch::kFloat64) - v0.to(torch::kFloat64)).norm(2, 1) / (double) s.step, {0.5, 0.9, 1.0});
    st.emplace_back("moved_median", moved[0]);
    st.emplace_back("moved_p90", moved[1]);
    st.emplace_back("moved_max", moved[2]);
    const auto qb = SortedAt(q0, {0.5, 0.05}), qa = SortedAt(MeshFaceQuality(v, out.faces), {0.5, 0.05});
    st.emplace_back("quality_median_before", qb[0]);
    st.emplace_back("quality_p05_before", qb[1]);
    st.emplace_back("quality_median_after", qa[0]);
    st.emplace_back("quality_p05_after", qa[1]);
    const int64_t flipped =
        out.faces.size(0) > 0 ? ((FaceNormalsF64(v0, out.faces) * FaceNormalsF64(v, out.faces)).sum(1) < 0).sum().item<int64_t>() : 0;
    st.emplace_back("flipped_faces", (double) flipped);
    Tensor ec = ring.edge_counts.cpu();
    st.emplace_back("boundary_edges", (double) ec.data_ptr<int32_t>()[0]);
    st.emplace_back("nonmanifold_edges", (double) ec.data_ptr<int32_t>()[1]);
    out.verts = v.contiguous();
  }
  if (!normals && !colors) return out;
  Tensor nrm;
  if (sparse != 0) {  // the field's own gradient alone: (0, 0, 0) where it vanishes
    nrm = FieldNormals(out.verts);
  } else {
    nrm = GridNormals(grid, out.verts, s.lo, s.step);
  }
  if (from_field && sparse == 0) {  // the field's own gradient at the vertex; the grid's where that vanishes
    Tensor fn = FieldNormals(out.verts);
    nrm = torch::where((fn == 0).all(1, /*keepdim=*/true), nrm, fn).contiguous();
  }
  if (normals) out.normals = nrm;
  if (colors) {
    // a vertex colour is the radiance AT the vertex seen along the inward normal (by a viewer in front of the surface)
    Tensor flat = (nrm == 0).all(1, /*keepdim=*/true);
    Tensor fallback = torch::tensor({0.f, 0.f, -1.f}, DevF32()).view({1, 3});
    Tensor dirs = torch::where(flat, fallback, -nrm).contiguous();
    out.colors = std::get<1>(QueryRadiance(out.verts, dirs));  // (the shader's range: [-1e-3, 1 + 1e-3]; mesh.write_ply clips)
  }
  return out;
}

}  // namespace f2n
