// Renderer glue on gfx950: early-stop pre-pass, sample compaction, volume-rendering compositing forward /
// backward, WeightVar loss and the seam-level FlexOps.  Semantics: Renderer/Renderer.cpp:105-208,
// Renderer/Renderer.cu:8-50, Utils/CustomOps/{FlexOps.cu:5-93, CustomOps.cu:12-80, CustomOps.cpp:9-18}.
// The per-ray fp32 accumulations add left to right, one term after the other, because that order is part of the
// parity contract; everything that the reference spreads over a dozen ATen element-wise
// launches is done inside the same walk.
#include "rows_dev.h"

// Every walk below keeps the NEXT 16-sample chunk's loads in flight while the current chunk goes through its exp /
// division / scan chain: with 4 rays per wave and the kernel's tail being its longest ray (400 samples on a converged
// scene = 25 chunks per walk), a load issued where its value is used exposed a full HBM round trip per chunk and walk --
// that, not arithmetic, was ~80 % of the compositing kernels' time (converged scene: backward 0.16 ms for 2.6e5 samples).

// Renderer.cpp:115-126
__global__ __launch_bounds__(256) void early_stop_kernel(int n_rays, const int32_t* __restrict__ se, const float* __restrict__ f0,
                                                         int f0_stride, const float* __restrict__ dt, float* __restrict__ weights,
                                                         float* __restrict__ alphas, int32_t* __restrict__ mask,
                                                         int32_t* __restrict__ kept) {
  F2N_RAISE_PRIO();
  const int c = threadIdx.x & 15;
  const int ray = blockIdx.x * F2N_ROW_RAYS_PER_BLOCK + (threadIdx.x >> 4);
  if (ray >= n_rays) return;
  const int s = se[2 * ray], e = se[2 * ray + 1];
  float acc = 0.f;
  int cnt = 0;
  float n_f0 = 0.f, n_dt = 0.f;
  if (s < e) {
    const int i = min(s + c, e - 1);
    n_f0 = f0[(size_t) i * f0_stride];
    n_dt = dt[i];
  }
  for (int base = s; base < e; base += 16) {
    const int i = base + c;
    const bool in = i < e;
    const float c_f0 = n_f0, c_dt = n_dt;
    if (base + 16 < e) {
      const int j = min(i + 16, e - 1);
      n_f0 = f0[(size_t) j * f0_stride];
      n_dt = dt[j];
    }
    float sec = 0.f;
    if (in) sec = expf(c_f0 - F2N_DENSITY_SHIFT) * c_dt;
    const float alpha = 1.f - expf(-sec);
    float excl;
    f2n_row_chain1x(sec, acc, excl);
    const float trans = expf(-excl);  // exclusive cumulative density
    const int m = (in && trans > F2N_T_EPS) ? 1 : 0;
    if (in) {
      weights[i] = trans * alpha;
      alphas[i] = alpha;
      mask[i] = m;
    }
    cnt += m;
  }
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 16);
  if (c == 0) kept[ray] = cnt;
}

// Renderer.cpp:128-135: order-preserving compaction of masked samples; one wave per ray.  The mask of a ray is
// (numerically) a prefix, but nothing here relies on it: positions come from a wave-level ballot prefix count.
__global__ __launch_bounds__(256) void compact_kernel(int n_rays, const int32_t* __restrict__ old_se,
                                                      const int32_t* __restrict__ new_se, const int32_t* __restrict__ mask,
                                                      const float* __restrict__ pts, const float* __restrict__ dirs,
                                                      const float* __restrict__ dt, const float* __restrict__ t,
                                                      const int32_t* __restrict__ anchors, float* __restrict__ o_pts,
                                                      float* __restrict__ o_dirs, float* __restrict__ o_dt, float* __restrict__ o_t,
                                                      int32_t* __restrict__ o_anchors, int32_t* __restrict__ o_src,
                                                      int32_t* __restrict__ o_vol, const int32_t* __restrict__ ray_val,
                                                      int32_t* __restrict__ o_ray_val) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (ray >= n_rays) return;
  const int s = old_se[2 * ray], e = old_se[2 * ray + 1];
  int dst = new_se[2 * ray];
  const int rv = o_ray_val != nullptr ? ray_val[ray] : 0;  // ScatterIdx (Scatter.cu:110-120) of the survivors, for free
  for (int base = s; base < e; base += 64) {
    const int i = base + lane;
    const bool keep = i < e && mask[i] != 0;
    const unsigned long long bal = __ballot(keep);
    if (keep) {
      const int k = dst + __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
      for (int c = 0; c < 3; c++) {
        o_pts[3 * (size_t) k + c] = pts[3 * (size_t) i + c];
        o_dirs[3 * (size_t) k + c] = dirs[3 * (size_t) i + c];
      }
      if (o_anchors != nullptr) {  // (a streaming training step reads only o_vol of the survivors' anchors)
#pragma unroll
        for (int c = 0; c < 3; c++) o_anchors[3 * (size_t) k + c] = anchors[3 * (size_t) i + c];
      }
      o_dt[k] = dt[i];
      o_t[k] = t[i];
      if (o_src != nullptr) o_src[k] = i;
      if (o_vol != nullptr) o_vol[k] = anchors[3 * (size_t) i];  // trans idx as a unit-stride array (the field's volume index)
      if (o_ray_val != nullptr) o_ray_val[k] = rv;
    }
    dst += __popcll(bal);
  }
}

// Renderer.cpp:190-208 forward.
// CustomOps.cu:12-66.  mean = (sum w_i * i/16) / (1e-6 + sum w_i), both sums left to right.
__device__ __forceinline__ void f2n_wv_stats(const float* __restrict__ w, int n, int c, float& mean, float& wsum) {
  float m = 0.f, ws = 1e-6f;
  for (int base = 0; base < n; base += 16) {
    const int i = base + c;
    const float wi = i < n ? w[i] : 0.f;
    m = f2n_row_last(f2n_row_seq_scan(wi * ((float) i / 16.f), m, c));
    ws = f2n_row_last(f2n_row_seq_scan(wi, ws, c));
  }
  mean = m / ws;
  wsum = ws;
}

__global__ __launch_bounds__(256) void composite_fwd_kernel(int n_rays, const int32_t* __restrict__ se, const float* __restrict__ f0,
                                                            int f0_stride, const float* __restrict__ dt, const float* __restrict__ t,
                                                            const float* __restrict__ rgb, const float* __restrict__ bg,
                                                            float* __restrict__ colors, float* __restrict__ disparity,
                                                            float* __restrict__ depth, float* __restrict__ weights,
                                                            float* __restrict__ out_vars) {
  F2N_RAISE_PRIO();
  const int c = threadIdx.x & 15;
  const int ray = blockIdx.x * F2N_ROW_RAYS_PER_BLOCK + (threadIdx.x >> 4);
  if (ray >= n_rays) return;
  const int s = se[2 * ray], e = se[2 * ray + 1];
  float acc = 0.f, col[3] = {0.f, 0.f, 0.f}, disp = 0.f, dep = 0.f;
  // WeightVarLoss forward statistics (f2n_wv_stats) ride along in the same walk: same terms, same order
  const bool with_var = out_vars != nullptr;
  float wv_m = 0.f, wv_ws = 1e-6f;
  struct In {
    float f0, dt, t, c0, c1, c2;
  };
  auto fetch = [&](int i) {
    In r;
    r.f0 = f0[(size_t) i * f0_stride];
    r.dt = dt[i];
    r.t = t[i];
    r.c0 = rgb[3 * (size_t) i];
    r.c1 = rgb[3 * (size_t) i + 1];
    r.c2 = rgb[3 * (size_t) i + 2];
    return r;
  };
  In nxt = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (s < e) nxt = fetch(min(s + c, e - 1));
  for (int base = s; base < e; base += 16) {
    const int i = base + c;
    const bool in = i < e;
    const In cur = nxt;
    if (base + 16 < e) nxt = fetch(min(i + 16, e - 1));
    float sec = 0.f, tt = 1.f, cr[3] = {0.f, 0.f, 0.f};
    if (in) {
      sec = expf(cur.f0 - F2N_DENSITY_SHIFT) * cur.dt;
      tt = cur.t + F2N_T_BIAS;
      cr[0] = cur.c0; cr[1] = cur.c1; cr[2] = cur.c2;
    }
    const float alpha = 1.f - expf(-sec);
    const float incl = f2n_row_seq_scan(sec, acc, c);
    const float trans = expf(-f2n_row_exclusive(incl, acc, c));
    acc = f2n_row_last(incl);
    const float w = in ? trans * alpha : 0.f;  // lanes past the end add exact zeros to the running sums
    if (in) weights[i] = w;
#pragma unroll
    for (int k = 0; k < 3; k++) col[k] = f2n_row_last(f2n_row_seq_scan(w * cr[k], col[k], c));
    disp = f2n_row_last(f2n_row_seq_scan(w / tt, disp, c));
    dep = f2n_row_last(f2n_row_seq_scan(w * tt, dep, c));
    if (with_var) {
      wv_m = f2n_row_last(f2n_row_seq_scan(w * ((float) (i - s) / 16.f), wv_m, c));
      wv_ws = f2n_row_last(f2n_row_seq_scan(w, wv_ws, c));
    }
  }
  if (c == 0) {
    const float last_trans = expf(-acc);
#pragma unroll
    for (int k = 0; k < 3; k++) colors[3 * ray + k] = col[k] + last_trans * bg[3 * ray + k];
    disparity[ray] = disp;
    depth[ray] = dep / (1.f - last_trans + 1e-4f);
  }
  if (with_var) {  // WeightVarLoss forward (weight_var_fwd_kernel): second walk over the weights this row has just written
    float var = 0.f;
    if (s < e) {
      const float mean = wv_m / wv_ws;
      float n_w = weights[min(s + c, e - 1)];
      for (int base = 0; base + s < e; base += 16) {
        const int i = base + c;
        const float c_w = n_w;
        if (base + 16 + s < e) n_w = weights[min(i + 16 + s, e - 1)];
        const float b = (float) i / 16.f - mean;
        const float wi = i + s < e ? c_w : 0.f;
        var = f2n_row_last(f2n_row_seq_scan(wi * b * b, var, c));
      }
    }
    if (c == 0) out_vars[ray] = var;
  }
}

// Backward of the compositing chain (FlexOps backward kernels FlexOps.cu:17-26,42-53,75-93; TruncExp backward
// CustomOps.cpp:15-18; GradientScaling backward CustomOps.cu:68-80) in two walks per ray: a forward walk to
// rebuild T_i / w_i and the ray totals, and a reverse walk carrying the suffix sum of d(acc).  In the reverse walk
// lane c of a row takes sample hi-1-c, so the left-to-right row chain runs over descending sample indices.
__global__ __launch_bounds__(256) void composite_bwd_kernel(int n_rays, const int32_t* __restrict__ se, const float* __restrict__ f0,
                                                            int f0_stride, const float* __restrict__ dt, const float* __restrict__ t,
                                                            const float* __restrict__ rgb, const float* __restrict__ bg,
                                                            const float* __restrict__ dcolors, const float* __restrict__ ddisparity,
                                                            const float* __restrict__ ddepth, const float* __restrict__ dweights,
                                                            float gs_progress, float* __restrict__ drgb, float* __restrict__ df0, int df0_stride,
                                                            const float* __restrict__ var_weights, const float* __restrict__ dvars) {
  F2N_RAISE_PRIO();
  const int c = threadIdx.x & 15;
  const int ray = blockIdx.x * F2N_ROW_RAYS_PER_BLOCK + (threadIdx.x >> 4);
  if (ray >= n_rays) return;
  const int s = se[2 * ray], e = se[2 * ray + 1];
  if (s >= e) return;
  float dC[3] = {0.f, 0.f, 0.f};
  if (dcolors != nullptr) { dC[0] = dcolors[3 * ray]; dC[1] = dcolors[3 * ray + 1]; dC[2] = dcolors[3 * ray + 2]; }
  const float dDisp = ddisparity != nullptr ? ddisparity[ray] : 0.f;
  const float dDep = ddepth != nullptr ? ddepth[ray] : 0.f;
  const bool with_var = var_weights != nullptr && dvars != nullptr;
  // walk 1: totals (cumulative density, depth numerator) and, in the same walk, the WeightVarLoss statistics (f2n_wv_stats)
  float acc = 0.f, dep_sum = 0.f, wv_m = 0.f, wv_ws = 1e-6f;
  {
    struct In {
      float f0, dt, t, vw;
    };
    auto fetch = [&](int i) {
      In r;
      r.f0 = f0[(size_t) i * f0_stride];
      r.dt = dt[i];
      r.t = t[i];
      r.vw = with_var ? var_weights[i] : 0.f;
      return r;
    };
    In nxt = fetch(min(s + c, e - 1));
    for (int base = s; base < e; base += 16) {
      const int i = base + c;
      const bool in = i < e;
      const In cur = nxt;
      if (base + 16 < e) nxt = fetch(min(i + 16, e - 1));
      float sec = 0.f, tt = 1.f;
      if (in) {
        sec = expf(cur.f0 - F2N_DENSITY_SHIFT) * cur.dt;
        tt = cur.t + F2N_T_BIAS;
      }
      const float incl = f2n_row_seq_scan(sec, acc, c);
      const float w = in ? expf(-f2n_row_exclusive(incl, acc, c)) * (1.f - expf(-sec)) : 0.f;
      acc = f2n_row_last(incl);
      dep_sum = f2n_row_last(f2n_row_seq_scan(w * tt, dep_sum, c));
      if (with_var) {
        const float wi = in ? cur.vw : 0.f;
        wv_m = f2n_row_last(f2n_row_seq_scan(wi * ((float) (i - s) / 16.f), wv_m, c));
        wv_ws = f2n_row_last(f2n_row_seq_scan(wi, wv_ws, c));
      }
    }
  }
  const float total = acc;
  const float last_trans = expf(-total);
  const float denom = 1.f - last_trans + 1e-4f;
  // d(last_trans): colors = .. + last_trans*bg ; depth = dep_sum / (1 - last_trans + 1e-4)
  const float d_last = (dC[0] * bg[3 * ray] + dC[1] * bg[3 * ray + 1] + dC[2] * bg[3 * ray + 2]) +
                       dDep * dep_sum / (denom * denom);
  const float d_total = -last_trans * d_last;  // last_trans = exp(-sum sec): every sec_i receives this
  const float dDepW = dDep / denom;
  // WeightVarLoss backward (weight_var_bwd_kernel) folded in: d var / d w_i = dv * (b_i^2 - tmp * (i/16) / ws)
  float wv_mean = 0.f, wv_tmp = 0.f, wv_dv = 0.f;
  if (with_var) {
    wv_mean = wv_m / wv_ws;
    float n_w = var_weights[min(s + c, e - 1)];
    for (int base = 0; base + s < e; base += 16) {
      const int i = base + c;
      const float c_w = n_w;
      if (base + 16 + s < e) n_w = var_weights[min(i + 16 + s, e - 1)];
      const float b = (float) i / 16.f - wv_mean;
      const float wi = i + s < e ? c_w : 0.f;
      wv_tmp = f2n_row_last(f2n_row_seq_scan(wi * 2.f * b, wv_tmp, c));
    }
    wv_dv = dvars[ray];
  }
  // walk 2: reverse, suffix carries sum_{j>i} d(acc_j)
  struct RIn {
    float f0, dt, t, c0, c1, c2, dw;
  };
  auto rfetch = [&](int i) {
    RIn r;
    r.f0 = f0[(size_t) i * f0_stride];
    r.dt = dt[i];
    r.t = t[i];
    r.c0 = rgb[3 * (size_t) i];
    r.c1 = rgb[3 * (size_t) i + 1];
    r.c2 = rgb[3 * (size_t) i + 2];
    r.dw = dweights != nullptr ? dweights[i] : 0.f;
    return r;
  };
  float suffix = 0.f;
  RIn rn = rfetch(max(e - 1 - c, s));
  for (int hi = e; hi > s; hi -= 16) {
    const int i = hi - 1 - c;
    const bool in = i >= s;
    const RIn rc = rn;
    if (hi - 16 > s) rn = rfetch(max(i - 16, s));
    float x = 0.f, dti = 0.f, sigma = 0.f, tt = 1.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, dwi = 0.f;
    if (in) {
      x = rc.f0 - F2N_DENSITY_SHIFT;
      sigma = expf(x);
      dti = rc.dt;
      tt = rc.t + F2N_T_BIAS;
      c0 = rc.c0; c1 = rc.c1; c2 = rc.c2;
      dwi = rc.dw;
    }
    const float sec = in ? sigma * dti : 0.f;
    // acc -= sec, rebuilt backwards: the exclusive cumulative density of sample i
    const float acc_i = f2n_row_seq_scan(-sec, acc, c);
    acc = f2n_row_last(acc_i);
    const float trans = expf(-acc_i);
    const float ems = expf(-sec);
    const float alpha = 1.f - ems;
    const float w = trans * alpha;
    float dw = (dC[0] * c0 + dC[1] * c1 + dC[2] * c2) + dDisp / tt + dDepW * tt;
    if (dweights != nullptr) dw += dwi;
    if (with_var && in) {
      const float r = (float) (i - s) / 16.f, b = r - wv_mean;
      dw += wv_dv * (b * b + wv_tmp * -r / wv_ws);
    }
    // w = trans*alpha ; trans = exp(-acc_excl) ; alpha = 1 - exp(-sec)
    const float d_acc = in ? -dw * w : 0.f;
    const float suf_incl = f2n_row_seq_scan(d_acc, suffix, c);
    const float suf_i = f2n_row_exclusive(suf_incl, suffix, c);
    suffix = f2n_row_last(suf_incl);
    if (in) {
      const float d_sec = dw * trans * ems + suf_i + d_total;
      float d_sigma = d_sec * dti;
      float g0 = dC[0] * w, g1 = dC[1] * w, g2 = dC[2] * w;
      if (gs_progress < 1.f) {  // CustomOps.cu:68-80
        const float a = ((float) (i - s) + .5f) / (float) (e - s);
        const float sc = gs_progress + (1.f - gs_progress) * a * a;
        d_sigma *= sc;
        g0 *= sc; g1 *= sc; g2 *= sc;
      }
      drgb[3 * (size_t) i] = g0;
      drgb[3 * (size_t) i + 1] = g1;
      drgb[3 * (size_t) i + 2] = g2;
      // TruncExp backward: grad * exp(clamp(x, -100, 5))
      df0[(size_t) i * df0_stride] = d_sigma * expf(fminf(fmaxf(x, -100.f), 5.f));
    }
  }
}


// ---------------------------------------------------------------------------------------------------
// Compositing forward + the loss of ExpRunner::Train + compositing backward in ONE launch (round 4; the streaming training
// step).  Renderer.cpp:196-208 / FlexOps.cu:55-93 forward, ExpRunner.cpp:95-120, then the backward chain of composite_bwd_kernel.
// Everything between a ray's colour and the gradient of its samples is per ray: d loss / d colour = (pred - gt) / sqrt(.) / 3R,
// d / d disparity, d / d weight-variance are element-wise functions of that ray's own outputs (the means' denominators are
// known on the host), so the row that has just walked a ray forward turns around and walks it backward -- with the totals the
// backward's first walk used to rebuild (cumulative density, depth numerator, WeightVar statistics) still in its registers.
// Replaces composite_fwd -> train_loss (+ its finalisation) -> composite_bwd: three dependent launches of the step's main
// queue and one re-walk of every ray.  Arithmetic and order of every sum are those of the three kernels: colours, weights,
// drgb, df0 are bit-identical (tests/test_gpu_parity.py::test_composite_train_equals_three_launches).
// The loss VALUES (reported only) leave as per-block partial sums of pre-scaled terms, folded by the step's deferred
// reduction (f2n_reduce_deferred) in a fixed order: out_losses = {loss, colour, var, disparity, tv, mse, 0, 0}.
// Blocks behind the ray blocks (tv_blocks of them) take the TV term over the edge features (ExpRunner.cpp:101) and its gradient.
// ---------------------------------------------------------------------------------------------------
// COLORS_IN (debug variant only, tools/n1_bound.py): the rays' sums of w * c arrive precomputed -- as they would from an order-free
// sum in the colour network's epilogue (north star / judge row N1) -- and the forward walk neither loads the samples' colours nor
// carries their three scan chains: what that walk can save AT MOST, measured instead of argued (profiles/r05_n1_bound.txt).
#define F2N_CT_TERMS 8
template <bool COLORS_IN>
__global__ __launch_bounds__(256) void composite_train_kernel(
    int n_rays, const int32_t* __restrict__ se, const float* __restrict__ f0, int f0_stride, const float* __restrict__ dt,
    const float* __restrict__ t, const float* __restrict__ rgb, const float* __restrict__ bg, const float* __restrict__ gt,
    float var_w, float disp_w, float tv_w, float gs_progress, int n_edge, int feat_dim, const float* __restrict__ edge,
    float* __restrict__ dedge, float* __restrict__ colors, float* __restrict__ weights, float* __restrict__ drgb,
    float* __restrict__ df0, int df0_stride, float* __restrict__ partials, float* __restrict__ out_losses, int ray_blocks,
    const float* __restrict__ colors_in) {
  F2N_RAISE_PRIO();
  __shared__ float s_terms[F2N_ROW_RAYS_PER_BLOCK][4];
  __shared__ float s_tv[256];
  if (blockIdx.x == 0 && threadIdx.x < F2N_CT_TERMS) out_losses[threadIdx.x] = 0.f;  // (the deferred reduction ADDS the partial sums)
  if ((int) blockIdx.x >= ray_blocks) {
    // ---- TV term: mean (edge_feat[:,0,:] - edge_feat[:,1,:])^2 and its gradient, element-wise ----
    const int n_tv = n_edge * feat_dim;
    const float inv_tv = 1.f / (float) max(n_tv, 1);
    const int tvb = gridDim.x - ray_blocks;
    float acc = 0.f;
    for (int i = (blockIdx.x - ray_blocks) * 256 + threadIdx.x; i < n_tv; i += tvb * 256) {
      const int e = i / feat_dim, f = i - e * feat_dim;
      const size_t i0 = ((size_t) 2 * e) * feat_dim + f, i1 = i0 + feat_dim;
      const float d = edge[i0] - edge[i1];
      acc += d * d;
      if (dedge != nullptr) {
        const float g = tv_w * 2.f * d * inv_tv;
        dedge[i0] = g;
        dedge[i1] = -g;
      }
    }
    s_tv[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
      if ((int) threadIdx.x < off) s_tv[threadIdx.x] += s_tv[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x < F2N_CT_TERMS) {
      const float tv = s_tv[0] * inv_tv;
      partials[(size_t) blockIdx.x * F2N_CT_TERMS + threadIdx.x] = threadIdx.x == 0 ? tv * tv_w : threadIdx.x == 4 ? tv : 0.f;
    }
    return;
  }
  const int c = threadIdx.x & 15, row = threadIdx.x >> 4;
  const int ray = blockIdx.x * F2N_ROW_RAYS_PER_BLOCK + row;
  const bool live = ray < n_rays;
  int s = 0, e = 0;
  if (live) {
    s = se[2 * ray];
    e = se[2 * ray + 1];
  }
  // ================= forward walk (composite_fwd_kernel, with the WeightVar statistics riding along) =================
  // (the eight running sums are chains that keep their state in the row from chunk to chunk: rows_dev.h)
  float acc = 0.f, col[3] = {0.f, 0.f, 0.f}, disp = 0.f, dep = 0.f, wv_m = 0.f, wv_ws = 1e-6f;
  {
    struct In {
      float f0, dt, t, c0, c1, c2;
    };
    auto fetch = [&](int i) {
      In r;
      r.f0 = f0[(size_t) i * f0_stride];
      r.dt = dt[i];
      r.t = t[i];
      if (!COLORS_IN) {
        r.c0 = rgb[3 * (size_t) i];
        r.c1 = rgb[3 * (size_t) i + 1];
        r.c2 = rgb[3 * (size_t) i + 2];
      } else {
        r.c0 = r.c1 = r.c2 = 0.f;
      }
      return r;
    };
    In nxt = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (s < e) nxt = fetch(min(s + c, e - 1));
    for (int base = s; base < e; base += 16) {
      const int i = base + c;
      const bool in = i < e;
      const In cur = nxt;
      if (base + 16 < e) nxt = fetch(min(i + 16, e - 1));
      float sec = 0.f, tt = 1.f, cr[3] = {0.f, 0.f, 0.f};
      if (in) {
        sec = expf(cur.f0 - F2N_DENSITY_SHIFT) * cur.dt;
        tt = cur.t + F2N_T_BIAS;
        cr[0] = cur.c0; cr[1] = cur.c1; cr[2] = cur.c2;
      }
      const float alpha = 1.f - expf(-sec);
      float excl;
      f2n_row_chain1x(sec, acc, excl);
      const float trans = expf(-excl);
      const float w = in ? trans * alpha : 0.f;
      if (in) weights[i] = w;
      const float x_disp = w / tt, x_dep = w * tt, x_m = w * ((float) (i - s) / 16.f);
      if (!COLORS_IN) {
        f2n_row_chain4(w * cr[0], w * cr[1], w * cr[2], x_disp, col[0], col[1], col[2], disp);
        f2n_row_chain3(x_dep, x_m, w, dep, wv_m, wv_ws);
      } else {
        f2n_row_chain4(x_disp, x_dep, x_m, w, disp, dep, wv_m, wv_ws);
      }
    }
    acc = f2n_row_last(acc);
#pragma unroll
    for (int k = 0; k < 3; k++) col[k] = f2n_row_last(col[k]);
    disp = f2n_row_last(disp);
    dep = f2n_row_last(dep);
    wv_m = f2n_row_last(wv_m);
    wv_ws = f2n_row_last(wv_ws);
  }
  if (COLORS_IN && live) {
#pragma unroll
    for (int k = 0; k < 3; k++) col[k] = colors_in[3 * ray + k];
  }
  const float total = acc;
  const float last_trans = expf(-total);
  float bgc[3] = {0.f, 0.f, 0.f}, gtc[3] = {0.f, 0.f, 0.f};
  if (live) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      bgc[k] = bg[3 * ray + k];
      gtc[k] = gt[3 * ray + k];
    }
  }
  float pred[3];
#pragma unroll
  for (int k = 0; k < 3; k++) pred[k] = col[k] + last_trans * bgc[k];
  if (live && c < 3) colors[3 * ray + c] = c == 0 ? pred[0] : c == 1 ? pred[1] : pred[2];
  // WeightVarLoss forward (weight_var_fwd_kernel) and the first half of its backward (wv_tmp of weight_var_bwd_kernel): one more
  // walk over the weights this row has just written
  float var = 0.f, wv_tmp = 0.f;
  const float wv_mean = wv_m / wv_ws;
  if (s < e) {
    float n_w = weights[min(s + c, e - 1)];
    for (int base = 0; base + s < e; base += 16) {
      const int i = base + c;
      const float c_w = n_w;
      if (base + 16 + s < e) n_w = weights[min(i + 16 + s, e - 1)];
      const float b = (float) i / 16.f - wv_mean;
      const float wi = i + s < e ? c_w : 0.f;
      f2n_row_chain2(wi * b * b, wi * 2.f * b, var, wv_tmp);
    }
    var = f2n_row_last(var);
    wv_tmp = f2n_row_last(wv_tmp);
  }
  // ================= the loss of this ray and its gradients (train_loss_kernel, element-wise per ray) =================
  const float inv_col = 1.f / (float) max(3 * n_rays, 1), inv_ray = 1.f / (float) max(n_rays, 1);
  float dC[3], t_col = 0.f, t_mse = 0.f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float d = pred[k] - gtc[k];
    const float r = sqrtf(d * d + 1e-4f);
    t_col += r;
    t_mse += d * d;
    dC[k] = d / r * inv_col;
  }
  const float r_var = sqrtf(var + 1e-2f);
  const float wv_dv = var_w * .5f / r_var * inv_ray;
  const float dDisp = disp_w * 2.f * disp * inv_ray;
  if (c == 0) {
    s_terms[row][0] = live ? t_col * inv_col : 0.f;
    s_terms[row][1] = live ? r_var * inv_ray : 0.f;
    s_terms[row][2] = live ? disp * disp * inv_ray : 0.f;
    s_terms[row][3] = live ? t_mse * inv_col : 0.f;
  }
  __syncthreads();
  if (threadIdx.x < F2N_CT_TERMS) {  // this block's partial sums, rows in a fixed order
    float sc = 0.f, sv = 0.f, sd = 0.f, sm = 0.f;
    for (int r = 0; r < F2N_ROW_RAYS_PER_BLOCK; r++) {
      sc += s_terms[r][0];
      sv += s_terms[r][1];
      sd += s_terms[r][2];
      sm += s_terms[r][3];
    }
    const int k = threadIdx.x;
    partials[(size_t) blockIdx.x * F2N_CT_TERMS + k] =
        k == 0 ? sc + sv * var_w + sd * disp_w : k == 1 ? sc : k == 2 ? sv : k == 3 ? sd : k == 5 ? sm : 0.f;
  }
  if (s >= e) return;
  // ================= backward walk (composite_bwd_kernel's second walk; its first walk's totals are in registers) =================
  const float dep_sum = dep;
  const float denom = 1.f - last_trans + 1e-4f;
  const float dDep = 0.f;  // (the depth output carries no loss term)
  const float d_last = (dC[0] * bgc[0] + dC[1] * bgc[1] + dC[2] * bgc[2]) + dDep * dep_sum / (denom * denom);
  const float d_total = -last_trans * d_last;
  const float dDepW = dDep / denom;
  struct RIn {
    float f0, dt, t, c0, c1, c2;
  };
  auto rfetch = [&](int i) {
    RIn r;
    r.f0 = f0[(size_t) i * f0_stride];
    r.dt = dt[i];
    r.t = t[i];
    r.c0 = rgb[3 * (size_t) i];
    r.c1 = rgb[3 * (size_t) i + 1];
    r.c2 = rgb[3 * (size_t) i + 2];
    return r;
  };
  float suffix = 0.f;
  RIn rn = rfetch(max(e - 1 - c, s));
  for (int hi = e; hi > s; hi -= 16) {
    const int i = hi - 1 - c;
    const bool in = i >= s;
    const RIn rc = rn;
    if (hi - 16 > s) rn = rfetch(max(i - 16, s));
    float x = 0.f, dti = 0.f, sigma = 0.f, tt = 1.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (in) {
      x = rc.f0 - F2N_DENSITY_SHIFT;
      sigma = expf(x);
      dti = rc.dt;
      tt = rc.t + F2N_T_BIAS;
      c0 = rc.c0; c1 = rc.c1; c2 = rc.c2;
    }
    const float sec = in ? sigma * dti : 0.f;
    f2n_row_chain1(-sec, acc);
    const float acc_i = acc;
    const float trans = expf(-acc_i);
    const float ems = expf(-sec);
    const float alpha = 1.f - ems;
    const float w = trans * alpha;
    float dw = (dC[0] * c0 + dC[1] * c1 + dC[2] * c2) + dDisp / tt + dDepW * tt;
    if (in) {
      const float r = (float) (i - s) / 16.f, b = r - wv_mean;
      dw += wv_dv * (b * b + wv_tmp * -r / wv_ws);
    }
    const float d_acc = in ? -dw * w : 0.f;
    float suf_i;
    f2n_row_chain1x(d_acc, suffix, suf_i);
    if (in) {
      const float d_sec = dw * trans * ems + suf_i + d_total;
      float d_sigma = d_sec * dti;
      float g0 = dC[0] * w, g1 = dC[1] * w, g2 = dC[2] * w;
      if (gs_progress < 1.f) {  // CustomOps.cu:68-80
        const float a = ((float) (i - s) + .5f) / (float) (e - s);
        const float sc = gs_progress + (1.f - gs_progress) * a * a;
        d_sigma *= sc;
        g0 *= sc; g1 *= sc; g2 *= sc;
      }
      drgb[3 * (size_t) i] = g0;
      drgb[3 * (size_t) i + 1] = g1;
      drgb[3 * (size_t) i + 2] = g2;
      df0[(size_t) i * df0_stride] = d_sigma * expf(fminf(fmaxf(x, -100.f), 5.f));
    }
  }
}

__global__ __launch_bounds__(256) void weight_var_fwd_kernel(int n_rays, const float* __restrict__ weights,
                                                             const int32_t* __restrict__ se, float* __restrict__ out) {
  const int c = threadIdx.x & 15;
  const int ray = blockIdx.x * F2N_ROW_RAYS_PER_BLOCK + (threadIdx.x >> 4);
  if (ray >= n_rays) return;
  const int s = se[2 * ray], e = se[2 * ray + 1];
  if (s >= e) {
    if (c == 0) out[ray] = 0.f;
    return;
  }
  float mean, ws;
  f2n_wv_stats(weights + s, e - s, c, mean, ws);
  float var = 0.f;
  for (int base = 0; base + s < e; base += 16) {
    const int i = base + c;
    const float b = (float) i / 16.f - mean;
    const float wi = i + s < e ? weights[i + s] : 0.f;
    var = f2n_row_last(f2n_row_seq_scan(wi * b * b, var, c));
  }
  if (c == 0) out[ray] = var;
}

__global__ __launch_bounds__(256) void weight_var_bwd_kernel(int n_rays, const float* __restrict__ weights,
                                                             const int32_t* __restrict__ se, const float* __restrict__ dvars,
                                                             float* __restrict__ dw) {
  const int c = threadIdx.x & 15;
  const int ray = blockIdx.x * F2N_ROW_RAYS_PER_BLOCK + (threadIdx.x >> 4);
  if (ray >= n_rays) return;
  const int s = se[2 * ray], e = se[2 * ray + 1];
  if (s >= e) return;
  float mean, ws;
  f2n_wv_stats(weights + s, e - s, c, mean, ws);
  float tmp = 0.f;
  for (int base = 0; base + s < e; base += 16) {
    const int i = base + c;
    const float b = (float) i / 16.f - mean;
    const float wi = i + s < e ? weights[i + s] : 0.f;
    tmp = f2n_row_last(f2n_row_seq_scan(wi * 2.f * b, tmp, c));
  }
  const float dv = dvars[ray];
  for (int i = c; i + s < e; i += 16) {
    const float b = (float) i / 16.f - mean;
    const float g = (b * b + tmp * -((float) i / 16.f) / ws);
    dw[i + s] = dv * g;
  }
}

// ---------------------------------------------------------------------------------------------------
// Distortion loss of mip-NeRF 360 (eq. 15) on the warped step length dt, the coordinate compositing integrates over (no reference
// counterpart; include/f2n_abi.h has the definition and every rounding).  Sample k is the interval of length dt_k behind the
// intervals of the ray's earlier survivors, m_k its midpoint: dist = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 dt_i, in O(n)
// from four running sums of non-negative terms -- no cumulative coordinate, no subtraction, nothing cancels:
//   forward   P_k = sum_{j<k} w_j      D_k = D_{k-1} + P_k h_k   = sum_{j<k} w_j (m_k - m_j)     h_k = (dt_{k-1} + dt_k) / 2
//   reverse   S_k = sum_{j>k} w_j      U_k = U_{k+1} + S_k h_{k+1} = sum_{j>k} w_j (m_j - m_k)
// The walks are those of composite_bwd_kernel: one row per ray, 16-sample chunks, the next chunk's loads in flight; P feeds D (and D
// the ray's sum), so the chains of a chunk depend on one another and run one behind the other.  The neighbour's dt comes from the
// neighbouring lane (lane 0: the previous chunk's last lane), not from a second load.
// ---------------------------------------------------------------------------------------------------
// the forward walk: lane c's D_k of every sample goes to d_out (if given), returns the ray's dist in every lane
template <bool STORE_D>
__device__ __forceinline__ float f2n_distortion_walk(int s, int e, int c, const float* __restrict__ weights, const float* __restrict__ dt,
                                                     float* d_out) {
  float P = 0.f, D = 0.f, dist = 0.f, dt_last = 0.f;
  float n_w = weights[min(s + c, e - 1)], n_dt = dt[min(s + c, e - 1)];
  for (int base = s; base < e; base += 16) {
    const int i = base + c;
    const bool in = i < e;
    const float w = in ? n_w : 0.f, dti = in ? n_dt : 0.f;
    if (base + 16 < e) {
      n_w = weights[min(i + 16, e - 1)];
      n_dt = dt[min(i + 16, e - 1)];
    }
    const float dt_prev = f2n_row_exclusive(dti, dt_last, c);
    dt_last = f2n_row_last(dti);
    const float h = (in && i > s) ? .5f * (dt_prev + dti) : 0.f;
    float Pk;
    f2n_row_chain1x(w, P, Pk);
    f2n_row_chain1(Pk * h, D);
    if (STORE_D && in) d_out[i] = D;
    const float l = in ? w * (2.f * D) + ((w * w) * dti) * (1.f / 3.f) : 0.f;
    f2n_row_chain1(l, dist);
  }
  return f2n_row_last(dist);
}

__global__ __launch_bounds__(256) void distortion_fwd_kernel(int n_rays, const int32_t* __restrict__ se, const float* __restrict__ weights,
                                                             const float* __restrict__ dt, float* __restrict__ dist) {
  const int c = threadIdx.x & 15;
  const int ray = blockIdx.x * F2N_ROW_RAYS_PER_BLOCK + (threadIdx.x >> 4);
  if (ray >= n_rays) return;
  const int s = se[2 * ray], e = se[2 * ray + 1];
  float d = 0.f;
  if (s < e) d = f2n_distortion_walk<false>(s, e, c, weights, dt, nullptr);
  if (c == 0) dist[ray] = d;
}

// D_k is made by lane (k - s) % 16 of the forward walk and needed by lane (e - 1 - k) % 16 of the reverse walk.  It travels through
// the output itself: the forward walk parks D_k in dweights[k], the reverse walk reads it back and overwrites it with g_k (the lane
// that reads a slot is the only one that writes it again).  dweights is therefore NOT __restrict__, and a workgroup-scope fence
// stands between the walks: the row's stores have to be visible to the other lanes of its wave before they load, and the compiler
// may move neither across it.  No LDS and no second [M] buffer.
__global__ __launch_bounds__(256) void distortion_bwd_kernel(int n_rays, const int32_t* __restrict__ se, const float* __restrict__ weights,
                                                             const float* __restrict__ dt, const float* __restrict__ ddist,
                                                             float* dweights, float* __restrict__ dist) {
  const int c = threadIdx.x & 15;
  const int ray = blockIdx.x * F2N_ROW_RAYS_PER_BLOCK + (threadIdx.x >> 4);
  if (ray >= n_rays) return;
  const int s = se[2 * ray], e = se[2 * ray + 1];
  if (s >= e) {
    if (dist != nullptr && c == 0) dist[ray] = 0.f;
    return;
  }
  const float total = f2n_distortion_walk<true>(s, e, c, weights, dt, dweights);
  if (dist != nullptr && c == 0) dist[ray] = total;
  const float dd = ddist[ray];
  __threadfence_block();
  // reverse walk: lane c takes sample hi-1-c, the row chains run over descending sample indices
  struct RIn {
    float w, dt, D;
  };
  auto rfetch = [&](int i) {
    RIn r;
    r.w = weights[i];
    r.dt = dt[i];
    r.D = dweights[i];
    return r;
  };
  float S = 0.f, U = 0.f, dt_last = 0.f;
  RIn rn = rfetch(max(e - 1 - c, s));
  for (int hi = e; hi > s; hi -= 16) {
    const int i = hi - 1 - c;
    const bool in = i >= s;
    const RIn rc = rn;
    if (hi - 16 > s) rn = rfetch(max(i - 16, s));
    const float w = in ? rc.w : 0.f, dti = in ? rc.dt : 0.f;
    const float dt_next = f2n_row_exclusive(dti, dt_last, c);
    dt_last = f2n_row_last(dti);
    const float h = (in && i < e - 1) ? .5f * (dti + dt_next) : 0.f;
    float Sk;
    f2n_row_chain1x(w, S, Sk);
    f2n_row_chain1(Sk * h, U);
    if (in) dweights[i] = dd * (2.f * (rc.D + U) + ((2.f / 3.f) * w) * dti);
  }
}

// losses[slot] = mean(x), losses[0] += weight * mean(x): one workgroup, fp64 accumulators, a fixed stride and a fixed tree, so the
// result is a function of the inputs alone.
__global__ __launch_bounds__(256) void loss_add_mean_kernel(int n, const float* __restrict__ x, float weight, float* __restrict__ losses,
                                                            int slot) {
  __shared__ double s_sum[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += (double) x[i];
  s_sum[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int) threadIdx.x < off) s_sum[threadIdx.x] += s_sum[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float mean = (float) (s_sum[0] / (double) n);
    losses[slot] = mean;
    losses[0] = losses[0] + weight * mean;
  }
}

// Geometry buffers of rendered rays (no reference counterpart): per sample the world-space direction of the density gradient,
// g = J^T df0/dw with J = f2n_warp_jac of the sample's leaf at x = o + t d (the point the march warped), and n = -g / |g| -- the
// expressions of density_grad_scatter_kernel (f2n_warp_jac_t_mul / f2n_unit3, f2n_dev.h), so the two agree bit for bit; per ray
// opacity = sum w, N = sum w n (normalised behind the walk) and the first sample whose inclusive running sum of w reaches tau.
// The walk of composite_fwd_kernel: 16 lanes take 16 consecutive samples, the four sums are row chains that add left to right, one
// term after the other, and the next chunk's loads are in flight while this chunk's Jacobians run.  A lane reads its leaf's
// transform (132 floats) through its own pointer: the lanes of a chunk mostly sit in one leaf, so the reads are same-address
// broadcasts out of L1 / L2.  Every lane remembers the first sample at which ITS inclusive sum reached tau; one row minimum
// behind the walk picks the ray's.  No atomics, no LDS: the outputs are a function of the inputs alone.
__global__ __launch_bounds__(256) void composite_geometry_kernel(
    int n_rays, const int32_t* __restrict__ se, const float* __restrict__ weights, const float* __restrict__ t,
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, const int32_t* __restrict__ anchors,
    const F2nTransInfo* __restrict__ transes, const float* __restrict__ df0_dw, float tau, float* __restrict__ opacity,
    float* __restrict__ normal, int32_t* __restrict__ surf_idx, float* __restrict__ surf_t, float* __restrict__ surf_point,
    float* __restrict__ surf_normal, float* __restrict__ sample_grad, float* __restrict__ sample_normal) {
  const int c = threadIdx.x & 15;
  const int ray = blockIdx.x * F2N_ROW_RAYS_PER_BLOCK + (threadIdx.x >> 4);
  if (ray >= n_rays) return;
  const int s = se[2 * ray], e = se[2 * ray + 1];
  const float o[3] = {rays_o[3 * ray], rays_o[3 * ray + 1], rays_o[3 * ray + 2]};
  const float d[3] = {rays_d[3 * ray], rays_d[3 * ray + 1], rays_d[3 * ray + 2]};
  const int kNone = 0x7fffffff;
  float op = 0.f, N[3] = {0.f, 0.f, 0.f};
  int first = kNone;  // the first sample of this lane's whose inclusive sum reached tau, and what is written for it
  float f_t = 0.f, f_x[3] = {0.f, 0.f, 0.f}, f_n[3] = {0.f, 0.f, 0.f};
  struct In {
    float w, t, g0, g1, g2;
    int a;
  };
  auto fetch = [&](int i) {
    In r;
    r.w = weights[i];
    r.t = t[i];
    r.a = anchors[3 * (size_t) i];
    r.g0 = df0_dw[3 * (size_t) i];
    r.g1 = df0_dw[3 * (size_t) i + 1];
    r.g2 = df0_dw[3 * (size_t) i + 2];
    return r;
  };
  In nxt = {0.f, 0.f, 0.f, 0.f, 0.f, 0};
  if (s < e) nxt = fetch(min(s + c, e - 1));
  for (int base = s; base < e; base += 16) {
    const int i = base + c;
    const bool in = i < e;
    const In cur = nxt;
    if (base + 16 < e) nxt = fetch(min(i + 16, e - 1));
    float w = 0.f, x[3] = {0.f, 0.f, 0.f}, nr[3] = {0.f, 0.f, 0.f};
    if (in) {
      w = cur.w;
#pragma unroll
      for (int k = 0; k < 3; k++) x[k] = o[k] + d[k] * cur.t;  // (sampler.hip: xyz = o + d * cur_t)
      float g[3] = {0.f, 0.f, 0.f};
      if (cur.a >= 0) {  // (a survivor always has a leaf; a negative index reads no transform and gives the zero normal)
        const float gw[3] = {cur.g0, cur.g1, cur.g2};
        f2n_warp_jac_t_mul(transes + cur.a, x, gw, g);
      }
      f2n_unit3<true>(g, nr);
      if (sample_grad != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; k++) sample_grad[3 * (size_t) i + k] = g[k];
      }
      if (sample_normal != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; k++) sample_normal[3 * (size_t) i + k] = nr[k];
      }
    }
    // lanes past the end add exact zeros to the running sums
    f2n_row_chain4(w, w * nr[0], w * nr[1], w * nr[2], op, N[0], N[1], N[2]);
    if (in && first == kNone && op >= tau) {
      first = i;
      f_t = cur.t;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        f_x[k] = x[k];
        f_n[k] = nr[k];
      }
    }
  }
  int hit = first;
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) hit = min(hit, __shfl_xor(hit, off, 16));
  op = f2n_row_last(op);
#pragma unroll
  for (int k = 0; k < 3; k++) N[k] = f2n_row_last(N[k]);
  if (c == 0) {
    float un[3];
    f2n_unit3<false>(N, un);
    opacity[ray] = op;
#pragma unroll
    for (int k = 0; k < 3; k++) normal[3 * ray + k] = un[k];
    if (hit == kNone) {
      surf_idx[ray] = -1;
      surf_t[ray] = 0.f;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        surf_point[3 * ray + k] = 0.f;
        surf_normal[3 * ray + k] = 0.f;
      }
    }
  }
  if (hit != kNone && first == hit) {  // (sample indices are distinct across the lanes: exactly one lane)
    surf_idx[ray] = hit;
    surf_t[ray] = f_t;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      surf_point[3 * ray + k] = f_x[k];
      surf_normal[3 * ray + k] = f_n[k];
    }
  }
}

// FlexOps.cu:5-93
__global__ void flex_sum_fwd_kernel(int n, int vec, const float* __restrict__ val, const int32_t* __restrict__ se,
                                    float* __restrict__ sum) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  for (int j = 0; j < vec; j++) {
    float s = 0.f;
    for (int i = se[2 * r]; i < se[2 * r + 1]; i++) s += val[(size_t) i * vec + j];
    sum[(size_t) r * vec + j] = s;
  }
}
__global__ void flex_sum_bwd_kernel(int n, int vec, const float* __restrict__ dsum, const int32_t* __restrict__ se,
                                    float* __restrict__ dval) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  for (int j = 0; j < vec; j++) {
    const float f = dsum[(size_t) r * vec + j];
    for (int i = se[2 * r]; i < se[2 * r + 1]; i++) dval[(size_t) i * vec + j] = f;
  }
}
__global__ void flex_acc_fwd_kernel(int n, int include_this, const float* __restrict__ val, const int32_t* __restrict__ se,
                                    float* __restrict__ sum) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  float s = 0.f;
  for (int i = se[2 * r]; i < se[2 * r + 1]; i++) {
    if (include_this) { s += val[i]; sum[i] = s; }
    else { sum[i] = s; s += val[i]; }
  }
}
__global__ void flex_acc_bwd_kernel(int n, int include_this, const float* __restrict__ dsum, const int32_t* __restrict__ se,
                                    float* __restrict__ dval) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  float wp = 0.f;
  for (int i = se[2 * r + 1] - 1; i >= se[2 * r]; i--) {
    if (include_this) { wp += dsum[i]; dval[i] = wp; }
    else { dval[i] = wp; wp += dsum[i]; }
  }
}

#define F2N_RAY_LAUNCH(kernel, n_rays, ...)                                                                          \
  do {                                                                                                               \
    if ((n_rays) < 0) return F2N_ERR_INVALID_ARG;                                                                    \
    if ((n_rays) == 0) return F2N_OK;                                                                                \
    hipLaunchKernelGGL(kernel, dim3(f2n_div_up((n_rays), 64)), dim3(64), 0, (hipStream_t) stream, (n_rays), __VA_ARGS__); \
    return f2n_launch_status();                                                                                      \
  } while (0)

#define F2N_ROW_LAUNCH(kernel, n_rays, ...)                                                                          \
  do {                                                                                                               \
    if ((n_rays) < 0) return F2N_ERR_INVALID_ARG;                                                                    \
    if ((n_rays) == 0) return F2N_OK;                                                                                \
    hipLaunchKernelGGL(kernel, dim3(f2n_div_up((n_rays), F2N_ROW_RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t) stream, \
                       (n_rays), __VA_ARGS__);                                                                       \
    return f2n_launch_status();                                                                                      \
  } while (0)

extern "C" {

int f2n_early_stop(void* stream, int n_rays, const int32_t* pts_start_end, const float* f0, int f0_stride, const float* dt,
                   float* weights, float* alphas, int32_t* mask, int32_t* kept) {
  if (f0_stride < 1) return F2N_ERR_INVALID_ARG;
  F2N_ROW_LAUNCH(early_stop_kernel, n_rays, pts_start_end, f0, f0_stride, dt, weights, alphas, mask, kept);
}

int f2n_compact_samples(void* stream, int n_rays, const int32_t* old_start_end, const int32_t* new_start_end,
                        const int32_t* mask, const float* pts, const float* dirs, const float* dt, const float* t,
                        const int32_t* anchors, float* o_pts, float* o_dirs, float* o_dt, float* o_t, int32_t* o_anchors) {
  if (n_rays < 0) return F2N_ERR_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  hipLaunchKernelGGL(compact_kernel, dim3(f2n_div_up(n_rays, 4)), dim3(256), 0, (hipStream_t) stream, n_rays, old_start_end,
                     new_start_end, mask, pts, dirs, dt, t, anchors, o_pts, o_dirs, o_dt, o_t, o_anchors, nullptr, nullptr, nullptr,
                     nullptr);
  return f2n_launch_status();
}

int f2n_compact_samples_src(void* stream, int n_rays, const int32_t* old_start_end, const int32_t* new_start_end,
                            const int32_t* mask, const float* pts, const float* dirs, const float* dt, const float* t,
                            const int32_t* anchors, float* o_pts, float* o_dirs, float* o_dt, float* o_t, int32_t* o_anchors,
                            int32_t* o_src, int32_t* o_vol, const int32_t* ray_val, int32_t* o_ray_val) {
  if (n_rays < 0 || o_src == nullptr || (o_ray_val != nullptr && ray_val == nullptr)) return F2N_ERR_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  hipLaunchKernelGGL(compact_kernel, dim3(f2n_div_up(n_rays, 4)), dim3(256), 0, (hipStream_t) stream, n_rays, old_start_end,
                     new_start_end, mask, pts, dirs, dt, t, anchors, o_pts, o_dirs, o_dt, o_t, o_anchors, o_src, o_vol, ray_val,
                     o_ray_val);
  return f2n_launch_status();
}

int f2n_composite_fwd(void* stream, int n_rays, const int32_t* pts_start_end, const float* f0, int f0_stride, const float* dt,
                      const float* t, const float* rgb, const float* bg, float* colors, float* disparity, float* depth,
                      float* weights, float* out_vars) {
  if (f0_stride < 1) return F2N_ERR_INVALID_ARG;
  F2N_ROW_LAUNCH(composite_fwd_kernel, n_rays, pts_start_end, f0, f0_stride, dt, t, rgb, bg, colors, disparity, depth, weights,
                 out_vars);
}

int f2n_composite_bwd(void* stream, int n_rays, const int32_t* pts_start_end, const float* f0, int f0_stride, const float* dt,
                      const float* t, const float* rgb, const float* bg, const float* dcolors, const float* ddisparity,
                      const float* ddepth, const float* dweights, float grad_scaling_progress, float* drgb, float* df0,
                      int df0_stride, const float* var_weights, const float* dvars) {
  if (f0_stride < 1 || df0_stride < 1 || ((var_weights == nullptr) != (dvars == nullptr))) return F2N_ERR_INVALID_ARG;
  F2N_ROW_LAUNCH(composite_bwd_kernel, n_rays, pts_start_end, f0, f0_stride, dt, t, rgb, bg, dcolors, ddisparity, ddepth, dweights,
                 grad_scaling_progress, drgb, df0, df0_stride, var_weights, dvars);
}

static int f2n_composite_train_impl(void* stream, int n_rays, const int32_t* pts_start_end, const float* f0, int f0_stride, const float* dt,
                        const float* t, const float* rgb, const float* bg, const float* gt_colors, float var_w, float disp_w, float tv_w,
                        float grad_scaling_progress, int n_edge, int feat_dim, const float* edge_feats, float* dedge_feats,
                        float* colors, float* weights, float* drgb, float* df0, int df0_stride, float* out_losses, int defer_reduce,
                        const float* colors_in) {
  if (n_rays < 1 || f0_stride < 1 || df0_stride < 1 || n_edge < 0 || (n_edge > 0 && (edge_feats == nullptr || feat_dim < 1)) ||
      out_losses == nullptr)
    return F2N_ERR_INVALID_ARG;
  const int ray_blocks = (int) f2n_div_up(n_rays, F2N_ROW_RAYS_PER_BLOCK);
  const int tv_blocks = n_edge > 0 ? (int) min((long) 32, (long) f2n_div_up((long) n_edge * feat_dim, 256)) : 0;
  const int blocks = ray_blocks + tv_blocks;
  float* partials = (float*) f2n_ws_get(F2N_WS_LOSS, sizeof(float) * ((size_t) blocks * F2N_CT_TERMS + 64 * 8 + 16));
  if (partials == nullptr) return F2N_ERR_INVALID_ARG;
  partials += 64 * 8 + 16;  // (the head of this slot belongs to f2n_train_loss: its partials and arrival counter)
#if F2N_DEBUG_BUILD
  if (colors_in != nullptr)
    hipLaunchKernelGGL(composite_train_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t) stream, n_rays, pts_start_end, f0, f0_stride, dt,
                       t, rgb, bg, gt_colors, var_w, disp_w, tv_w, grad_scaling_progress, n_edge, feat_dim, edge_feats, dedge_feats, colors,
                       weights, drgb, df0, df0_stride, partials, out_losses, ray_blocks, colors_in);
  else
#endif
  hipLaunchKernelGGL(composite_train_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t) stream, n_rays, pts_start_end, f0, f0_stride, dt,
                     t, rgb, bg, gt_colors, var_w, disp_w, tv_w, grad_scaling_progress, n_edge, feat_dim, edge_feats, dedge_feats, colors,
                     weights, drgb, df0, df0_stride, partials, out_losses, ray_blocks, colors_in);
  const int rc = f2n_launch_status();
  if (rc != F2N_OK) return rc;
  if (defer_reduce) return f2n_defer_reduction(F2N_CT_TERMS, blocks, partials, out_losses);
  return f2n_reduce_partials(stream, F2N_CT_TERMS, blocks, partials, out_losses);
}

int f2n_composite_train(void* stream, int n_rays, const int32_t* pts_start_end, const float* f0, int f0_stride, const float* dt,
                        const float* t, const float* rgb, const float* bg, const float* gt_colors, float var_w, float disp_w, float tv_w,
                        float grad_scaling_progress, int n_edge, int feat_dim, const float* edge_feats, float* dedge_feats,
                        float* colors, float* weights, float* drgb, float* df0, int df0_stride, float* out_losses, int defer_reduce) {
  return f2n_composite_train_impl(stream, n_rays, pts_start_end, f0, f0_stride, dt, t, rgb, bg, gt_colors, var_w, disp_w, tv_w,
                                  grad_scaling_progress, n_edge, feat_dim, edge_feats, dedge_feats, colors, weights, drgb, df0, df0_stride,
                                  out_losses, defer_reduce, nullptr);
}

#if F2N_DEBUG_BUILD
int f2n_debug_composite_train_colors_in(void* stream, int n_rays, const int32_t* pts_start_end, const float* f0, int f0_stride,
                                        const float* dt, const float* t, const float* rgb, const float* bg, const float* gt_colors,
                                        float var_w, float disp_w, float tv_w, float grad_scaling_progress, float* colors, float* weights,
                                        float* drgb, float* df0, float* out_losses, const float* colors_in) {
  return f2n_composite_train_impl(stream, n_rays, pts_start_end, f0, f0_stride, dt, t, rgb, bg, gt_colors, var_w, disp_w, tv_w,
                                  grad_scaling_progress, 0, 16, nullptr, nullptr, colors, weights, drgb, df0, 1, out_losses, 0, colors_in);
}
#endif

int f2n_weight_var_fwd(void* stream, int n_rays, const float* weights, const int32_t* pts_start_end, float* out_vars) {
  F2N_ROW_LAUNCH(weight_var_fwd_kernel, n_rays, weights, pts_start_end, out_vars);
}

int f2n_weight_var_bwd(void* stream, int n_rays, const float* weights, const int32_t* pts_start_end, const float* dvars,
                       float* dweights) {
  F2N_ROW_LAUNCH(weight_var_bwd_kernel, n_rays, weights, pts_start_end, dvars, dweights);
}

int f2n_distortion_fwd(void* stream, int n_rays, const int32_t* pts_start_end, const float* weights, const float* dt, float* dist) {
  if (n_rays > 0 && (pts_start_end == nullptr || weights == nullptr || dt == nullptr || dist == nullptr)) return F2N_ERR_INVALID_ARG;
  F2N_ROW_LAUNCH(distortion_fwd_kernel, n_rays, pts_start_end, weights, dt, dist);
}

int f2n_distortion_bwd(void* stream, int n_rays, const int32_t* pts_start_end, const float* weights, const float* dt, const float* ddist,
                       float* dweights, float* dist) {
  if (n_rays > 0 && (pts_start_end == nullptr || weights == nullptr || dt == nullptr || ddist == nullptr || dweights == nullptr ||
                     dweights == weights || dweights == dt))
    return F2N_ERR_INVALID_ARG;
  F2N_ROW_LAUNCH(distortion_bwd_kernel, n_rays, pts_start_end, weights, dt, ddist, dweights, dist);
}

int f2n_loss_add_mean(void* stream, int n, const float* x, float weight, float* losses, int slot) {
  if (n < 1 || x == nullptr || losses == nullptr || slot < 1 || slot > 7) return F2N_ERR_INVALID_ARG;
  hipLaunchKernelGGL(loss_add_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t) stream, n, x, weight, losses, slot);
  return f2n_launch_status();
}

int f2n_composite_geometry(void* stream, int n_rays, const int32_t* pts_start_end, const float* weights, const float* t, const float* rays_o,
                           const float* rays_d, const int32_t* anchors, const void* transes, const float* df0_dw, float tau,
                           float* out_opacity, float* out_normal, int32_t* out_surf_idx, float* out_surf_t, float* out_surf_point,
                           float* out_surf_normal, float* out_sample_grad, float* out_sample_normal) {
  if (!(tau > 0.f && tau <= 1.f)) return F2N_ERR_INVALID_ARG;  // (false for NaN as well)
  if (n_rays > 0 && (pts_start_end == nullptr || weights == nullptr || t == nullptr || rays_o == nullptr || rays_d == nullptr ||
                     anchors == nullptr || transes == nullptr || df0_dw == nullptr || out_opacity == nullptr || out_normal == nullptr ||
                     out_surf_idx == nullptr || out_surf_t == nullptr || out_surf_point == nullptr || out_surf_normal == nullptr))
    return F2N_ERR_INVALID_ARG;
  F2N_ROW_LAUNCH(composite_geometry_kernel, n_rays, pts_start_end, weights, t, rays_o, rays_d, anchors, (const F2nTransInfo*) transes, df0_dw,
                 tau, out_opacity, out_normal, out_surf_idx, out_surf_t, out_surf_point, out_surf_normal, out_sample_grad, out_sample_normal);
}

int f2n_flex_sum_fwd(void* stream, int n_rays, int vec, const float* val, const int32_t* start_end, float* sum) {
  if (vec < 1) return F2N_ERR_INVALID_ARG;
  F2N_RAY_LAUNCH(flex_sum_fwd_kernel, n_rays, vec, val, start_end, sum);
}
int f2n_flex_sum_bwd(void* stream, int n_rays, int vec, const float* dsum, const int32_t* start_end, float* dval) {
  if (vec < 1) return F2N_ERR_INVALID_ARG;
  F2N_RAY_LAUNCH(flex_sum_bwd_kernel, n_rays, vec, dsum, start_end, dval);
}
int f2n_flex_acc_fwd(void* stream, int n_rays, int include_this, const float* val, const int32_t* start_end, float* sum) {
  F2N_RAY_LAUNCH(flex_acc_fwd_kernel, n_rays, include_this, val, start_end, sum);
}
int f2n_flex_acc_bwd(void* stream, int n_rays, int include_this, const float* dsum, const int32_t* start_end, float* dval) {
  F2N_RAY_LAUNCH(flex_acc_bwd_kernel, n_rays, include_this, dsum, start_end, dval);
}

}  // extern "C"
