// Ray generation on gfx950: pixel -> world ray with the reference's Newton undistortion
// (Dataset/Dataset.cu:13-123), plus the pixel gather that turns resident images into a ground-truth colour batch.
// One ray per lane: ~150 flops and at most a few Newton iterations per ray; the point of having it on the device is
// residency -- the reference draws camera / pixel indices on the CPU and uploads rays and colours every iteration
// (Dataset.cpp:275-298), which sits directly in front of a 2 ms training step.
#include "f2n_dev.h"

__device__ __forceinline__ void f2n_distort(const float* k, float u, float v, float& du, float& dv) {  // :13-27
  const float k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3];
  const float u2 = u * u, uv = u * v, v2 = v * v;
  const float r2 = u2 + v2;
  const float radial = k1 * r2 + k2 * r2 * r2;
  du = u * radial + 2.f * p1 * uv + p2 * (r2 + 2.f * u2);
  dv = v * radial + 2.f * p2 * uv + p1 * (r2 + 2.f * v2);
}

// iterative_camera_undistortion, Dataset.cu:30-72: Newton with central differences; Eigen's 2x2 inverse spelled out
// (invdet = 1/det, det = m00*m11 - m10*m01) so that the oracle and this kernel agree bit for bit.
__device__ __forceinline__ void f2n_undistort(const float* k, float& u, float& v) {
  const float eps = 1.1920928955078125e-07f;
  const float x0[2] = {u, v};
  float x[2] = {u, v};
  for (int it = 0; it < 100; it++) {
    const float step0 = fmaxf(eps, fabsf(1e-6f * x[0]));
    const float step1 = fmaxf(eps, fabsf(1e-6f * x[1]));
    float dx[2], d0b[2], d0f[2], d1b[2], d1f[2];
    f2n_distort(k, x[0], x[1], dx[0], dx[1]);
    f2n_distort(k, x[0] - step0, x[1], d0b[0], d0b[1]);
    f2n_distort(k, x[0] + step0, x[1], d0f[0], d0f[1]);
    f2n_distort(k, x[0], x[1] - step1, d1b[0], d1b[1]);
    f2n_distort(k, x[0], x[1] + step1, d1f[0], d1f[1]);
    const float j00 = 1.f + (d0f[0] - d0b[0]) / (2.f * step0);
    const float j01 = (d1f[0] - d1b[0]) / (2.f * step1);
    const float j10 = (d0f[1] - d0b[1]) / (2.f * step0);
    const float j11 = 1.f + (d1f[1] - d1b[1]) / (2.f * step1);
    const float invdet = 1.f / (j00 * j11 - j10 * j01);
    const float i00 = j11 * invdet, i10 = -j10 * invdet, i01 = -j01 * invdet, i11 = j00 * invdet;
    const float r0 = x[0] + dx[0] - x0[0], r1 = x[1] + dx[1] - x0[1];
    const float s0 = i00 * r0 + i01 * r1, s1 = i10 * r0 + i11 * r1;
    x[0] -= s0;
    x[1] -= s1;
    if (s0 * s0 + s1 * s1 < 1e-10f) break;
  }
  u = x[0];
  v = x[1];
}

// Img2WorldRayKernel, Dataset.cu:93-123, with the half-pixel shift of :126 applied here.
__global__ void img2world_kernel(int n_rays, const float* __restrict__ poses, const float* __restrict__ intri,
                                 const float* __restrict__ dist, const int32_t* __restrict__ cam_idx,
                                 const int32_t* __restrict__ ij, float* __restrict__ rays_o, float* __restrict__ rays_d) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const int c = cam_idx[r];
  const float* K = intri + 9 * (size_t) c;
  const float* P = poses + 12 * (size_t) c;
  const float i = (float) ij[2 * r] + .5f, j = (float) ij[2 * r + 1] + .5f;
  const float cx = K[2], cy = K[5], fx = K[0], fy = K[4];
  float u = (j - cx) / fx;
  float v = (i - cy) / fy;  // OpenCV style
  float k[4] = {dist[4 * (size_t) c], dist[4 * (size_t) c + 1], dist[4 * (size_t) c + 2], dist[4 * (size_t) c + 3]};
  f2n_undistort(k, u, v);
  const float dir[3] = {u, -v, -1.f};  // OpenGL style
#pragma unroll
  for (int a = 0; a < 3; a++) {
    rays_d[3 * (size_t) r + a] = f2n_sum3(P[4 * a] * dir[0], P[4 * a + 1] * dir[1], P[4 * a + 2] * dir[2]);
    rays_o[3 * (size_t) r + a] = P[4 * a + 3];
  }
}

// gt_colors[r] = images[cam][i][j] and bounds[r] = cam_bounds[cam] (Dataset.cpp:291-295): resident images, no upload.
__global__ void gather_pixels_kernel(int n_rays, int height, int width, const float* __restrict__ images,
                                     const float* __restrict__ cam_bounds, const int32_t* __restrict__ cam_idx,
                                     const int32_t* __restrict__ ij, float* __restrict__ colors, float* __restrict__ bounds) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const int c = cam_idx[r];
  if (colors != nullptr) {
    const size_t px = ((size_t) c * height + ij[2 * r]) * width + ij[2 * r + 1];
#pragma unroll
    for (int a = 0; a < 3; a++) colors[3 * (size_t) r + a] = images[3 * px + a];
  }
  if (bounds != nullptr) {
    bounds[2 * (size_t) r] = cam_bounds[2 * (size_t) c];
    bounds[2 * (size_t) r + 1] = cam_bounds[2 * (size_t) c + 1];
  }
}

// Dataset::RandRaysData (Dataset.cpp:275-298) in ONE launch: three uniforms per ray pick an image of the set and a pixel, the
// ray is generated (img2world_kernel's arithmetic) and the ground-truth colour / bounds gathered.  The ATen spelling -- three
// randint, an index, a stack, then the two kernels above -- was eight dependent launches on the training step's main queue,
// once per iteration.
__global__ void draw_ray_batch_kernel(int n_rays, const float* __restrict__ u01, unsigned long long key, unsigned long long seq,
                                      const int32_t* __restrict__ image_set, int n_set,
                                      int height, int width, const float* __restrict__ poses, const float* __restrict__ intri,
                                      const float* __restrict__ dist, const float* __restrict__ images,
                                      const float* __restrict__ cam_bounds, int32_t* __restrict__ cam_idx, int32_t* __restrict__ ij,
                                      float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ colors,
                                      float* __restrict__ bounds) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  float u3[3];
  if (u01 != nullptr) {
    u3[0] = u01[3 * (size_t) r]; u3[1] = u01[3 * (size_t) r + 1]; u3[2] = u01[3 * (size_t) r + 2];
  } else {  // keyed: ray r of batch `seq` draws its own three uniforms (no rand launch in front of this kernel)
    uint32_t x[4];
    f2n_philox4x32((uint32_t) r, 0u, (uint32_t) seq, (uint32_t) (seq >> 32), (uint32_t) key, (uint32_t) (key >> 32), x);
    u3[0] = f2n_u01(x[0]); u3[1] = f2n_u01(x[1]); u3[2] = f2n_u01(x[2]);
  }
  const int c = image_set[min((int) (u3[0] * (float) n_set), n_set - 1)];
  const int pi = min((int) (u3[1] * (float) height), height - 1);
  const int pj = min((int) (u3[2] * (float) width), width - 1);
  cam_idx[r] = c;
  ij[2 * r] = pi;
  ij[2 * r + 1] = pj;
  const float* K = intri + 9 * (size_t) c;
  const float* P = poses + 12 * (size_t) c;
  const float i = (float) pi + .5f, j = (float) pj + .5f;
  const float cx = K[2], cy = K[5], fx = K[0], fy = K[4];
  float u = (j - cx) / fx;
  float v = (i - cy) / fy;
  float k[4] = {dist[4 * (size_t) c], dist[4 * (size_t) c + 1], dist[4 * (size_t) c + 2], dist[4 * (size_t) c + 3]};
  f2n_undistort(k, u, v);
  const float dir[3] = {u, -v, -1.f};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    rays_d[3 * (size_t) r + a] = f2n_sum3(P[4 * a] * dir[0], P[4 * a + 1] * dir[1], P[4 * a + 2] * dir[2]);
    rays_o[3 * (size_t) r + a] = P[4 * a + 3];
  }
  if (colors != nullptr) {
    const size_t px = ((size_t) c * height + pi) * width + pj;
#pragma unroll
    for (int a = 0; a < 3; a++) colors[3 * (size_t) r + a] = images[3 * px + a];
  }
  bounds[2 * (size_t) r] = cam_bounds[2 * (size_t) c];
  bounds[2 * (size_t) r + 1] = cam_bounds[2 * (size_t) c + 1];
}

// TSDF fusion of depth maps (include/f2n_abi.h, f2n_tsdf_integrate): the inverse of img2world_kernel's camera model -- a grid point is
// taken into every view's camera frame, distorted (f2n_distort, no Newton: the forward direction of the model) and looked up in that
// view's depth map at the nearest pixel.  One thread owns one voxel and walks the views in index order with its two running sums in
// registers: no atomics, the state is read once and written once, and the sums of a launch over [0, V) are those of launches over
// [0, k) and [k, V).  A view's 20 constants (pose, fx, fy, cx, cy, distortion) are addressed by the loop variable alone: wave-uniform,
// fetched by scalar loads into SGPRs, so that the vector registers hold the voxel's own state only.
// Steps 1-6 of f2n_tsdf_integrate for the point p and the view v: false behind the camera, else q = p - o_v and the point's map
// coordinates (x, y).  v is the callers' loop variable: the view's constants stay wave-uniform.
__device__ __forceinline__ bool tsdf_project(const float p[3], int v, const float* __restrict__ poses, const float* __restrict__ intri,
                                             const float* __restrict__ dist, float q[3], float& x, float& y) {
  const float* P = poses + 12 * (size_t) v;
  const float* K = intri + 9 * (size_t) v;
  q[0] = F2N_SUB_RN(p[0], P[3]);
  q[1] = F2N_SUB_RN(p[1], P[7]);
  q[2] = F2N_SUB_RN(p[2], P[11]);
  float c[3];  // R^T q: the point in the camera frame (x right, y up, z backwards: OpenGL style)
#pragma unroll
  for (int a = 0; a < 3; a++) c[a] = f2n_sum3(F2N_MUL_RN(P[a], q[0]), F2N_MUL_RN(P[4 + a], q[1]), F2N_MUL_RN(P[8 + a], q[2]));
  const float s = -c[2];
  if (!(s > 0.f)) return false;  // behind the camera (NaN as well)
  const float un = F2N_DIV_RN(c[0], s), vn = F2N_DIV_RN(-c[1], s);
  float du, dv;
  f2n_distort(dist + 4 * (size_t) v, un, vn, du, dv);
  x = F2N_ADD_RN(F2N_MUL_RN(K[0], F2N_ADD_RN(un, du)), K[2]);
  y = F2N_ADD_RN(F2N_MUL_RN(K[4], F2N_ADD_RN(vn, dv)), K[5]);
  return true;
}

// Steps 1-10 of f2n_tsdf_integrate for the point p and the view v: false where the view is skipped, else sdf and wgt of steps 9-10.
__device__ __forceinline__ bool tsdf_observe(const float p[3], int v, const float* __restrict__ poses, const float* __restrict__ intri,
                                             const float* __restrict__ dist, const float* __restrict__ depth,
                                             const float* __restrict__ conf, int h, int w, float trunc, float& sdf, float& wgt) {
  float q[3], x, y;
  if (!tsdf_project(p, v, poses, intri, dist, q, x, y)) return false;
  const float fb = floorf(x), fa = floorf(y);
  if (!(fa >= 0.f && fa < (float) h && fb >= 0.f && fb < (float) w)) return false;  // outside the image (NaN as well)
  const size_t px = ((size_t) v * h + (int) fa) * w + (int) fb;
  const float D = depth[px];
  if (!(D > 0.f)) return false;  // no surface along this pixel's ray
  wgt = conf != nullptr ? conf[px] : 1.f;
  if (!(wgt > 0.f)) return false;
  sdf = F2N_SUB_RN(D, f2n_norm3(q[0], q[1], q[2]));
  return !(sdf < -trunc);  // further than trunc behind the surface: not observed
}

// The views [0, n_views) added to the running sums of the voxel at p, in index order (steps 1-12): what the dense kernel and the
// brick kernel both do to a voxel.
__device__ __forceinline__ void tsdf_voxel(const float p[3], int n_views, const float* __restrict__ poses, const float* __restrict__ intri,
                                           const float* __restrict__ dist, const float* __restrict__ depth, const float* __restrict__ conf,
                                           int h, int w, float trunc, float& s_sum, float& w_sum) {
  for (int v = 0; v < n_views; v++) {
    float sdf, wgt;
    if (!tsdf_observe(p, v, poses, intri, dist, depth, conf, h, w, trunc, sdf, wgt)) continue;
    const float ratio = F2N_DIV_RN(sdf, trunc);
    const float d = ratio < 1.f ? ratio : 1.f;
    s_sum = F2N_ADD_RN(s_sum, F2N_MUL_RN(wgt, d));
    w_sum = F2N_ADD_RN(w_sum, wgt);
  }
}

__global__ void __launch_bounds__(256) tsdf_integrate_kernel(int64_t n, int nx, int ny, float lo0, float lo1, float lo2, float step, int n_views,
                                                            const float* __restrict__ poses, const float* __restrict__ intri,
                                                            const float* __restrict__ dist, const float* __restrict__ depth,
                                                            const float* __restrict__ conf, int h, int w, float trunc,
                                                            float* __restrict__ S, float* __restrict__ W) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t plane = (int64_t) nx * ny;
  const int64_t r = i % plane;
  const float p[3] = {f2n_grid_coord(lo0, step, (int) (r % nx)), f2n_grid_coord(lo1, step, (int) (r / nx)),
                      f2n_grid_coord(lo2, step, (int) (i / plane))};
  float s_sum = S[i], w_sum = W[i];
  tsdf_voxel(p, n_views, poses, intri, dist, depth, conf, h, w, trunc, s_sum, w_sum);
  S[i] = s_sum;
  W[i] = w_sum;
}

// ---- sparse TSDF fusion on bricks (include/f2n_abi.h, "Sparse TSDF fusion on bricks") ---------------------------------------------
// The virtual grid and its bricks are those of the sparse mesher (csrc/octree.hip): brick b = (b_z nb_y + b_y) nb_x + b_x reads the
// (B + 1)^3 corners b B + l, local x fastest; a corner with i_k > n_k - 1 does not exist.
struct TsdfBrickGrid {
  float lo[3], step;
  int n[3], nb[3], B;
};

// x0 = the grid index of the local corner (0, 0, 0) of brick b (0 <= b < 2^31: 32-bit arithmetic)
__device__ __forceinline__ void tsdf_brick_origin(const TsdfBrickGrid& g, int b, int x0[3]) {
  const int row = b / g.nb[0];
  x0[0] = (b - row * g.nb[0]) * g.B;
  x0[2] = row / g.nb[1];
  x0[1] = (row - x0[2] * g.nb[1]) * g.B;
  x0[2] *= g.B;
}

// local corner l of the brick at x0: false where it does not exist, else its position
__device__ __forceinline__ bool tsdf_brick_corner(const TsdfBrickGrid& g, int S1, const int x0[3], int l, float p[3]) {
  const int lc[3] = {l % S1, (l / S1) % S1, l / (S1 * S1)};
  bool exists = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int ik = x0[k] + lc[k];
    exists = exists && ik <= g.n[k] - 1;
    p[k] = f2n_grid_coord(g.lo[k], g.step, ik);
  }
  return exists;
}

// tsdf_integrate_kernel for the corners of listed bricks: row (j, l) = brick j of the list, local corner l.  One thread per row entry;
// a corner that does not exist and a brick id outside the grid keep their state.
__global__ void __launch_bounds__(256) tsdf_integrate_bricks_kernel(TsdfBrickGrid g, int64_t n_total, int64_t n,
                                                                   const int32_t* __restrict__ brick_ids, int n_views,
                                                                   const float* __restrict__ poses, const float* __restrict__ intri,
                                                                   const float* __restrict__ dist, const float* __restrict__ depth,
                                                                   const float* __restrict__ conf, int h, int w, float trunc,
                                                                   float* __restrict__ S, float* __restrict__ W) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int P = (g.B + 1) * (g.B + 1) * (g.B + 1);
  const int64_t b = brick_ids[i / P];
  if (b < 0 || b >= n_total) return;
  int x0[3];
  tsdf_brick_origin(g, (int) b, x0);
  float p[3];
  if (!tsdf_brick_corner(g, g.B + 1, x0, (int) (i % P), p)) return;
  float s_sum = S[i], w_sum = W[i];
  tsdf_voxel(p, n_views, poses, intri, dist, depth, conf, h, w, trunc, s_sum, w_sum);
  S[i] = s_sum;
  W[i] = w_sum;
}

// flags[b] = some existing corner of brick b's row has a hit in some view: tsdf_observe and sdf < 0.  One workgroup per brick (the
// bricks strided over the launch's blocks), the views in the outer loop and one corner per lane and round in the inner one (a view's
// constants are loaded once per brick); after every group of F2N_TSDF_MARK_VOTE views the block votes, and a brick with a hit leaves.
// No atomics: a flag is written once, by its own block.
#define F2N_TSDF_MARK_VOTE 4
#define F2N_TSDF_MARK_MAX_BLOCKS (1 << 20)
template <int B>
__global__ void __launch_bounds__(256) tsdf_brick_mark_kernel(TsdfBrickGrid g, unsigned n_total, int n_views, const float* __restrict__ poses,
                                                             const float* __restrict__ intri, const float* __restrict__ dist,
                                                             const float* __restrict__ depth, const float* __restrict__ conf, int h, int w,
                                                             float trunc, uint8_t* __restrict__ flags) {
  constexpr int S1 = B + 1, P = S1 * S1 * S1;
  for (unsigned b = blockIdx.x; b < n_total; b += gridDim.x) {  // (n_total < 2^31 and at most 2^20 blocks: b does not wrap)
    int x0[3];
    tsdf_brick_origin(g, (int) b, x0);
    bool hit = false;
    int any = 0;
    for (int v0 = 0; v0 < n_views && any == 0; v0 += F2N_TSDF_MARK_VOTE) {
      const int v1 = min(v0 + F2N_TSDF_MARK_VOTE, n_views);
#pragma unroll 1  // (one view's constants in SGPRs at a time)
      for (int v = v0; v < v1; v++) {
        for (int l = threadIdx.x; l < P && !hit; l += 256) {
          float p[3], sdf, wgt;
          if (!tsdf_brick_corner(g, S1, x0, l, p)) continue;
          if (tsdf_observe(p, v, poses, intri, dist, depth, conf, h, w, trunc, sdf, wgt) && sdf < 0.f) hit = true;
        }
      }
      any = __syncthreads_or(hit ? 1 : 0);
    }
    if (threadIdx.x == 0) flags[b] = any != 0 ? 1 : 0;
  }
}

// ---- view-colour fusion (include/f2n_abi.h, "View-colour fusion") -------------------------------------------------------------------
// The TSDF kernel's projection turned round: a surface point is taken into every view (tsdf_project), tested for occlusion against
// that view's depth at the four pixels around it, and takes the bilinear blend of the image at the pixels that see it.  One thread
// owns one point and walks the views in index order with its C + 2 running sums in registers (C is a template parameter: no private
// array is indexed dynamically); a view's 20 constants are addressed by the loop variable alone, wave-uniform scalar loads as in
// tsdf_observe.  The rejections that need no map (behind the camera, facing away, no tap in the image) come first; image is read
// for valid taps only.  No atomics: the state is read once and written once.
template <int C>
__global__ void __launch_bounds__(256) view_colors_kernel(int64_t n, const float* __restrict__ points, const float* __restrict__ normals,
                                                         int n_views, const float* __restrict__ poses, const float* __restrict__ intri,
                                                         const float* __restrict__ dist, const float* __restrict__ depth,
                                                         const float* __restrict__ conf, const float* __restrict__ image, int h, int w,
                                                         float tol, float cos_min, float* __restrict__ acc, float* __restrict__ wsum,
                                                         int32_t* __restrict__ count) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
  float nr[3] = {0.f, 0.f, 0.f};
  bool has_normal = false;
  if (normals != nullptr) {
    nr[0] = normals[3 * i]; nr[1] = normals[3 * i + 1]; nr[2] = normals[3 * i + 2];
    const float inf = __builtin_huge_valf();
    has_normal = fabsf(nr[0]) < inf && fabsf(nr[1]) < inf && fabsf(nr[2]) < inf && (nr[0] != 0.f || nr[1] != 0.f || nr[2] != 0.f);
  }
  float a_sum[C];
#pragma unroll
  for (int c = 0; c < C; c++) a_sum[c] = acc[C * i + c];
  float w_sum = wsum[i];
  int cnt = count[i];
  const float fh = (float) h, fw = (float) w;
  for (int v = 0; v < n_views; v++) {
    float q[3], x, y;
    if (!tsdf_project(p, v, poses, intri, dist, q, x, y)) continue;
    const float r = f2n_norm3(q[0], q[1], q[2]);
    float facing = 1.f;
    if (has_normal) {
      facing = F2N_DIV_RN(f2n_sum3(F2N_MUL_RN(nr[0], -q[0]), F2N_MUL_RN(nr[1], -q[1]), F2N_MUL_RN(nr[2], -q[2])), r);
      if (!(facing > cos_min)) continue;  // seen from behind or at a grazing angle (NaN as well)
    }
    const float xs = F2N_SUB_RN(x, .5f), ys = F2N_SUB_RN(y, .5f);
    const float b0 = floorf(xs), a0 = floorf(ys);
    if (!(a0 >= -1.f && a0 < fh && b0 >= -1.f && b0 < fw)) continue;  // no tap exists (NaN as well)
    const float fx = F2N_SUB_RN(xs, b0), fy = F2N_SUB_RN(ys, a0);
    const float wy[2] = {F2N_SUB_RN(1.f, fy), fy}, wx[2] = {F2N_SUB_RN(1.f, fx), fx};
    float om = 0.f, col[C];
#pragma unroll
    for (int c = 0; c < C; c++) col[c] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float ta = F2N_ADD_RN(a0, (float) (k >> 1)), tb = F2N_ADD_RN(b0, (float) (k & 1));
      if (!(ta >= 0.f && ta < fh && tb >= 0.f && tb < fw)) continue;  // beyond the border: no observation
      const size_t px = ((size_t) v * h + (int) ta) * w + (int) tb;
      const float D = depth[px];
      if (!(D > 0.f)) continue;
      const float cf = conf != nullptr ? conf[px] : 1.f;
      if (!(cf > 0.f)) continue;
      const float d = F2N_SUB_RN(D, r);
      if (d < -tol || d > tol) continue;  // occluded in this view, or in front of what it sees
      const float ok = F2N_MUL_RN(F2N_MUL_RN(wy[k >> 1], wx[k & 1]), cf);
      om = F2N_ADD_RN(om, ok);
#pragma unroll
      for (int c = 0; c < C; c++) col[c] = F2N_ADD_RN(col[c], F2N_MUL_RN(ok, image[C * px + c]));
    }
    if (!(om > 0.f)) continue;
#pragma unroll
    for (int c = 0; c < C; c++) a_sum[c] = F2N_ADD_RN(a_sum[c], F2N_MUL_RN(facing, col[c]));
    w_sum = F2N_ADD_RN(w_sum, F2N_MUL_RN(facing, om));
    cnt += 1;
  }
#pragma unroll
  for (int c = 0; c < C; c++) acc[C * i + c] = a_sum[c];
  wsum[i] = w_sum;
  count[i] = cnt;
}

__global__ void __launch_bounds__(256) view_colors_finalize_kernel(int64_t n, int C, const float* __restrict__ acc,
                                                                  const float* __restrict__ wsum, const int32_t* __restrict__ count,
                                                                  int min_views, float* __restrict__ rgb, uint8_t* __restrict__ known) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float ws = wsum[i];
  const bool ok = count[i] >= min_views && ws > 0.f;
  for (int c = 0; c < C; c++) rgb[C * i + c] = ok ? F2N_DIV_RN(acc[C * i + c], ws) : 0.f;
  known[i] = ok ? 1 : 0;
}

// SSIM of two images (include/f2n_abi.h, f2n_image_ssim; scripts/eval.py:29-75, the mip-NeRF definition): fp64 throughout, one rounding per
// operation, every sum in a fixed tap order, the mean as an exact integer sum -- so an image's SSIM is a function of the two images
// alone.  A 256-thread block owns a 16 x 32 tile of outputs (blockIdx.x, row-major) of ONE channel (blockIdx.z) with its fs - 1 halo:
//   stage:      the (16 + fs - 1) x (32 + fs - 1) pixels of a and b as floats in LDS (pixels beyond the image: 0, they feed only outputs
//               that do not exist);
//   vertical:   one item per (output row, input column): the five window sums x, y, xx, yy, xy down the column, taps ascending, in
//               registers, then to LDS as doubles (adjacent lanes, adjacent columns: no bank conflict);
//   horizontal: one item per output: the five sums along the row from LDS, the formula, the map, the lane's fixed-point pair;
//   reduce:     integer sums over the wave (shuffles), over the four waves (LDS), then ONE 64-bit vector atomic per statistic.
// Dynamic LDS: (16 + fs - 1)(32 + fs - 1) 8 B + 5 x 16 (32 + fs - 1) 8 B: 35.6 KB for fs = 11, 64 KB for fs = 33 (the cross-wave sums
// reuse the staging area).
#define F2N_SSIM_TILE_H 16
#define F2N_SSIM_TILE_W 32
#define F2N_SSIM_MAX_FS 33

struct SsimWindow {
  double w[F2N_SSIM_MAX_FS];
};

// lines 56-73 of the reference for one output; the comparisons are spelled out so that a NaN goes through as numpy's maximum / minimum /
// sign carry it
__device__ __forceinline__ double f2n_ssim_value(double m0, double m1, double b00, double b11, double b01, double c1, double c2) {
  const double mu00 = m0 * m0, mu11 = m1 * m1, mu01 = m0 * m1;
  double s00 = b00 - mu00, s11 = b11 - mu11, s01 = b01 - mu01;
  s00 = s00 < 0.0 ? 0.0 : s00;
  s11 = s11 < 0.0 ? 0.0 : s11;
  const double t = sqrt(s00 * s11), a = fabs(s01);
  const double m = t < a ? t : a;
  s01 = s01 < 0.0 ? -m : m;
  const double numer = (2.0 * mu01 + c1) * (2.0 * s01 + c2);
  const double denom = ((mu00 + mu11) + c1) * ((s00 + s11) + c2);
  return numer / denom;
}

__global__ void __launch_bounds__(256) image_ssim_kernel(int height, int width, int channels, const float* __restrict__ img_a,
                                                         const float* __restrict__ img_b, SsimWindow win, int fs, double c1, double c2,
                                                         double* __restrict__ map, unsigned long long* __restrict__ stats) {
  extern __shared__ double ssim_lds[];
  const int tid = threadIdx.x, c = blockIdx.z;
  const int oh = height - fs + 1, ow = width - fs + 1;
  const int tiles_x = (ow + F2N_SSIM_TILE_W - 1) / F2N_SSIM_TILE_W;  // (tiles are numbered along blockIdx.x: a grid's y extent is 65535)
  const int tile_y = blockIdx.x / tiles_x;
  const int y0 = tile_y * F2N_SSIM_TILE_H, x0 = (blockIdx.x - tile_y * tiles_x) * F2N_SSIM_TILE_W;
  const int in_rows = F2N_SSIM_TILE_H + fs - 1, in_cols = F2N_SSIM_TILE_W + fs - 1;
  float* raw_a = (float*) ssim_lds;
  float* raw_b = raw_a + in_rows * in_cols;
  double* vert = ssim_lds + in_rows * in_cols;  // [5][TILE_H][in_cols]
  const int plane = F2N_SSIM_TILE_H * in_cols;
  for (int i = tid; i < in_rows * in_cols; i += 256) {
    const int r = i / in_cols, j = i - r * in_cols;
    const int y = y0 + r, x = x0 + j;
    float va = 0.f, vb = 0.f;
    if (y < height && x < width) {
      const size_t px = ((size_t) y * width + x) * channels + c;
      va = img_a[px];
      vb = img_b[px];
    }
    raw_a[i] = va;
    raw_b[i] = vb;
  }
  __syncthreads();
  for (int i = tid; i < plane; i += 256) {
    const int r = i / in_cols, j = i - r * in_cols;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int k = 0; k < fs; k++) {
      const double w = win.w[k];
      const double x = (double) raw_a[(r + k) * in_cols + j], y = (double) raw_b[(r + k) * in_cols + j];
      sx = sx + w * x;
      sy = sy + w * y;
      sxx = sxx + w * (x * x);
      syy = syy + w * (y * y);
      sxy = sxy + w * (x * y);
    }
    vert[i] = sx;
    vert[plane + i] = sy;
    vert[2 * plane + i] = sxx;
    vert[3 * plane + i] = syy;
    vert[4 * plane + i] = sxy;
  }
  __syncthreads();
  long long sum = 0, cnt = 0;
  for (int i = tid; i < F2N_SSIM_TILE_H * F2N_SSIM_TILE_W; i += 256) {
    const int r = i / F2N_SSIM_TILE_W, j = i - r * F2N_SSIM_TILE_W;
    const int y = y0 + r, x = x0 + j;
    if (y >= oh || x >= ow) continue;
    const double* v = vert + r * in_cols + j;
    double m0 = 0.0, m1 = 0.0, b00 = 0.0, b11 = 0.0, b01 = 0.0;
    for (int k = 0; k < fs; k++) {
      const double w = win.w[k];
      m0 = m0 + w * v[k];
      m1 = m1 + w * v[plane + k];
      b00 = b00 + w * v[2 * plane + k];
      b11 = b11 + w * v[3 * plane + k];
      b01 = b01 + w * v[4 * plane + k];
    }
    const double val = f2n_ssim_value(m0, m1, b00, b11, b01, c1, c2);
    if (map != nullptr) map[((size_t) y * ow + x) * channels + c] = val;
    if (fabs(val) < __builtin_huge_val()) {  // (false for a NaN as well)
      sum += __double2ll_rn(val * 68719476736.0);
      cnt += 1;
    }
  }
  // integers: any order gives the same sums
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    sum += __shfl_xor(sum, d);
    cnt += __shfl_xor(cnt, d);
  }
  __syncthreads();  // (the staging area is free from here on)
  long long* part = (long long*) ssim_lds;
  if ((tid & 63) == 0) {
    part[2 * (tid >> 6)] = sum;
    part[2 * (tid >> 6) + 1] = cnt;
  }
  __syncthreads();
  if (tid < 2) {
    const long long tot = (part[tid] + part[2 + tid]) + (part[4 + tid] + part[6 + tid]);
    if (tot != 0) atomicAdd(stats + 2 * c + tid, (unsigned long long) tot);
  }
}

extern "C" {

int f2n_tsdf_integrate(void* stream, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int n_views, const float* poses,
                       const float* intri, const float* dist_params, const float* depth, const float* conf, int h, int w, float trunc,
                       float* S, float* W) {
  if (lo == nullptr || nx < 0 || ny < 0 || nz < 0 || n_views < 0 || h < 0 || w < 0 || !(trunc > 0.f) || !(trunc < __builtin_huge_valf()))
    return F2N_ERR_INVALID_ARG;
  const int64_t n = (int64_t) nx * ny * nz;
  if (n_views == 0 || n == 0) return F2N_OK;
  // (pixel coordinates are compared as floats: exact up to 2^24; a depth map's index is computed in 64 bits)
  if (h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24) || n > (int64_t) 0x7fffffff * 256) return F2N_ERR_INVALID_ARG;
  if (poses == nullptr || intri == nullptr || dist_params == nullptr || depth == nullptr || S == nullptr || W == nullptr)
    return F2N_ERR_INVALID_ARG;
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, nx, ny, lo[0], lo[1], lo[2],
                     step, n_views, poses, intri, dist_params, depth, conf, h, w, trunc, S, W);
  return f2n_launch_status();
}

// the brick grid of (n, B), or the status that refuses it (as csrc/octree.hip's)
static int tsdf_brick_grid(const float* lo, float step, int nx, int ny, int nz, int B, TsdfBrickGrid* g, int64_t* n_total) {
  if (nx < 2 || ny < 2 || nz < 2 || nx > F2N_BRICK_MAX_POINTS || ny > F2N_BRICK_MAX_POINTS || nz > F2N_BRICK_MAX_POINTS) return F2N_ERR_INVALID_ARG;
  if (B != 4 && B != 8 && B != 16) return F2N_ERR_INVALID_ARG;
  const int n[3] = {nx, ny, nz};
  for (int k = 0; k < 3; k++) {
    g->lo[k] = lo[k];
    g->n[k] = n[k];
    g->nb[k] = (n[k] - 1 + B - 1) / B;
  }
  g->step = step;
  g->B = B;
  *n_total = (int64_t) g->nb[0] * g->nb[1] * g->nb[2];
  return *n_total > 0x7fffffff ? F2N_ERR_UNSUPPORTED : F2N_OK;
}

int f2n_tsdf_brick_mark(void* stream, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int B, int n_views, const float* poses,
                        const float* intri, const float* dist_params, const float* depth, const float* conf, int h, int w, float trunc,
                        uint8_t* flags) {
  if (lo == nullptr || n_views < 0 || h < 0 || w < 0 || !(trunc > 0.f) || !(trunc < __builtin_huge_valf())) return F2N_ERR_INVALID_ARG;
  TsdfBrickGrid g;
  int64_t n_total;
  const int e = tsdf_brick_grid(lo, step, nx, ny, nz, B, &g, &n_total);
  if (e != F2N_OK) return e;
  if (n_views == 0) return F2N_OK;
  if (h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24)) return F2N_ERR_INVALID_ARG;
  if (poses == nullptr || intri == nullptr || dist_params == nullptr || depth == nullptr || flags == nullptr) return F2N_ERR_INVALID_ARG;
  const unsigned blocks = (unsigned) (n_total < F2N_TSDF_MARK_MAX_BLOCKS ? n_total : F2N_TSDF_MARK_MAX_BLOCKS);
#define F2N_TSDF_MARK(BB)                                                                                                              \
  hipLaunchKernelGGL(tsdf_brick_mark_kernel<BB>, dim3(blocks), dim3(256), 0, (hipStream_t) stream, g, (unsigned) n_total, n_views, poses, \
                     intri, dist_params, depth, conf, h, w, trunc, flags)
  if (B == 4) F2N_TSDF_MARK(4);
  else if (B == 8) F2N_TSDF_MARK(8);
  else F2N_TSDF_MARK(16);
#undef F2N_TSDF_MARK
  return f2n_launch_status();
}

int f2n_tsdf_integrate_bricks(void* stream, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int B, int n_bricks,
                              const int32_t* brick_ids, int n_views, const float* poses, const float* intri, const float* dist_params,
                              const float* depth, const float* conf, int h, int w, float trunc, float* S, float* W) {
  if (lo == nullptr || n_bricks < 0 || n_views < 0 || h < 0 || w < 0 || !(trunc > 0.f) || !(trunc < __builtin_huge_valf()))
    return F2N_ERR_INVALID_ARG;
  TsdfBrickGrid g;
  int64_t n_total;
  const int e = tsdf_brick_grid(lo, step, nx, ny, nz, B, &g, &n_total);
  if (e != F2N_OK) return e;
  const int64_t n = (int64_t) n_bricks * (B + 1) * (B + 1) * (B + 1);
  if (n > 0x7fffffff) return F2N_ERR_INVALID_ARG;
  if (n_views == 0 || n == 0) return F2N_OK;
  if (h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24)) return F2N_ERR_INVALID_ARG;
  if (brick_ids == nullptr || poses == nullptr || intri == nullptr || dist_params == nullptr || depth == nullptr || S == nullptr || W == nullptr)
    return F2N_ERR_INVALID_ARG;
  hipLaunchKernelGGL(tsdf_integrate_bricks_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, g, n_total, n, brick_ids,
                     n_views, poses, intri, dist_params, depth, conf, h, w, trunc, S, W);
  return f2n_launch_status();
}

int f2n_view_colors_accumulate(void* stream, int64_t n, const float* points, const float* normals, int n_views, const float* poses,
                               const float* intri, const float* dist_params, const float* depth, const float* conf, const float* image, int C,
                               int h, int w, float tol, float cos_min, float* acc, float* wsum, int32_t* count) {
  if (n < 0 || n_views < 0 || h < 0 || w < 0 || C < 1 || C > 4 || !(tol > 0.f) || !(tol < __builtin_huge_valf()) || cos_min != cos_min)
    return F2N_ERR_INVALID_ARG;
  if (n_views == 0 || n == 0) return F2N_OK;
  if (h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24) || n > (int64_t) 0x7fffffff * 256) return F2N_ERR_INVALID_ARG;
  if (points == nullptr || poses == nullptr || intri == nullptr || dist_params == nullptr || depth == nullptr || image == nullptr ||
      acc == nullptr || wsum == nullptr || count == nullptr)
    return F2N_ERR_INVALID_ARG;
#define F2N_VIEW_COLORS(CC)                                                                                                            \
  hipLaunchKernelGGL(view_colors_kernel<CC>, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, points, normals, n_views, \
                     poses, intri, dist_params, depth, conf, image, h, w, tol, cos_min, acc, wsum, count)
  if (C == 1) F2N_VIEW_COLORS(1);
  else if (C == 2) F2N_VIEW_COLORS(2);
  else if (C == 3) F2N_VIEW_COLORS(3);
  else F2N_VIEW_COLORS(4);
#undef F2N_VIEW_COLORS
  return f2n_launch_status();
}

int f2n_view_colors_finalize(void* stream, int64_t n, int C, const float* acc, const float* wsum, const int32_t* count, int min_views,
                             float* rgb, uint8_t* known) {
  if (n < 0 || C < 1 || C > 4 || n > (int64_t) 0x7fffffff * 256) return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  if (acc == nullptr || wsum == nullptr || count == nullptr || rgb == nullptr || known == nullptr) return F2N_ERR_INVALID_ARG;
  hipLaunchKernelGGL(view_colors_finalize_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, C, acc, wsum, count,
                     min_views, rgb, known);
  return f2n_launch_status();
}

int f2n_draw_ray_batch(void* stream, int n_rays, const float* u01, const int32_t* image_set, int n_set, int height, int width,
                       const float* poses, const float* intri, const float* dist_params, const float* images, const float* cam_bounds,
                       int32_t* cam_indices, int32_t* ij, float* rays_o, float* rays_d, float* gt_colors, float* bounds) {
  if (n_rays < 0 || n_set < 1 || height <= 0 || width <= 0 || (gt_colors != nullptr && images == nullptr) || cam_bounds == nullptr || u01 == nullptr)
    return F2N_ERR_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  hipLaunchKernelGGL(draw_ray_batch_kernel, dim3(f2n_div_up(n_rays, 256)), dim3(256), 0, (hipStream_t) stream, n_rays, u01, 0ull, 0ull, image_set,
                     n_set, height, width, poses, intri, dist_params, images, cam_bounds, cam_indices, ij, rays_o, rays_d, gt_colors,
                     bounds);
  return f2n_launch_status();
}

int f2n_draw_ray_batch_keyed(void* stream, int n_rays, uint64_t key, uint64_t seq, const int32_t* image_set, int n_set, int height, int width,
                             const float* poses, const float* intri, const float* dist_params, const float* images, const float* cam_bounds,
                             int32_t* cam_indices, int32_t* ij, float* rays_o, float* rays_d, float* gt_colors, float* bounds) {
  if (n_rays < 0 || n_set < 1 || height <= 0 || width <= 0 || (gt_colors != nullptr && images == nullptr) || cam_bounds == nullptr)
    return F2N_ERR_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  hipLaunchKernelGGL(draw_ray_batch_kernel, dim3(f2n_div_up(n_rays, 256)), dim3(256), 0, (hipStream_t) stream, n_rays, (const float*) nullptr,
                     (unsigned long long) key, (unsigned long long) seq, image_set, n_set, height, width, poses, intri, dist_params, images,
                     cam_bounds, cam_indices, ij, rays_o, rays_d, gt_colors, bounds);
  return f2n_launch_status();
}

int f2n_img2world_rays(void* stream, int n_rays, const float* poses, const float* intri, const float* dist_params,
                       const int32_t* cam_indices, const int32_t* ij, float* rays_o, float* rays_d) {
  if (n_rays < 0) return F2N_ERR_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  hipLaunchKernelGGL(img2world_kernel, dim3(f2n_div_up(n_rays, 256)), dim3(256), 0, (hipStream_t) stream, n_rays, poses, intri,
                     dist_params, cam_indices, ij, rays_o, rays_d);
  return f2n_launch_status();
}

int f2n_gather_pixels(void* stream, int n_rays, int height, int width, const float* images, const float* cam_bounds,
                      const int32_t* cam_indices, const int32_t* ij, float* gt_colors, float* bounds) {
  if (n_rays < 0 || height <= 0 || width <= 0) return F2N_ERR_INVALID_ARG;
  if (gt_colors != nullptr && images == nullptr) return F2N_ERR_INVALID_ARG;
  if (bounds != nullptr && cam_bounds == nullptr) return F2N_ERR_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  hipLaunchKernelGGL(gather_pixels_kernel, dim3(f2n_div_up(n_rays, 256)), dim3(256), 0, (hipStream_t) stream, n_rays, height, width,
                     images, cam_bounds, cam_indices, ij, gt_colors, bounds);
  return f2n_launch_status();
}

int f2n_ssim_window(int filter_size, double sigma, double* out) {
  if (filter_size < 1 || filter_size > F2N_SSIM_MAX_FS || !(sigma > 0.0) || !(sigma < __builtin_huge_val()) || out == nullptr)
    return F2N_ERR_INVALID_ARG;
  const int hw = filter_size / 2;
  const double shift = (double) (2 * hw - filter_size + 1) / 2.0;
  double sum = 0.0;
  for (int i = 0; i < filter_size; i++) {
    const double u = ((double) (i - hw) + shift) / sigma;
    out[i] = exp(-0.5 * (u * u));
    sum = sum + out[i];
  }
  for (int i = 0; i < filter_size; i++) out[i] = out[i] / sum;
  return F2N_OK;
}

int f2n_image_ssim(void* stream, int height, int width, int channels, const float* a, const float* b, const double* window, int filter_size,
                   double c1, double c2, double* map_or_null, int64_t* stats) {
  if (channels < 1 || channels > 4 || filter_size < 1 || filter_size > F2N_SSIM_MAX_FS || height < filter_size || width < filter_size ||
      a == nullptr || b == nullptr || window == nullptr || stats == nullptr)
    return F2N_ERR_INVALID_ARG;
  const int oh = height - filter_size + 1, ow = width - filter_size + 1;
  if ((int64_t) oh * ow > ((int64_t) 1 << 26)) return F2N_ERR_INVALID_ARG;
  const unsigned tiles = f2n_div_up(oh, F2N_SSIM_TILE_H) * f2n_div_up(ow, F2N_SSIM_TILE_W);  // (at most 2^26 outputs: below 2^27 tiles)
  SsimWindow win;
  for (int k = 0; k < F2N_SSIM_MAX_FS; k++) win.w[k] = k < filter_size ? window[k] : 0.0;
  const hipError_t e = hipMemsetAsync(stats, 0, sizeof(int64_t) * 2 * channels, (hipStream_t) stream);
  if (e != hipSuccess) return -(1000 + (int) e);
  const int in_rows = F2N_SSIM_TILE_H + filter_size - 1, in_cols = F2N_SSIM_TILE_W + filter_size - 1;
  const size_t lds = sizeof(double) * ((size_t) in_rows * in_cols + 5 * (size_t) F2N_SSIM_TILE_H * in_cols);
  hipLaunchKernelGGL(image_ssim_kernel, dim3(tiles, 1, channels), dim3(256), lds, (hipStream_t) stream, height,
                     width, channels, a, b, win, filter_size, c1, c2, map_or_null, (unsigned long long*) stats);
  return f2n_launch_status();
}

void f2n_ssim_tile(int* tile_h, int* tile_w) {
  *tile_h = F2N_SSIM_TILE_H;
  *tile_w = F2N_SSIM_TILE_W;
}

}  // extern "C"
