/* f2n_abi.h -- C-ABI of the MI355X-native (gfx950, HIP) implementation of F2-NeRF's per-ray hot path.
 *
 * The reference (Totoro97/f2-nerf) has no FFI: its hot path is a set of first-party CUDA kernels launched
 * from C++ plugin classes (PersSampler / Hash3DAnchored / SHShader / Renderer) plus the third-party
 * tiny-cuda-nn `tcnn::cpp::Module`.  This header declares, seam for seam, what a binding for that path
 * would bind; each entry point cites the reference interface it replaces (paths relative to
 * /root/reference/src).  INTEGRATION.md shows the reference-side stubs.
 *
 * Conventions
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).  Every call only ENQUEUES work on
 *     that stream; nothing here allocates or frees caller-visible memory.
 *   - Internal scratch: the backward / loss / large-batch field entry points (f2n_field_fwd for n >= 8192, f2n_field_bwd*,
 *     f2n_mlp_bwd, f2n_shade_bwd*, f2n_hash_bwd with level_entries > 0, f2n_train_loss) keep per-block partial sums, feature
 *     planes and scatter queues in ONE library-owned workspace per device and slot.  Consequences: (a) calls that share a
 *     slot must be issued on ONE stream per device (or be ordered by the caller) -- two streams running f2n_field_bwd at
 *     the same time would share partials; the host layer issues all of them on the compute stream and only sampler kernels
 *     (which use no workspace) on its side stream; (b) the first calls, and a call that needs more scratch than any before
 *     it, grow the workspace: that path drains the device (hipDeviceSynchronize) before the old buffer is released,
 *     because queued kernels may still hold it.  Sizes settle after the first iterations; steady-state calls never
 *     synchronise.
 *   - All pointers are DEVICE pointers to contiguous buffers in exactly the layouts named below, unless
 *     the parameter is documented as host data.  TreeNode = 64 B, TransInfo = 544 B, EdgePool = 64 B as in
 *     PtsSampler/PersSampler.h:15-37.  "h16" = IEEE binary16.
 *   - Return value: 0 on success, F2N_ERR_* (< 0) otherwise; a HIP launch error e is returned as
 *     -(1000 + e).  Callable from any host thread (e.g. the autograd engine thread); the caller selects
 *     the device (hipSetDevice) before calling.
 *   - Variable-length results use count -> f2n_segment_scan -> fill, so no host read-back is needed:
 *     callers may size outputs for the worst case (n_rays * 1024) and read totals lazily.
 */
#ifndef F2N_ABI_H
#define F2N_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F2N_OK 0
#define F2N_ERR_INVALID_ARG (-1)
#define F2N_ERR_UNSUPPORTED (-2)

#define F2N_N_LEVELS 16            /* Field/Hash3DAnchored.h:16 */
#define F2N_N_CHANNELS 2           /* Field/Hash3DAnchored.h:15 */
#define F2N_MAX_SAMPLE_PER_RAY 1024 /* PtsSampler/PersSampler.cu:9 */
#define F2N_MLP_OUT_PAD 16         /* tcnn FullyFusedMLP pads the output width to 16 */

/* Library / device introspection (host-only). */
int f2n_abi_version(void);
/* 0 = product numerics; 1 = the reference-numerics build of this library (libf2n_hip_refnum.so, -DF2N_REFERENCE_NUMERICS=1):
 * the two places where the product deviates from the reference's arithmetic ON PURPOSE are switched back -- the hash
 * gradient is accumulated by per-addend packed-f16 atomics in arrival order (Hash3DAnchored.cu:145-153) instead of fp32 /
 * fp64 owner sums rounded once, and the MLP forward products use an f16 accumulator fragment (the other plausible reading
 * of tcnn's FullyFusedMLP).  Same ABI; used to A/B whole trainings (bench.py "psnr_numerics_ab"). */
int f2n_numerics_mode(void);
const char* f2n_build_info(void);
/* Data-parallel runs (one all-reduce of the hash-table gradient per step): the owner launch of the binned scatter behind
 * f2n_hash_bwd / f2n_field_bwd[_dyn] can be cut into n_buckets launches over contiguous ranges of table slices -- bucket b = slices
 * [b * S / n, (b + 1) * S / n) of the S = 17 * (level_entries / 8192) slices of 4096 entries (8192 halves) that the active prefix of
 * the table spans -- and fn(user, b, n) is called on the calling host thread right behind bucket b's launch: that range of the
 * gradient table is final once the launch has run, so its all-reduce can start (on another stream, behind an event) while the
 * later buckets' owners still run, instead of the whole 17 MiB waiting for the step's last kernel.  Per device; n_buckets <= 1 or
 * fn == NULL removes the hook.  A scatter that does not take the binned path (small batches, tiny tables) calls nothing: the caller
 * sends what is left when the backward returns (host/DataParallel.cpp). */
typedef void (*f2n_bucket_fn)(void* user, int bucket, int n_buckets);
int f2n_set_scatter_buckets(int n_buckets, f2n_bucket_fn fn, void* user);
/* ABI v13 (round-5 advisor): the hook is for ONE gradient table -- only a scatter into grad_table_h16 is cut into buckets and
 * reports them; any other f2n_hash_bwd / f2n_field_bwd on the device (a second runner, a test, a taped backward into another
 * buffer) runs its owner launch in one piece and calls nobody.  grad_table_h16 == NULL: whatever table (the v12 behaviour). */
int f2n_set_scatter_buckets_for(int n_buckets, f2n_bucket_fn fn, void* user, const void* grad_table_h16);
/* (an addition to ABI v13) Which instantiation of the producer kernel the owner-binned scatter behind f2n_hash_bwd / f2n_field_bwd[_dyn] /
 * the step tail launches, for the whole process: 1 (the default) = the staged instantiation, which keeps its level's hash constants in
 * LDS (three blocks per CU; pools of more than 512 transforms still get the non-staged one); 0 = the non-staged instantiation (constants
 * from global memory behind the transform index, four blocks per CU), kept for A/B measurements.  Both fill the same queue segments with the same records -- in
 * another order, which the owners' exact sums do not see: the gradient table is the same byte for byte as long as
 * f2n_debug_counters()[0] stays 0.  Host-only; takes effect with the next launch.  Any other value: F2N_ERR_INVALID_ARG. */
int f2n_set_scatter_producer(int variant);
/* Diagnostics (host-only, synchronous; no reference counterpart): eight device-side event counters copied to host memory,
 * optionally reset.  [0] = scatter records of f2n_hash_bwd's owner-binned path that found their queue segment full and were
 * applied by a packed-f16 atomic instead (the only order-dependent addition of that path); [1] = table slices whose owner left
 * its packed fixed-point image for exact fp64 sums because the slice's addends could have left the 32-bit fields' range (same
 * bits either way: a cost counter, not an error counter); [2] (debug variant only) = the largest sum of |addend| an owner saw in
 * a slice, as float bits; [3] = scatter records that found their queue segment full and travelled through their producer block's
 * overflow list instead (summed by the owners like every other record: order-free; [0] counts only what found that list full
 * too).  The rest are reserved (0). */
int f2n_debug_counters(int32_t* out8_host /* or NULL */, int reset);
/* (The two debugging launches of rounds 3-4 -- a delay on a stream, a launch that leaves garbage in every CU's LDS and registers
 * -- are not part of this ABI: include/f2n_debug.h, compiled into the debug variant of the library only.) */

/* ---------------------------------------------------------------------------------------------------
 * Sampler -- replaces PersSampler::GetSamples' kernels (PtsSampler/PersSampler.cu:21-434).
 * ------------------------------------------------------------------------------------------------- */

/* rays_d / ||rays_d|| (PersSampler.cu:319, torch::linalg_norm there).  Fixed fp32 order: sqrt((x*x + y*y) + z*z),
 * IEEE division, so that the CPU oracle restates it bit for bit.  out may alias dirs. */
int f2n_normalize_dirs(void* stream, int n, const float* dirs /*[n,3]*/, float* out /*[n,3]*/);
/* f2n_normalize_dirs + zero[0..n_zero) = 0 (the hit / sample totals of f2n_oct_intersect_strided / f2n_segment_scan) +
 * f2n_march_noise (u -> noise_out, n_noise values; 0: none) in ONE launch: the head of a GetSamples call. */
int f2n_sampler_prologue(void* stream, int n_rays, const float* dirs, float* out, int32_t* zero, int n_zero, int n_noise,
                         const float* u, float fineness, float* noise_out);
/* The same with the march noise DRAWN by the launch (round 5): element i of the noise is uniform number i of the batch with sequence
 * number `seq` under `key` (Philox4x32-10, counter = (i / 4, 0, seq), key = seed ^ purpose: host/KeyedDraws.h) -- a function of what
 * the draw is for, not of how many draws were made before it -- mapped like f2n_march_noise.  No rand launch in front of the chain. */
int f2n_sampler_prologue_keyed(void* stream, int n_rays, const float* dirs, float* out, int32_t* zero, int n_zero, int n_noise,
                               uint64_t key, uint64_t seq, float fineness, float* noise_out /*[n_noise]*/);

/* FindRayOctreeIntersectionKernel<false> (PersSampler.cu:53-152, launched :342-351).
 * rays_d must already be unit length (GetSamples normalises at :319); [near, far] is the global bound the
 * reference substitutes for its `bounds` argument (:322-323: near = pts_sampler.near, far = 1e8).
 * hit_counts[r] = number of valid leaves hit by ray r, capped at max_hits. */
int f2n_oct_intersect_count(void* stream, int n_rays, int max_hits, const uint8_t* search_order /*[64]*/,
                            const float* rays_o /*[R,3]*/, const float* rays_d /*[R,3]*/, float near_, float far_,
                            const void* tree_nodes, int32_t* hit_counts /*[R]*/, const void* child_blocks /*or NULL*/);

/* Ray-ordered segment allocation: start_end[i] = (sum_{j<i} counts[j], sum_{j<=i} counts[j]);
 * total[0] = sum.  Replaces the racing atomicAdd allocator (PersSampler.cu:144) and the
 * torch::cumsum + .item() host sync (:395-397); also FilterIdxBounds' cumsum (Renderer/Renderer.cu:44-48).
 * Any n in [0, 2^31 - 1] is accepted (n < 0: F2N_ERR_INVALID_ARG): the element index, the chunk counter and the start_end offset 2 i
 * are 64-bit for n > 2^29 and 32-bit below, where nothing can overflow (one instantiation of the kernel each; the results are the
 * same).  The sums themselves are int32: the caller keeps the total below 2^31. */
int f2n_segment_scan(void* stream, int n, const int32_t* counts, int32_t* start_end /*[n,2]*/, int32_t* total /*[1]*/);
/* The same, and the host's copy of the result from the same launch: `mirror` (or NULL) is a DEVICE pointer to MAPPED HOST
 * memory (hipHostMallocMapped + hipHostGetDevicePointer) that receives also[0..n_also) followed by the total -- e.g. the hit
 * total of f2n_oct_intersect_strided next to the sample total, the pair the reference reads back with two .item() calls
 * (PersSampler.cu:353,397).  The host reads it after an event recorded behind this call; no device-to-host copy is queued
 * (on an in-order queue that copy is one more dependent launch between the scan and the kernel that consumes it).
 * n_also <= 4. */
int f2n_segment_scan_ex(void* stream, int n, const int32_t* counts, int32_t* start_end /*[n,2]*/, int32_t* total /*[1]*/,
                        int32_t* mirror /*mapped host [n_also+1] or NULL*/, const int32_t* also /*device [n_also] or NULL*/,
                        int n_also);

/* FindRayOctreeIntersectionKernel<true> (PersSampler.cu:357-366): fills each ray's segment with
 * (leaf node index, t_near, t_far), front to back. */
int f2n_oct_intersect_fill(void* stream, int n_rays, const uint8_t* search_order, const float* rays_o,
                           const float* rays_d, float near_, float far_, const void* tree_nodes,
                           const int32_t* oct_start_end /*[R,2]*/, int32_t* oct_idx /*[K]*/,
                           float* oct_near_far /*[K,2]*/, const void* child_blocks /*or NULL*/);

/* Single-pass variant of count + scan + fill for callers that do not need a compact list: ray r owns the fixed
 * slot range [r*max_hits, r*max_hits + hits_r) of oct_idx / oct_near_far (both sized n_rays*max_hits);
 * oct_start_end[r] = that range, total[0] += sum of hits (must be zeroed by the caller).  Per-ray contents are
 * identical to the count/fill pair; the march kernels accept either segment layout. */
int f2n_oct_intersect_strided(void* stream, int n_rays, int max_hits, const uint8_t* search_order, const float* rays_o,
                              const float* rays_d, float near_, float far_, const void* tree_nodes,
                              int32_t* oct_start_end /*[R,2]*/, int32_t* oct_idx /*[R*max_hits]*/,
                              float* oct_near_far /*[R*max_hits,2]*/, int32_t* total /*[1]*/,
                              int32_t* oct_trans /*[R*max_hits] or NULL: trans_idx of every listed leaf*/,
                              const void* child_blocks /*or NULL*/);
/* The same walk with the records of every node that HAS a child (the only ones a walk expands) copied into LDS when a block
 * starts: interior_nodes[r] = index of the r-th such node in index order, rank_of[node] = its r (both derived from the node
 * array; they change only when child indices do, i.e. with f2n_oct_build_child_blocks).  For trees of up to
 * f2n_oct_lds_max_interior() such nodes (F2N_ERR_UNSUPPORTED beyond).  Output bit-identical to f2n_oct_intersect_strided; the
 * point is latency: the reference's one-thread-per-ray DFS (PersSampler.cu:53-152) and the walk above are chains of dependent
 * reads, which take ~6x longer when the kernel runs underneath a kernel that saturates the L2s (as the prefetched sampling of
 * the next batch does, under the hash gather). */
int f2n_oct_lds_max_interior(void);
int f2n_oct_intersect_strided_lds(void* stream, int n_rays, int max_hits, const uint8_t* search_order, const float* rays_o,
                                  const float* rays_d, float near_, float far_, const void* tree_nodes,
                                  int32_t* oct_start_end /*[R,2]*/, int32_t* oct_idx /*[R*max_hits]*/,
                                  float* oct_near_far /*[R*max_hits,2]*/, int32_t* total /*[1]*/,
                                  int32_t* oct_trans /*[R*max_hits] or NULL*/, const void* child_blocks,
                                  const int32_t* interior_nodes /*[n_interior]*/, const int32_t* rank_of /*[n_nodes]*/,
                                  int n_interior);


/* Optional acceleration structure for the three intersection entry points: child_blocks [n_nodes][8] x 32 B, entry
 * [u][c] = {center xyz, side_len, child index (-1: none), child's trans_idx, child has children, pad} of child slot c of
 * node u.  With it, expanding a node is one coalesced 256-byte read instead of the reference's dependent pair
 * "childs[] of the node, then the child nodes" (PersSampler.cu:93-120); results are identical.  Rebuild after every
 * host-side change of the tree; f2n_oct_update_stats keeps the trans_idx copies current when given the pointer. */
int f2n_oct_build_child_blocks(void* stream, int n_nodes, const void* tree_nodes, void* child_blocks);

/* GetVisiCams (PtsSampler/PersSampler.cpp:27-66) for n_boxes candidate octree nodes at once:
 * visible[b, c] = 1 iff any ray of camera c's res_h x res_w pixel-grid bundle (pixel centres pix_i [res_h] rows,
 * pix_j [res_w] columns; direction ((j-cx)/fx, -(i-cy)/fy, -1) rotated by c2w[c]) hits box b = (centre xyz, side)
 * within the camera's [near, far] bounds.  boxes [n_boxes,4], c2w [n_cams,3,4], bounds [n_cams,2]. */
int f2n_oct_visible_cams(void* stream, int n_boxes, int n_cams, const float* boxes, const float* c2w,
                         const float* bounds, float fx, float fy, float cx, float cy, int res_h, int res_w,
                         const float* pix_i, const float* pix_j, uint8_t* visible /*[n_boxes,n_cams]*/);

/* The march noise of PersSampler.cu:372-381 from uniform draws u in [0,1): out = ((u - 0.5) + 1) * fineness, in that
 * fp32 order (the reference: three ATen launches). */
int f2n_march_noise(void* stream, int n, const float* u, float fineness, float* out);

/* RayMarchKernel<false> (PersSampler.cu:189-314, launched :383-393).  noise has
 * F2N_MAX_SAMPLE_PER_RAY + n_rays + 10 floats, already multiplied by ray_march_fineness (:372-381), and is
 * indexed [ray + k] exactly as in the reference (:203,:266). */
int f2n_ray_march_count(void* stream, int n_rays, float sample_l, int scale_by_dis, const float* rays_o,
                        const float* rays_d, const float* noise, const int32_t* oct_start_end,
                        const int32_t* oct_idx, const float* oct_near_far, const void* tree_nodes,
                        const void* transes, int32_t* pts_counts /*[R]*/);

/* RayMarchKernel<true> (PersSampler.cu:407-423).  Outputs are the SampleResultFlex tensors
 * (PtsSampler/PtsSampler.h:13-22): pts = WARPED coordinates, dirs = unit world direction, dt = warped-space
 * step, t = world distance, anchors[:,0] = trans_idx, anchors[:,1] = leaf node index, anchors[:,2] = 0. */
int f2n_ray_march_fill(void* stream, int n_rays, float sample_l, int scale_by_dis, const float* rays_o,
                       const float* rays_d, const float* noise, const int32_t* oct_start_end,
                       const int32_t* oct_idx, const float* oct_near_far, const void* tree_nodes,
                       const void* transes, const int32_t* pts_start_end /*[R,2]*/, float* pts /*[N,3]*/,
                       float* dirs /*[N,3]*/, float* dt /*[N]*/, float* t /*[N]*/, int32_t* anchors /*[N,3]*/,
                       float* first_oct_dis /*[R]*/);

/* Single-pass variant of count + scan + fill: ONE march writes every ray's samples into its fixed-stride slot
 * [r*F2N_MAX_SAMPLE_PER_RAY, ...) of s_pts [R*1024,3], s_dt / s_t [R*1024], s_anchors [R*1024,2] = (trans_idx, node)
 * and its sample count into pts_counts[r]; after f2n_segment_scan(pts_counts), f2n_pack_samples copies the filled
 * prefixes into the ray-ordered compact SampleResultFlex arrays (dirs come from rays_d, anchors[:,2] = 0).
 * Per-ray contents are identical to the count/fill pair (same march, executed once instead of twice); the slot
 * buffers are scratch of which only the filled prefixes are ever touched. */
int f2n_ray_march_strided(void* stream, int n_rays, float sample_l, int scale_by_dis, const float* rays_o,
                          const float* rays_d, const float* noise, const int32_t* oct_start_end, const int32_t* oct_idx,
                          const float* oct_near_far, const void* tree_nodes, const void* transes,
                          int32_t* pts_counts /*[R]*/, float* s_pts, float* s_dt, float* s_t, int32_t* s_anchors,
                          float* first_oct_dis /*[R]*/,
                          const int32_t* oct_trans /*NULL, or f2n_oct_intersect_strided's: spares a node read per leaf*/);
/* s_pts may be NULL in both calls: the march then skips the warped point (one division and three reductions less on its
 * sequential path) and f2n_pack_samples computes pts = warp(o + d*t) for all samples in parallel -- same expressions,
 * same bits (PersSampler.cu:155-169); rays_o and transes are only read in that case. */
int f2n_pack_samples(void* stream, int n_rays, const int32_t* pts_start_end /*[R,2]*/, const float* rays_o,
                     const float* rays_d, const void* transes, const float* s_pts, const float* s_dt, const float* s_t,
                     const int32_t* s_anchors, float* pts /*[N,3]*/, float* dirs /*[N,3]*/, float* dt /*[N]*/,
                     float* t /*[N]*/, int32_t* anchors /*[N,3]*/);

/* GetEdgeSamplesKernel (PersSampler.cu:436-452).  edge_idx/edge_coords are the random draws of :456-457. */
int f2n_edge_samples(void* stream, int n_pts, const void* edge_pool, const void* transes, const int32_t* edge_idx,
                     const float* edge_coords /*[n,2]*/, float* out_pts /*[n,2,3]*/, int32_t* out_idx /*[n,2]*/);
/* The same with (a) the draws optionally given as u01 [n,3] uniform in [0,1) -- idx = min(floor(u0 * n_edges), n_edges - 1),
 * coords = 2 u - 1: one random launch for :456-457 instead of two (edge_idx / edge_coords are then ignored, may be NULL) --,
 * (b) a stride for the index output (3: the transform column of an anchors array [.,3]) and (c) an optional second
 * destination (out_pts2 / out_idx2 both NULL or both given): a streaming training step appends the edge samples to the
 * sampler's arrays so that the density pre-pass gathers their hash features too, and heads the grad pass's arrays with them. */
int f2n_edge_samples_ex(void* stream, int n_pts, const void* edge_pool, int n_edges, const void* transes, const int32_t* edge_idx,
                        const float* edge_coords, const float* u01, float* out_pts, int32_t* out_idx, int idx_stride,
                        float* out_pts2, int32_t* out_idx2, int idx_stride2);

/* MarkVistNodeKernel (PersSampler.cu:475-526).  oct node index of sample i = anchors[i*anchor_stride + 1].
 * w_adder/a_adder must be pre-filled with -1, mark with 0 (:555-557); visit_cnt is persistent state. */
int f2n_oct_mark_visit(void* stream, int n_rays, int n_nodes, const int32_t* pts_start_end, const int32_t* anchors,
                       int anchor_stride, const float* weights, const float* alphas, int32_t* w_adder,
                       int32_t* a_adder, int32_t* mark, int32_t* visit_cnt);

/* The integer stat update of UpdateOctNodes (PersSampler.cu:579-593) fused with MarkInvalidNodes
 * (:528-534, :595-603): stats = clamp(max(stats, pos vote) + visited negative vote, -100, 2^20);
 * trans_idx = -1 where either stat < 0.  reset_votes != 0: the three vote buffers are re-initialised after use
 * (adders = -1, mark = 0: what the reference re-creates with torch::full / zeros every iteration, :555-557), so a
 * caller can keep one persistent buffer. */
int f2n_oct_update_stats(void* stream, int n_nodes, int32_t* w_adder, int32_t* a_adder, int32_t* mark, int32_t* w_stats,
                         int32_t* a_stats, void* tree_nodes, void* child_blocks /*or NULL*/, int reset_votes);

/* ---- Speculative sampling (ABI v8) -------------------------------------------------------------------------------------
 * The reference samples a batch AFTER the previous iteration's UpdateOctNodes (ExpRunner.cpp:88-93 -> Renderer.cpp:100 ->
 * PersSampler.cu:317, behind :536-615 of the iteration before): intersection and march of batch k+1 wait for the density
 * pre-pass of batch k.  Outside the ProcOctree iterations the only thing that update changes in the tree is trans_idx -> -1 of
 * the leaves that die (MarkInvalidNodes, :528-534), so batch k+1 can be sampled EARLY, against the tree as it stands, and
 * repaired afterwards: a ray whose leaf list holds no node that died since is already exact (see oct_intersect_coop_kernel
 * MODE 3 in csrc/sampler.hip for the argument), the others are walked and marched again into their fixed-stride slots.
 *   f2n_oct_update_stats_ex   as f2n_oct_update_stats; a leaf that dies in this call gets died_at[node] = epoch and
 *                             death_epoch[0] = epoch (both or neither may be NULL; epochs must increase from call to call)
 *   f2n_oct_intersect_repair  on the outputs of f2n_oct_intersect_strided computed while / before the updates of epochs
 *                             >= spec_epoch ran: rays whose list holds a node with died_at >= spec_epoch (or is at the
 *                             max_hits cap) are walked again on the updated tree, total[0] is adjusted, repair_flags[r] = 1 for
 *                             those rays and 0 for all others, n_repaired[0] (or NULL) += their number.  Returns immediately on
 *                             the device when death_epoch[0] < spec_epoch (then repair_flags is NOT written).
 *   f2n_ray_march_repair      f2n_ray_march_strided for the flagged rays only (same early exit).
 *   f2n_pack_samples_repair   f2n_pack_samples once more over the whole batch, but only when a leaf died since (same early exit):
 *                             a batch may be scanned and packed OPTIMISTICALLY right behind its speculative march -- long before
 *                             the stat update, in a stretch of the step where the memory system has room -- and is scanned again
 *                             and conditionally packed again behind the two repair calls.
 * After both, slots / counts / first_oct_dis are bit-identical to a fresh f2n_oct_intersect_strided + f2n_ray_march_strided on
 * the updated tree (tests/test_gpu_parity.py::test_speculative_sampling_repair). */
int f2n_oct_update_stats_ex(void* stream, int n_nodes, int32_t* w_adder, int32_t* a_adder, int32_t* mark, int32_t* w_stats,
                            int32_t* a_stats, void* tree_nodes, void* child_blocks /*or NULL*/, int reset_votes,
                            int32_t* died_at /*[n_nodes] or NULL*/, int epoch, int32_t* death_epoch /*[1] or NULL*/,
                            int32_t* death_epoch_host /*[1] device-accessible HOST word or NULL: also receives the epoch of a
                            death -- a hint the host may read without synchronising (whether speculating pays right now)*/);
/* f2n_oct_update_stats_ex and f2n_segment_scan_ex in ONE launch (round 5): the stat update of a streaming training step
 * (PersSampler.cu:579-593, :528-534) and the scan of the rays' surviving-sample counts (FilterIdxBounds, Renderer.cu:20-50) are
 * independent and used to be two dependent launches of the step's main queue.  Same results as the two calls. */
int f2n_oct_update_stats_scan(void* stream, int n_nodes, int32_t* w_adder, int32_t* a_adder, int32_t* mark, int32_t* w_stats,
                              int32_t* a_stats, void* tree_nodes, void* child_blocks, int reset_votes, int32_t* died_at, int epoch,
                              int32_t* death_epoch, int32_t* death_epoch_host, int n, const int32_t* counts, int32_t* start_end /*[n,2]*/,
                              int32_t* total /*[1]*/, int32_t* mirror, const int32_t* also, int n_also);
int f2n_oct_intersect_repair(void* stream, int n_rays, int max_hits, const uint8_t* search_order, const float* rays_o,
                             const float* rays_d, float near_, float far_, const void* tree_nodes, int32_t* oct_start_end,
                             int32_t* oct_idx, float* oct_near_far, int32_t* total, int32_t* oct_trans, const void* child_blocks,
                             const int32_t* died_at, int spec_epoch, const int32_t* death_epoch, int32_t* repair_flags /*[R]*/,
                             int32_t* n_repaired /*[1] or NULL*/);
int f2n_ray_march_repair(void* stream, int n_rays, float sample_l, int scale_by_dis, const float* rays_o, const float* rays_d,
                         const float* noise, const int32_t* oct_start_end, const int32_t* oct_idx, const float* oct_near_far,
                         const void* tree_nodes, const void* transes, int32_t* pts_counts, float* s_pts, float* s_dt, float* s_t,
                         int32_t* s_anchors, float* first_oct_dis, const int32_t* oct_trans, const int32_t* repair_flags,
                         const int32_t* death_epoch, int spec_epoch);
int f2n_pack_samples_repair(void* stream, int n_rays, const int32_t* pts_start_end, const float* rays_o, const float* rays_d,
                            const void* transes, const float* s_pts, const float* s_dt, const float* s_t, const int32_t* s_anchors,
                            float* pts, float* dirs, float* dt, float* t, int32_t* anchors, const int32_t* death_epoch /*[1]*/,
                            int spec_epoch);

/* ---- Tail repair of a speculatively sampled batch (ABI v10) -------------------------------------------------------------
 * The repair above walks and marches an invalidated ray again from its origin: as latency-bound as the sampler itself
 * (the longest invalidated ray), and it sits on the step's critical cycle.  Neither is necessary.  (1) The walk reads trans_idx
 * only to decide whether a leaf it has reached is listed, so the list a fresh walk produces is the old list minus its dead
 * entries (unless the old list was cut at max_hits).  (2) A march iteration looks at list entries only when it crosses out of
 * its current leaf, so every iteration before the one that first reached the first removed entry is untouched.
 *   f2n_ray_march_strided_rec  f2n_ray_march_strided that also records, per list entry it crosses into or past, the state the
 *                              iteration started from -- leaf_state[ray * max_hits + entry] = {bits of t, samples emitted |
 *                              list position << 11 | first-point flag << 22} -- and reached[ray] = the last list position it
 *                              looked at.  max_hits <= 2048.
 *   f2n_oct_list_repair        removes the entries whose node has died_at >= spec_epoch from every list IN PLACE (order, near /
 *                              far, trans kept), adjusts oct_start_end / total[0]; repair_from[ray] = position of the first
 *                              removed entry if the march had reached it, F2N_REPAIR_NONE (-1) if the ray needs no new march,
 *                              F2N_REPAIR_FULL (-2) if the list was cut at max_hits and lost an entry (n_full[0] += 1; the list is
 *                              left as it was).  Same early exit as the calls above (repair_from is then NOT written).
 *   f2n_oct_intersect_repair_flagged  walks the F2N_REPAIR_FULL rays again (returns at once when n_full[0] == 0) and sets their
 *                              repair_from to 0.
 *   f2n_ray_march_repair_tail  resumes the march of every ray with repair_from >= 0 from the state recorded at that entry (0: from
 *                              the origin) on the repaired list, recording again.
 * Result: bit-identical to a fresh f2n_oct_intersect_strided + f2n_ray_march_strided on the updated tree
 * (tests/test_gpu_scale.py::test_speculative_tail_repair). */
#define F2N_REPAIR_NONE (-1)
#define F2N_REPAIR_FULL (-2)
int f2n_ray_march_strided_rec(void* stream, int n_rays, int max_hits, float sample_l, int scale_by_dis, const float* rays_o,
                              const float* rays_d, const float* noise, const int32_t* oct_start_end, const int32_t* oct_idx,
                              const float* oct_near_far, const void* tree_nodes, const void* transes, int32_t* pts_counts, float* s_pts,
                              float* s_dt, float* s_t, int32_t* s_anchors, float* first_oct_dis, const int32_t* oct_trans,
                              void* leaf_state /*[R * max_hits] 8-byte records*/, int32_t* reached /*[R]*/);
/* f2n_ray_march_strided[_rec] on a small persistent grid: n_blocks persistent WAVES (in workgroups of block_waves waves, 1..16:
 * ABI v13 -- a workgroup's waves land on one CU, so 512 waves in blocks of 8 leave three quarters of the chip's CUs to the
 * register-hungry kernels of the main queue instead of parking one or two march waves on every CU) take groups of four rays off counter[0], rays
 * ordered by leaf count, longest first (order[R]: scratch, filled here; counter[1]: scratch, zeroed here).  For batches that are
 * sampled well ahead of their use (two-deep pipeline): a few hundred resident waves instead of R / 4, so that the occupancy-bound
 * kernels the march runs underneath keep their wave slots.  leaf_state / reached both NULL: no recording.  Same slots, same
 * bits (tests/test_gpu_scale.py::test_persistent_march). */
int f2n_ray_march_persistent(void* stream, int n_rays, int max_hits, int n_blocks, int block_waves, float sample_l, int scale_by_dis, const float* rays_o,
                             const float* rays_d, const float* noise, const int32_t* oct_start_end, const int32_t* oct_idx,
                             const float* oct_near_far, const void* tree_nodes, const void* transes, int32_t* pts_counts, float* s_pts,
                             float* s_dt, float* s_t, int32_t* s_anchors, float* first_oct_dis, const int32_t* oct_trans,
                             void* leaf_state /*or NULL*/, int32_t* reached /*or NULL*/, int32_t* order /*[R]*/, int32_t* counter /*[1]*/);
int f2n_oct_list_repair(void* stream, int n_rays, int max_hits, int32_t* oct_start_end, int32_t* oct_idx, float* oct_near_far,
                        int32_t* oct_trans /*or NULL*/, int32_t* total, const int32_t* died_at, int spec_epoch,
                        const int32_t* death_epoch, const int32_t* reached, int32_t* repair_from /*[R]*/,
                        int32_t* n_repaired /*[1] or NULL*/, int32_t* n_full /*[1], zeroed by the caller*/);
int f2n_oct_intersect_repair_flagged(void* stream, int n_rays, int max_hits, const uint8_t* search_order, const float* rays_o,
                                     const float* rays_d, float near_, float far_, const void* tree_nodes, int32_t* oct_start_end,
                                     int32_t* oct_idx, float* oct_near_far, int32_t* total, int32_t* oct_trans,
                                     const void* child_blocks, const int32_t* death_epoch, int spec_epoch, int32_t* repair_from,
                                     const int32_t* n_full);
int f2n_ray_march_repair_tail(void* stream, int n_rays, int max_hits, float sample_l, int scale_by_dis, const float* rays_o,
                              const float* rays_d, const float* noise, const int32_t* oct_start_end, const int32_t* oct_idx,
                              const float* oct_near_far, const void* tree_nodes, const void* transes, int32_t* pts_counts, float* s_pts,
                              float* s_dt, float* s_t, int32_t* s_anchors, float* first_oct_dis, const int32_t* oct_trans,
                              void* leaf_state, int32_t* reached, const int32_t* repair_from, const int32_t* death_epoch,
                              int spec_epoch);

/* MarkInvisibleNodesKernel (PersSampler.cu:618-680). */
int f2n_oct_mark_invisible(void* stream, int n_nodes, int n_cams, void* tree_nodes, const float* intris /*[C,3,3]*/,
                           const float* w2cs /*[C,3,4]*/, const float* bounds /*[C,2]*/);

/* ---------------------------------------------------------------------------------------------------
 * Hash grid -- replaces Hash3DAnchoredFunction::forward/backward (Field/Hash3DAnchored.cu:11-233).
 * `table_h` is the binary16 table [pool,2]; level l lives at table_h + local_idx[l] HALVES and is
 * addressed as pos*2+k with pos < local_size[l] (the 50 % level-overlap quirk of :37/:74-77 is kept).
 * level_scale[16] are the per-level multipliers exp2f(7*l/15+3) (:28) supplied by the host so that both
 * sides of a parity test use identical bits.  If pts_are_warped != 0 the kernel applies the
 * ((p + 1) * .5) of Hash3DAnchored.cpp:91 itself.  volume index of point i = volume_idx[i*vol_stride].
 * ------------------------------------------------------------------------------------------------- */
int f2n_hash_fwd(void* stream, int n, int n_volumes, const void* table_h, const int32_t* prim_pool /*[16,V,3]*/,
                 const int32_t* local_idx /*[16]*/, const int32_t* local_size /*[16]*/,
                 const float* bias_pool /*[16*V,3]*/, const float* level_scale /*[16]*/, const float* pts /*[n,3]*/,
                 int pts_are_warped, const int32_t* volume_idx, int vol_stride, void* out_h /*[n,32] h16*/);

/* grad_in_h: dL/dfeat already scaled by 128 and rounded to h16 (Hash3DAnchored.cu:220).  grad_table_h is
 * ACCUMULATED into (the reference's half2 atomicAdd, :151) and must be zeroed by the caller (:222).  The /128 and
 * fp32 widening of :232 are left to the optimiser step (f2n_adam_step_h16grad).
 * level_entries: 0, or the HOST-side statement that the table has the reference's layout (Hash3DAnchored.cpp:60-70):
 * local_size[l] = level_entries (a power of two) and local_idx[l] = l * level_entries halves for every level
 * (the device arrays cannot be read without a sync).  It lets large batches use the owner-binned scatter: records
 * binned per 4096-entry table slice, summed in LDS in fp64 by one owner block per slice and added to the table with
 * plain stores -- no global atomics (measured 3x faster at 8e5 samples).  0 = always packed-h16 global atomics,
 * any layout. */
int f2n_hash_bwd(void* stream, int n, int n_volumes, const int32_t* prim_pool, const int32_t* local_idx,
                 const int32_t* local_size, const float* bias_pool, const float* level_scale, const float* pts,
                 int pts_are_warped, const int32_t* volume_idx, int vol_stride, const void* grad_in_h /*[n,32]*/,
                 void* grad_table_h, int level_entries);

/* ---------------------------------------------------------------------------------------------------
 * Fully-fused MLP -- replaces the tcnn::cpp::Module surface used by Field/TCNNWP.cpp:94-97,150-154,
 * 217-227 ("FullyFusedMLP", ReLU, no output activation, no bias).  Supported shapes: d_in = 32,
 * d_hidden = 64, n_hidden in {1,2}, d_out <= 16 (padded to 16) -- the two networks of the reference
 * configs.  Parameter layout (fp32 master and h16 working copy alike): layers first->last, each
 * [n_out, n_in] row-major, last layer has 16 rows.  The h16 parameter block handed to the *_bwd entry points must be
 * 16-byte aligned (F2N_ERR_INVALID_ARG otherwise).
 * ------------------------------------------------------------------------------------------------- */
int f2n_mlp_n_params(int d_in, int d_hidden, int n_hidden);               /* Module::n_params() */
/* Module::initialize_params(seed, float*): Xavier-uniform from a counter-based generator (tcnn's pcg32
 * stream cannot be reproduced; weights are exchanged as flat fp32 arrays instead). */
int f2n_mlp_init_params(void* stream, uint64_t seed, int d_in, int d_hidden, int n_hidden, float* params_f32);
int f2n_params_to_h16(void* stream, int n, const float* params_f32, void* params_h); /* TCNNWP.cpp:111 */
/* Module::inference / forward: x is fp32 [n,32] (tcnn input precision), out is h16 [n,16]
 * (output_precision()).  No activations are stored: the backward recomputes them on the matrix cores. */
int f2n_mlp_fwd(void* stream, int n, int d_in, int d_hidden, int n_hidden, const void* params_h, const float* x,
                void* out_h);
/* Module::backward: dy fp32 [n,16] is multiplied by loss_scale and rounded to h16 (TCNNWP.cpp:174);
 * dparams_f32 [n_params] is ACCUMULATED (fp32 atomics) in the SCALED domain -- divide by loss_scale
 * afterwards (:232); dx_f32 (may be NULL) receives dL/dx / loss_scale (:231). */
int f2n_mlp_bwd(void* stream, int n, int d_in, int d_hidden, int n_hidden, float loss_scale, const void* params_h,
                const float* x, const float* dy, float* dparams_f32_scaled, float* dx_f32);

/* ---------------------------------------------------------------------------------------------------
 * Fused field = hash gather + density MLP (Hash3DAnchored::AnchoredQuery, Field/Hash3DAnchored.cpp:84-99).
 * Features never leave the register file between the gather and the matrix cores.
 *   out_feat_f32 [n,16]   (may be NULL) the AnchoredQuery result (h16 values widened, TCNNWP.cpp:112)
 *   out_f0       [n]      (may be NULL) channel 0 only: the density pre-activation for the no-grad
 *                         pre-pass of Renderer::Render (Renderer/Renderer.cpp:105-137)
 *   save_x_h     [n,32]   (may be NULL) the h16 hash features, kept for f2n_field_bwd
 * ------------------------------------------------------------------------------------------------- */
int f2n_field_fwd(void* stream, int n, int n_volumes, const void* table_h, const int32_t* prim_pool,
                  const int32_t* local_idx, const int32_t* local_size, const float* bias_pool,
                  const float* level_scale, const float* pts_warped, const int32_t* volume_idx, int vol_stride,
                  const void* mlp_params_h, float* out_feat_f32, float* out_f0, void* save_x_h);
/* f2n_field_fwd's one-kernel path (hash gather -> MLP inside one wave, features never in HBM) at ANY batch size: the A/B
 * comparator of the XCD-partitioned gather + plane-fed MLP that f2n_field_fwd uses for large batches.  Same results. */
int f2n_field_fwd_fused(void* stream, int n, int n_volumes, const void* table_h, const int32_t* prim_pool, const int32_t* local_idx,
                        const int32_t* local_size, const float* bias_pool, const float* level_scale, const float* pts_warped,
                        const int32_t* volume_idx, int vol_stride, const void* mlp_params_h, float* out_feat_f32 /*or NULL*/,
                        float* out_f0 /*or NULL*/, void* save_x_h /*or NULL*/);

/* The two halves of f2n_field_fwd's large-batch path, callable on their own.
 * f2n_hash_gather_planes: the 16-level gather with an XCD-aware partition -- workgroup b serves levels (2p, 2p+1),
 * p = b % 8, so that each of the 8 private 4 MiB L2s of an MI355X only ever sees a 3 MiB slice of the table
 * (~2.6x the rate of one wave gathering all 16 levels).  Output: h16 "planes" [8][n][4], plane p = features
 * 4p..4p+3 (levels 2p, 2p+1) of every sample; numerically the same features as f2n_hash_fwd (same fp32 order).
 * f2n_field_mlp_planes: the density MLP on such planes; outputs as f2n_field_fwd. */
int f2n_hash_gather_planes(void* stream, int n, int n_volumes, const void* table_h, const int32_t* prim_pool,
                           const int32_t* local_idx, const int32_t* local_size, const float* bias_pool,
                           const float* level_scale, const float* pts, int pts_are_warped, const int32_t* volume_idx,
                           int vol_stride, void* planes_h /*[8,n,4] h16*/);
/* The same gather with run combining and a cost-balanced split (ABI v6).  step01 = typical distance of consecutive
 * samples of a ray in the [0,1] hash space (the march's warped-space step / 2: sample_l * fineness / 2,
 * PersSampler.cu:262-270 and Hash3DAnchored.cpp:91); level_scale_host = the 16 level scales as a HOST array.  Samples
 * must be ray-ordered (as PersSampler::GetSamples emits them).  Consecutive samples in one cell of a level share their
 * eight table reads; the level pairs, which then differ in cost by up to 10x, are spread over the XCDs by expected cost
 * instead of one pair per XCD.  Bit-identical planes; step01 <= 0 or level_scale_host == NULL: exactly
 * f2n_hash_gather_planes. */
int f2n_hash_gather_planes_balanced(void* stream, int n, int n_volumes, const void* table_h, const int32_t* prim_pool,
                                    const int32_t* local_idx, const int32_t* local_size, const float* bias_pool,
                                    const float* level_scale, const float* pts, int pts_are_warped, const int32_t* volume_idx,
                                    int vol_stride, void* planes_h /*[8,n,4] h16*/, float step01, const float* level_scale_host);
/* Introspection (host only, no device work): the split f2n_hash_gather_planes_balanced would use for n_tiles tiles of 256
 * samples.  out [8][1 + 3*8] int32: per XCD the number of segments, then (level pair, first tile, tile count) per
 * segment (-1, 0, 0 for unused slots); cost8_out [8] (may be NULL): the modelled cost of one tile of each level pair. */
int f2n_gather_plan_query(int n_tiles, float step01, const float* level_scale_host, int32_t* out, float* cost8_out);
/* f2n_hash_gather_planes for tables that have left the L2s (Field/Hash3DAnchored.cu:11-79 at confs/wanjinyou_big.yaml's sizes and
 * beyond; level_entries = local_size[l] = a power of two, 8 * 8192 ... 2^23): level pairs >= first_binned_pair (0 ... 8) go through
 * a slice-binned pipeline -- requests binned by 8192-entry table slice per 1536-sample chunk, every slice read once into LDS and
 * its requests answered in place, values blended per sample in the reference's order -- instead of one 128-byte fabric line per
 * 4-byte read; pairs below it keep the partitioned gather.  Planes bit-identical to f2n_hash_gather_planes.
 * F2N_ERR_UNSUPPORTED: level_entries outside that range or n > 1536 * 1024.  Scratch: library workspace, 56 B per sample and
 * binned level (~0.65 GB at 8e5 samples and 14 levels). */
int f2n_hash_gather_planes_binned(void* stream, int n, int n_volumes, const void* table_h, const int32_t* prim_pool,
                                  const int32_t* local_idx, const int32_t* local_size, const float* bias_pool,
                                  const float* level_scale, const float* pts, int pts_are_warped, const int32_t* volume_idx,
                                  int vol_stride, void* planes_h, int level_entries, int first_binned_pair);
/* ... and the kernel variant it would launch for these sizes (host only, ABI v8): bit 0 = hash constants staged in LDS
 * (2 * n_volumes * 24 B <= 20000 and n >= 16384), bit 1 = run combining + balanced split (the cost model predicts a balanced
 * share below 0.8 x the costliest level pair).  Negative = error.  What the parity tests assert before they claim to have
 * exercised a variant. */
int f2n_hash_gather_variant(int n, int n_volumes, float step01, const float* level_scale_host);
int f2n_field_mlp_planes(void* stream, int n, const void* planes_h, const void* mlp_params_h, float* out_feat_f32,
                         float* out_f0, void* save_x_h);

/* AnchoredQuery for samples whose hash features are already known: Renderer::Render queries the field twice per
 * step with an unchanged table -- the no-grad density pre-pass over every marched sample (Renderer.cpp:115-123)
 * and the grad pass over the survivors (:152-166) -- so the 128 gathers per surviving sample of the second query
 * are a pure recomputation.  x_cache_h [n_cache,32] is the save_x_h of the pre-pass; sample i of this call takes
 * row src_rows[i] (NULL = row i).  Outputs as f2n_field_fwd: bit-identical to it by construction (same h16
 * features through the same MLP kernel).  save_x_h [n,32] (may be NULL) receives the gathered rows in call order,
 * ready for f2n_field_bwd. */
int f2n_field_fwd_cached(void* stream, int n, int n_cache, const int32_t* src_rows, const void* x_cache_h,
                         const void* mlp_params_h, float* out_feat_f32, float* out_f0, void* save_x_h);

/* Backward of the fused field: MLP backward (dparams accumulated, scaled domain) chained into the hash scatter.
 * dfeat fp32 [n,16].  level_entries as in f2n_hash_bwd (0: dL/dx goes straight from registers into global atomics;
 * > 0 and a large batch: through 64 B/sample of f16 workspace into the owner-binned scatter). */
int f2n_field_bwd(void* stream, int n, int n_volumes, const int32_t* prim_pool, const int32_t* local_idx,
                  const int32_t* local_size, const float* bias_pool, const float* level_scale,
                  const float* pts_warped, const int32_t* volume_idx, int vol_stride, const void* mlp_params_h,
                  const void* saved_x_h, const float* dfeat, float loss_scale, float* dparams_f32_scaled,
                  void* grad_table_h, int level_entries);

/* ---------------------------------------------------------------------------------------------------
 * Shader -- replaces SHShader::Query (Shader/SHShader.cpp:23-29) and SHKenerl (Shader/SHShader.cu:10-118).
 * ------------------------------------------------------------------------------------------------- */
int f2n_sh_encode(void* stream, int n, int degree /*1..8*/, const float* dirs /*[n,3]*/, float* out /*[n,degree^2]*/);

/* ScatterIdxKernal (Utils/CustomOps/Scatter.cu:110-120): out[i] = ray_val[r] for every sample i of ray r. */
int f2n_scatter_idx(void* stream, int n_rays, const int32_t* start_end, const int32_t* ray_val, int32_t* out /*[n]*/);

/* Fused colour path of Renderer::Render (Renderer/Renderer.cpp:181-189):
 *   shading_feat = [1 | feat[:,1:16]] (+ app_emb[sample_emb_idx[i]] when app_emb != NULL, Scatter.cu:10-18),
 *   input = [shading_feat | SH4(dir)] -> colour MLP 32->64->64->16 -> rgb = (1+2e-3)/(1+exp(-o)) - 1e-3.
 * sample_emb_idx [n] is the ScatterIdx result (image index per sample), only read when app_emb != NULL.
 * save_x_h [n,32] (may be NULL) keeps the h16 MLP input for the backward. */
int f2n_shade_fwd(void* stream, int n, const float* feat /*[n,16]*/, const float* dirs /*[n,3]*/,
                  const float* app_emb /*[n_img,16] or NULL*/, const int32_t* sample_emb_idx /*[n] or NULL*/,
                  const void* mlp_params_h, float* rgb /*[n,3]*/, void* save_x_h);

/* drgb [n,3] -> dfeat[:,1:16] written; column 0 belongs to the density path: left untouched when df0 is NULL, or
 * filled from the compact array df0 [n] (f2n_composite_bwd with df0_stride 1) so that every dfeat row is written once,
 * as whole cache lines.  dparams accumulated (scaled domain), dapp_emb [n_img,16] accumulated UNSCALED or NULL.
 * The network output needed for the sigmoid derivative is recomputed from saved_x_h on the matrix cores.
 * n_emb <= 480: the embedding gradient is accumulated per block in LDS and reduced (no same-address global atomics);
 * larger image counts fall back to global atomics like the reference's ScatterAddFuncBackward (Scatter.cu:20-40).
 * sample_emb_idx values outside [0, n_emb) contribute nothing (f2n_shade_fwd trusts its indices: it has no n_emb). */
int f2n_shade_bwd(void* stream, int n, const float* drgb, const int32_t* sample_emb_idx, const void* mlp_params_h,
                  const void* saved_x_h, float loss_scale, float* dfeat /*[n,16]*/, float* dparams_f32_scaled,
                  float* dapp_emb /*[n_emb,16] or NULL*/, int n_emb, const float* df0 /*[n] or NULL*/);

/* ---------------------------------------------------------------------------------------------------
 * PersOctree::ProcOctree on the device (PtsSampler/PersSampler.cpp:120-330; ABI v6): the reference copies the node array
 * to the host, edits it with index-ordered loops and copies it back; these four calls produce the same arrays without
 * leaving HBM.  All buffers are caller-allocated; node arrays are TreeNode[] (64 B).
 *   f2n_oct_prune_compress  compact loop + path compression (:139-215) on a copy: out_nodes [n] = edited nodes in the OLD
 *                           numbering, keep [n] = 1 for the nodes that survive (:219-224).  work_nodes [n], alive [n],
 *                           n_child [n] are scratch.
 *   f2n_oct_gather_kept     renumbering (:226-252): new_pos = f2n_segment_scan(keep) start_end layout [n,2]; gathers nodes
 *                           (parent / child indices rewritten), both statistics and the visit counts.
 *   f2n_oct_subtree_sizes + f2n_oct_subdivide   subdivision (:255-318): leaves with visit_cnt > 4 (or all: brute_force)
 *                           split into 8 children that inherit warp and statistics, the whole tree renumbered depth-first;
 *                           size[0] after the first call is the new node count (read it to allocate dst_*).
 * ------------------------------------------------------------------------------------------------- */
int f2n_oct_prune_compress(void* stream, int n_nodes, const void* tree_nodes, void* work_nodes, void* out_nodes, int32_t* alive,
                           int32_t* n_child, int32_t* keep);
int f2n_oct_gather_kept(void* stream, int n_nodes, const void* nodes, const int32_t* keep, const int32_t* new_pos,
                        const int32_t* w_stats, const int32_t* a_stats, const int32_t* visit_cnt, void* dst_nodes, int32_t* dst_w,
                        int32_t* dst_a, int32_t* dst_visit);
int f2n_oct_subtree_sizes(void* stream, int n_nodes, const void* nodes, const int32_t* visit_cnt, int brute_force, int32_t* depth,
                          int32_t* size);
int f2n_oct_subdivide(void* stream, int n_nodes, const void* nodes, const int32_t* visit_cnt, int brute_force, const int32_t* size,
                      const int32_t* w_stats, const int32_t* a_stats, int32_t* new_idx, void* dst_nodes, int32_t* dst_w, int32_t* dst_a);

/* ---------------------------------------------------------------------------------------------------
 * Device-side sample counts (ABI v6).  Renderer::Render learns the number of samples that survive the early stop from a
 * blocking read-back (Renderer.cpp:128-135: boolean-mask indexing) and only then launches the grad pass.  The _dyn entry
 * points take the count where it is produced: n_dev points at a DEVICE int32 (the `total` of f2n_segment_scan); the kernels
 * process min(n_max, *n_dev + n_off) rows, n_max sizes grids / workspaces / plane strides (buffers must hold n_max rows).
 * The host can therefore queue a whole training step without waiting for the device.  n_dev == NULL: exactly the plain
 * entry point with n = n_max.  Results for the rows processed are identical to the plain calls.
 * ------------------------------------------------------------------------------------------------- */
int f2n_field_fwd_cached_dyn(void* stream, int n_max, const int32_t* n_dev, int n_cache, const int32_t* src_rows,
                             const void* x_cache_h, const void* mlp_params_h, float* out_feat_f32, float* out_f0, void* save_x_h);
int f2n_field_bwd_dyn(void* stream, int n_max, const int32_t* n_dev, int n_off, int n_volumes, const int32_t* prim_pool,
                      const int32_t* local_idx, const int32_t* local_size, const float* bias_pool, const float* level_scale,
                      const float* pts_warped, const int32_t* volume_idx, int vol_stride, const void* mlp_params_h,
                      const void* saved_x_h, const float* dfeat, float loss_scale, float* dparams_f32_scaled, void* grad_table_h,
                      int level_entries, int defer_reduce);
int f2n_shade_fwd_dyn(void* stream, int n_max, const int32_t* n_dev, const float* feat, const float* dirs, const float* app_emb,
                      const int32_t* sample_emb_idx, const void* mlp_params_h, float* rgb, void* save_x_h);
/* f2n_field_fwd_cached + f2n_shade_fwd in one launch for the surviving samples of the grad pass (Renderer.cpp:152-189): the
 * field network's outputs go straight into the colour network's input fragment, `feat` [n,16] is never written.  Outputs:
 * out_f0 [n] (density pre-activation, for compositing), save_field_x_h / save_shade_x_h [n,32] (h16 inputs of the two
 * networks, for f2n_field_bwd / f2n_shade_bwd; either may be NULL), rgb [n,3].  Bit-identical to the two separate calls.
 * src_rows NULL: row i of x_cache_h.  n_dev as above (may be NULL). */
int f2n_field_shade_fwd_dyn(void* stream, int n_max, const int32_t* n_dev, const int32_t* src_rows, const void* x_cache_h,
                            const void* field_params_h, const float* dirs, const float* app_emb, const int32_t* sample_emb_idx,
                            const void* color_params_h, float* out_f0, void* save_field_x_h, void* save_shade_x_h, float* rgb);
/* ... plus n_extra rows that only go through the field MLP (x_extra_h [n_extra,32] -> feat_extra fp32 [n_extra,16], inputs
 * saved to save_x_extra_h or NULL): f2n_field_fwd_cached for the edge (TV) samples of Renderer.cpp:159-166 riding in the same
 * launch. */
int f2n_field_shade_fwd_extra(void* stream, int n_max, const int32_t* n_dev, const int32_t* src_rows, const void* x_cache_h,
                              const void* field_params_h, const float* dirs, const float* app_emb, const int32_t* sample_emb_idx,
                              const void* color_params_h, float* out_f0, void* save_field_x_h, void* save_shade_x_h, float* rgb,
                              int n_extra, const void* x_extra_h, float* feat_extra, void* save_x_extra_h);
int f2n_shade_bwd_dyn(void* stream, int n_max, const int32_t* n_dev, const float* drgb, const int32_t* sample_emb_idx,
                      const void* mlp_params_h, const void* saved_x_h, float loss_scale, float* dfeat, float* dparams_f32_scaled,
                      float* dapp_emb, int n_emb, const float* df0, int defer_reduce);
/* defer_reduce != 0 (f2n_shade_bwd_dyn, f2n_field_bwd_dyn): the per-block partial sums of the parameter gradients (and of the
 * appearance-embedding gradient) stay in the library's workspace; ONE later f2n_reduce_deferred(stream) folds everything
 * that was deferred on this device into the destinations named at the time (at most four pending reductions; same stream
 * rule as the workspace itself).  Saves two dependent launches per training step. */
int f2n_reduce_deferred(void* stream);
/* Drops every reduction registered on this device and not yet folded: call it at the start of a backward pass (the host's
 * ZeroGrad does), so that a step that failed between a deferring launch and f2n_reduce_deferred cannot leak its partial sums
 * into the next step's gradients.  No launch. */
int f2n_deferred_reset(void);

/* ---------------------------------------------------------------------------------------------------
 * Renderer -- replaces the per-ray glue of Renderer::Render (Renderer/Renderer.cpp:105-208), i.e.
 * TruncExp (CustomOps.cpp:9-18), FlexOps::Sum/AccumulateSum (FlexOps.cu:5-93), CountValidPts /
 * FilterIdxBounds (Renderer.cu:8-50), GradientScaling (CustomOps.cu:68-80).  One sequential left-to-right
 * walk per ray, as in the reference (the add order is part of the parity contract).
 * ------------------------------------------------------------------------------------------------- */

/* No-grad pre-pass (Renderer.cpp:115-137): sigma = exp(f0-3), sec = sigma*dt, alpha = 1-exp(-sec),
 * T = exp(-exclusive_cumsum(sec)), w = T*alpha, mask = T > 1e-4.  f0 of sample i = f0[i*f0_stride].
 * kept[r] = number of samples of ray r with mask set. */
int f2n_early_stop(void* stream, int n_rays, const int32_t* pts_start_end, const float* f0, int f0_stride,
                   const float* dt, float* weights /*[N]*/, float* alphas /*[N]*/, int32_t* mask /*[N]*/,
                   int32_t* kept /*[R]*/);
/* f2n_early_stop followed by f2n_oct_mark_visit (the occupancy votes of PersSampler.cu:475-526 over the weights / alphas the
 * early stop has just produced) in ONE launch: same outputs, bit for bit.  anchors: node index of sample i at
 * anchors[i*anchor_stride + 1]; vote buffers as f2n_oct_mark_visit expects them. */
int f2n_early_stop_votes(void* stream, int n_rays, const int32_t* pts_start_end, const float* f0, int f0_stride, const float* dt,
                         float* weights, float* alphas, int32_t* mask, int32_t* kept, int n_nodes, const int32_t* anchors,
                         int anchor_stride, int32_t* w_adder, int32_t* a_adder, int32_t* mark, int32_t* visit_cnt);

/* Compaction of the surviving samples (Renderer.cpp:128-135: the five index-gathers).  Sample order is
 * preserved; new_start_end comes from f2n_segment_scan(kept).  f2n_compact_samples_src: o_anchors may be NULL (the
 * compacted anchors are then not written: a streaming training step reads only o_vol of them). */
int f2n_compact_samples(void* stream, int n_rays, const int32_t* old_start_end, const int32_t* new_start_end,
                        const int32_t* mask, const float* pts, const float* dirs, const float* dt, const float* t,
                        const int32_t* anchors, float* o_pts, float* o_dirs, float* o_dt, float* o_t,
                        int32_t* o_anchors);
/* Same, and o_src[k] = index of surviving sample k in the uncompacted arrays (the row of the pre-pass feature
 * cache that f2n_field_fwd_cached reuses for it). */
int f2n_compact_samples_src(void* stream, int n_rays, const int32_t* old_start_end, const int32_t* new_start_end,
                            const int32_t* mask, const float* pts, const float* dirs, const float* dt, const float* t,
                            const int32_t* anchors, float* o_pts, float* o_dirs, float* o_dt, float* o_t,
                            int32_t* o_anchors, int32_t* o_src /*[M]*/,
                            int32_t* o_vol /*[M] or NULL: anchors[:,0] of the survivors as a unit-stride array*/,
                            const int32_t* ray_val /*[R] or NULL*/,
                            int32_t* o_ray_val /*[M] or NULL: ray_val of each survivor's ray = f2n_scatter_idx on the new bounds*/);

/* Compositing (Renderer.cpp:196-208): colors = sum w*c + T_last*bg, disparity = sum w/(t+.01),
 * depth = sum w*(t+.01) / (1 - T_last + 1e-4); weights [M] is also returned (RenderResult, Renderer.h:18-27).
 * f0 of sample i = f0[i * f0_stride]: stride 16 reads column 0 of the field output [M,16] as the reference does,
 * stride 1 reads a compact density array (f2n_field_fwd*'s out_f0: a quarter of the cache lines). */
int f2n_composite_fwd(void* stream, int n_rays, const int32_t* pts_start_end, const float* f0, int f0_stride,
                      const float* dt, const float* t, const float* rgb /*[M,3]*/, const float* bg /*[R,3]*/,
                      float* colors /*[R,3]*/, float* disparity /*[R]*/, float* depth /*[R]*/, float* weights /*[M]*/,
                      float* out_vars /*[R] or NULL: f2n_weight_var_fwd of the weights, same arithmetic, same launch*/);

/* Backward of the above through TruncExp; gradient scaling (CustomOps.cu:68-80) is applied to dsigma and
 * drgb when grad_scaling_progress < 1.  Any of dcolors/ddisparity/ddepth/dweights may be NULL (= zero).
 * Writes drgb [M,3] and d f0: df0[i * df0_stride] (stride 16 = column 0 of dfeat [M,16], other columns untouched;
 * stride 1 = a compact array that f2n_shade_bwd merges into the dfeat rows it writes anyway). */
int f2n_composite_bwd(void* stream, int n_rays, const int32_t* pts_start_end, const float* f0, int f0_stride,
                      const float* dt, const float* t, const float* rgb, const float* bg, const float* dcolors,
                      const float* ddisparity, const float* ddepth, const float* dweights,
                      float grad_scaling_progress, float* drgb, float* df0, int df0_stride,
                      const float* var_weights /*[M] or NULL*/, const float* dvars /*[R] or NULL*/);
/* var_weights + dvars (both or neither): the gradient f2n_weight_var_bwd would produce from them is added to dweights
 * inside this launch (same arithmetic), so a training step needs neither the extra launch nor the [M] buffer. */

/* WeightVarLoss forward/backward (CustomOps.cu:12-66). */
int f2n_weight_var_fwd(void* stream, int n_rays, const float* weights, const int32_t* pts_start_end, float* out_vars);
int f2n_weight_var_bwd(void* stream, int n_rays, const float* weights, const int32_t* pts_start_end,
                       const float* dvars, float* dweights);

/* Distortion loss on the warped ray intervals: no reference counterpart (mip-NeRF 360, eq. 15, on the coordinate compositing
 * itself integrates over: the step length dt, sec = sigma * dt).  Sample k of a ray is the interval of length dt_k that follows the
 * intervals of the ray's earlier surviving samples; m_k is its midpoint, m_{k+1} - m_k = (dt_k + dt_{k+1}) / 2.  Per ray, over its
 * samples s <= k < e (pts_start_end [R,2]) with weights w [M]:
 *     dist         = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 dt_i
 *     d dist/d w_k = 2 sum_j w_j |m_k - m_j| + (2/3) w_k dt_k
 * evaluated without a cumulative coordinate and without a subtraction.  All arithmetic is fp32, EVERY operation below is one
 * rounding (never an FMA), every running sum adds left to right in the order written, starting from 0.f:
 *   forward, k = s .. e-1:   h_k = 0.5f * (dt[k-1] + dt[k])                    (h_s = 0.f)
 *                            P_k = P_{k-1} + w[k-1]                            (P_s = 0.f: the exclusive running sum of w)
 *                            D_k = D_{k-1} + P_k * h_k                         (D before s is 0.f)
 *                            l_k = w[k] * (2.f * D_k) + ((w[k] * w[k]) * dt[k]) * (1.f / 3.f)
 *                            dist = (((0.f + l_s) + l_{s+1}) + ...) + l_{e-1}
 *   reverse, k = e-1 .. s:   S_k = S_{k+1} + w[k+1]                            (S_{e-1} = 0.f)
 *                            U_k = U_{k+1} + S_k * (0.5f * (dt[k] + dt[k+1]))  (U behind e-1 is 0.f; the term of k = e-1 is 0.f)
 *                            g_k = ddist[ray] * (2.f * (D_k + U_k) + ((2.f / 3.f) * w[k]) * dt[k])
 * (1.f / 3.f and 2.f / 3.f are the fp32 constants.)  Every term is non-negative for non-negative w and dt, so nothing cancels: the
 * relative error of dist is below (3n+8) 2^-24 and that of every g_k below (2n+8) 2^-24 for a ray of n samples.
 * f2n_distortion_fwd writes dist [R] (0.f for an empty ray).  f2n_distortion_bwd writes dweights[k] = g_k for the samples of
 * non-empty rays -- the rows of empty rays and everything outside [s, e) are untouched -- and, if dist is not NULL, dist [R] with the
 * bits of f2n_distortion_fwd.  dweights is also the kernel's scratch for D_k between its two walks: it must not alias weights or dt.
 * A NaN or infinite weight stays inside its own ray.  F2N_ERR_INVALID_ARG: n_rays < 0, or n_rays > 0 and a NULL pointer other than
 * f2n_distortion_bwd's dist, or dweights == weights or dt.  n_rays == 0: F2N_OK, nothing is touched. */
int f2n_distortion_fwd(void* stream, int n_rays, const int32_t* pts_start_end, const float* weights, const float* dt,
                       float* dist /*[R]*/);
int f2n_distortion_bwd(void* stream, int n_rays, const int32_t* pts_start_end, const float* weights, const float* dt,
                       const float* ddist /*[R]*/, float* dweights /*[M]: rows of empty rays untouched*/,
                       float* dist /*[R] or NULL*/);
/* f2n_loss_add_mean: no reference counterpart.  mean = (float) (sum / (double) n) with sum the fp64 sum of x [n]: work-item t of ONE
 * workgroup of 256 adds x[t], x[t + 256], ... in that order to its own fp64 accumulator (from 0.0), then a[t] += a[t + off] for
 * off = 128, 64, .., 1 over t < off.  Then losses[slot] = mean and losses[0] = losses[0] + weight * mean (two fp32 roundings): the
 * result is a function of the inputs alone.  n < 1, slot outside [1, 7] or a NULL pointer: F2N_ERR_INVALID_ARG. */
int f2n_loss_add_mean(void* stream, int n, const float* x, float weight, float* losses /*[8]*/, int slot);

/* Seam-level FlexOps (FlexOps.cu:5-93) for callers that keep the reference's op-by-op structure. */
int f2n_flex_sum_fwd(void* stream, int n_rays, int vec, const float* val, const int32_t* start_end, float* sum);
int f2n_flex_sum_bwd(void* stream, int n_rays, int vec, const float* dsum, const int32_t* start_end, float* dval);
int f2n_flex_acc_fwd(void* stream, int n_rays, int include_this, const float* val, const int32_t* start_end, float* sum);
int f2n_flex_acc_bwd(void* stream, int n_rays, int include_this, const float* dsum, const int32_t* start_end, float* dval);

/* ---------------------------------------------------------------------------------------------------
 * Ray generation -- replaces Dataset::Img2WorldRayFlex / CameraUndistort
 * (Dataset/Dataset.cu:13-152) and the colour / bounds gathers of Dataset::RandRaysData (Dataset/Dataset.cpp:275-298).
 * ------------------------------------------------------------------------------------------------- */
/* Img2WorldRayKernel (Dataset.cu:93-123): ij int32 [n,2] = (row, column); the half-pixel shift of :126 is applied
 * inside.  poses [C,3,4] row-major c2w, intri [C,3,3], dist_params [C,4] = (k1,k2,p1,p2); Newton undistortion with
 * central differences, <= 100 iterations (:30-72).  rays_d is NOT normalised (GetSamples does that, :319). */
int f2n_img2world_rays(void* stream, int n_rays, const float* poses, const float* intri, const float* dist_params,
                       const int32_t* cam_indices /*[n]*/, const int32_t* ij /*[n,2]*/, float* rays_o /*[n,3]*/,
                       float* rays_d /*[n,3]*/);
/* gt_colors[r] = images[cam][i][j][0:3] (images fp32 [C,H,W,3], resident in HBM) and bounds[r] = cam_bounds[cam]
 * ([C,2]); either output may be NULL. */
int f2n_gather_pixels(void* stream, int n_rays, int height, int width, const float* images, const float* cam_bounds,
                      const int32_t* cam_indices, const int32_t* ij, float* gt_colors /*[n,3]*/, float* bounds /*[n,2]*/);
/* Dataset::RandRaysData (Dataset/Dataset.cpp:275-298) in one launch: u01 [R,3] uniforms in [0,1) pick an image of image_set
 * (n_set entries) and a pixel (i = floor(u1 * height), j = floor(u2 * width)); then f2n_img2world_rays and f2n_gather_pixels for
 * those draws.  Outputs: cam_indices [R], ij [R,2], rays_o / rays_d [R,3], gt_colors [R,3] (or NULL), bounds [R,2]. */
int f2n_draw_ray_batch(void* stream, int n_rays, const float* u01, const int32_t* image_set, int n_set, int height, int width,
                       const float* poses, const float* intri, const float* dist_params, const float* images /*or NULL*/,
                       const float* cam_bounds, int32_t* cam_indices, int32_t* ij, float* rays_o, float* rays_d,
                       float* gt_colors /*or NULL*/, float* bounds);
/* The same with the three uniforms of ray r drawn by the launch itself: Philox4x32-10, counter = (r, 0, seq), key = seed ^ purpose
 * (host/KeyedDraws.h): batch `seq` is the same batch whenever, however often and with whatever else in between it is drawn. */
int f2n_draw_ray_batch_keyed(void* stream, int n_rays, uint64_t key, uint64_t seq, const int32_t* image_set, int n_set, int height,
                             int width, const float* poses, const float* intri, const float* dist_params, const float* images /*or NULL*/,
                             const float* cam_bounds, int32_t* cam_indices, int32_t* ij, float* rays_o, float* rays_d,
                             float* gt_colors /*or NULL*/, float* bounds);

/* ---------------------------------------------------------------------------------------------------
 * Optimiser -- replaces torch::optim::Adam::step over the groups of Hash3DAnchored::OptimParamGroups
 * (Field/Hash3DAnchored.cpp:124-150), SHShader (Shader/SHShader.cpp:44-56), Renderer (Renderer.cpp:238-258):
 * beta = (0.9, 0.99), eps = 1e-15, L2 weight decay added to the gradient (torch Adam semantics).
 * beta1 / beta2 are DOUBLES, as in torch::optim::AdamOptions (`opt->betas() = {0.9, 0.99}`, Hash3DAnchored.cpp:131): LibTorch forms
 * 1 - beta and the bias corrections 1 - beta^step in double and only then narrows them to the tensors' float, so (float)(1 - 0.9) =
 * 0.1f -- a float beta would give 1 - 0.9f = 0.100000024 and a second-moment coefficient that is 9e-7 off (ABI v12; up to v11 the
 * betas were floats).  f2n_adam_coefficients returns the nine scalars every Adam kernel of this library is launched with:
 * out[0..8] = -step_size's magnitude lr / (1 - beta1^step), sqrt(1 - beta2^step), beta1, beta2, 1 - beta1, 1 - beta2, eps,
 * weight_decay, grad_scale.  Host function, no device needed (tests pin it against LibTorch's own scalars).
 * ------------------------------------------------------------------------------------------------- */
int f2n_adam_coefficients(int step, float lr, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                          float* out9 /*host*/);
/* fp32 gradient (grad * grad_scale is the true gradient); optionally refreshes an h16 working copy.
 * grad_round_h16 != 0 reproduces the two binary16 roundings the reference applies to MLP parameter gradients:
 * g = f16(f16(grad) * grad_scale) (tcnn param-precision output while loss-scaled, Field/TCNNWP.cpp:214-215, then
 * autograd's cast of the unscaled gradient to the f16 dtype of the Function input, :111,:242). */
int f2n_adam_step(void* stream, int n, float* param, float* grad, float grad_scale, int grad_round_h16,
                  float* exp_avg, float* exp_avg_sq, int step, float lr, double beta1, double beta2, float eps,
                  float weight_decay, void* param_h_or_null, int zero_grad /* clear grad after use (also when skipped) */,
                  const int32_t* skip_flag /*device, or NULL*/);
/* The small parameter groups of an iteration in ONE launch: finiteness flags (TCNNWP.cpp:234-240; layout of
 * f2n_nonfinite_flags: flags[0] = group 0 has a non-finite gradient, flags[1] = group 1, flags[2] = either; only groups
 * 0 and 1 may ask for the check) followed by f2n_adam_step on every group, predicated on flags[2] and on *skip_flag.
 * `groups` is a HOST array of 1..4 descriptors; element-wise arithmetic identical to f2n_adam_step. */
typedef struct F2nAdamGroup {
  float* param;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  void* param_h;      /* h16 working copy to refresh, or NULL */
  int n;
  float grad_scale;
  float weight_decay;
  int grad_round_h16;
  int check_finite;
} F2nAdamGroup;
int f2n_adam_small_groups(void* stream, int n_groups, const F2nAdamGroup* groups, int step, float lr, double beta1,
                          double beta2, float eps, int zero_grad, int32_t* flags /*device [3] or NULL*/,
                          const int32_t* skip_flag /*device, or NULL*/);
/* Every group of an iteration in one launch: `groups` (HOST array of 0..4 descriptors; check_finite is ignored) as in
 * f2n_adam_small_groups and the h16-gradient table as in f2n_adam_step_h16grad, all predicated on *skip_flag (device, or
 * NULL) -- typically flags + 2 of a preceding f2n_nonfinite_flags.  Element-wise arithmetic identical to the separate
 * steps; no block-wide dependency inside (the flags-then-step single-block launch took 21 us in front of the table pass). */
int f2n_adam_fused(void* stream, int n_groups, const F2nAdamGroup* groups, int n_table, float* table_param, void* table_grad_h,
                   float table_grad_scale, float* table_exp_avg, float* table_exp_avg_sq, void* table_param_h, int step, float lr,
                   double beta1, double beta2, float eps, int zero_grad, const int32_t* skip_flag /*device, or NULL*/);
/* ---------------------------------------------------------------------------------------------------
 * The TAIL of a training step in one call (ABI v13, round 6) -- f2n_field_bwd_dyn + f2n_reduce_deferred + f2n_nonfinite_flags_ex +
 * f2n_adam_fused, re-ordered the way their data allows (ExpRunner.cpp:127-137: backward, finiteness check, optimizer->step(),
 * zero_grad()):
 *   stream:       field-MLP backward | hash_bin (scatter producers) ............... | owners: slice sums -> THE TABLE'S ADAM on that slice
 *   tail_stream:                     | reduce_deferred -> flags -> Adam of the small groups |  (joined in front of the owners)
 * The finiteness flags depend on the two MLPs' parameter gradients only (TCNNWP.cpp:234-240), which are complete once the
 * field-MLP backward kernel has run -- not on the scatter that follows it; and an owner block of the binned scatter holds the
 * finished gradient sums of its 4096-entry table slice in LDS, so it steps that slice's parameters itself (fp16->fp32 widening,
 * /128, Adam, fp32->fp16 refresh, the gradient table left zero: f2n_adam_step_h16grad's arithmetic, element for element)
 * instead of writing the sums to the gradient table for a 267 MB streaming pass behind the step's last kernel.  Parameters,
 * moments, working copies, flags and the (zero) gradient buffers end bit-identical to the four separate calls
 * (tests/test_gpu_parity.py::test_step_tail_equals_separate_launches).
 * tail_stream NULL: everything on `stream` (same results).  A batch that does not take the binned scatter (f2n_hash_bwd's
 * small-batch path), a table whose active prefix is not whole 4096-entry slices, or a bucket hook on this gradient table
 * (f2n_set_scatter_buckets_for: data-parallel runs all-reduce the gradient first) steps the table with the ordinary launch
 * behind the scatter.  `tail->groups`: HOST array as for f2n_adam_fused; every update is predicated on flags[2]. */
typedef struct F2nStepTail {
  int n_flags_a;                 /* f2n_nonfinite_flags_ex: field-MLP gradient ... */
  const float* flags_grad_a;
  int n_flags_b;                 /* ... colour-MLP gradient */
  const float* flags_grad_b;
  int32_t* flags;                /* device int32[3] */
  int32_t* flags_mirror;         /* mapped host words, or NULL */
  int n_groups;                  /* the small fp32 groups (0..4) */
  const F2nAdamGroup* groups;
  int n_table;                   /* halves of the table group's active prefix */
  float* table_param;
  float* table_exp_avg;
  float* table_exp_avg_sq;
  void* table_param_h;
  float table_grad_scale;
  int step;
  float lr;
  double beta1, beta2;
  float eps;
  /* Data-parallel hosts (the gradients travel before anything is stepped):
   * after_reduce != NULL: called on the calling host thread once the deferred reductions have been QUEUED on the tail stream (or on
   *   `stream` when there is none) -- the small gradient buffers are complete behind that point of that stream -- and before the flag
   *   kernel is: the host orders its exchange of the small buffers in between (event on that stream -> communicator stream -> event ->
   *   back), so that it travels beside the scatter's producers instead of behind the step;
   * leave_table_to_caller != 0: everything BUT the table's Adam -- the owners write their sums to the gradient table as
   *   f2n_field_bwd_dyn's do (a bucket hook on the table reports as usual), `stream` is left waiting for the tail chain, and the caller
   *   steps the table itself (f2n_adam_fused with no small groups, skip flag = flags + 2) once ITS exchange is through. */
  void (*after_reduce)(void* user, void* chain_stream);
  void* after_reduce_user;
  int leave_table_to_caller;
} F2nStepTail;
int f2n_field_bwd_step_tail(void* stream, void* tail_stream /* or NULL */, int n_max, const int32_t* n_dev, int n_off, int n_volumes,
                            const int32_t* prim_pool, const int32_t* local_idx, const int32_t* local_size, const float* bias_pool,
                            const float* level_scale, const float* pts_warped, const int32_t* volume_idx, int vol_stride,
                            const void* mlp_params_h, const void* saved_x_h, const float* dfeat, float loss_scale,
                            float* dparams_f32_scaled, void* grad_table_h, int level_entries, const F2nStepTail* tail,
                            int* table_stepped_by_owners /* out, or NULL: 1 when the owners applied the table's Adam */);
/* ---------------------------------------------------------------------------------------------------
 * Reuse of the density pre-pass's field outputs in the grad pass (same ABI version: additions only).  Renderer::Render queries the
 * field twice per step with an unchanged table AND unchanged network weights (Renderer.cpp:115-123 and :152-166; the optimiser
 * runs at the step's end), so the grad pass's 16 field outputs of a surviving sample are the pre-pass's, bit for bit.
 *   f2n_field_fwd_ex / f2n_field_fwd_fused_ex / f2n_field_mlp_planes_ex: the three pre-pass routes with one more output,
 *     out_feat_h [n,16] h16 (may be NULL: exactly the plain entry point) = the network's outputs at their f16 output precision
 *     (TCNNWP.cpp:143-144), i.e. out_feat_f32 before its widening.
 *   f2n_shade_fwd_feat: f2n_field_shade_fwd_extra without the field network -- sample i takes row src_rows[i] (NULL = row i) of
 *     feat_cache_h [*,16] (a pre-pass's out_feat_h), then [1 | feat[1:]] + app_emb | SH4 -> colour MLP -> sigmoid as there;
 *     out_f0 / save_shade_x_h / rgb as there; the n_extra edge rows (Renderer.cpp:159-166) are feat_extra_h [n_extra,16] widened
 *     into feat_extra fp32 [n_extra,16].  Nothing is saved for the field backward: see the _rows calls.
 *   f2n_field_bwd_dyn_rows / f2n_field_bwd_step_tail_rows: f2n_field_bwd_dyn / f2n_field_bwd_step_tail whose saved input is not
 *     a compact [n_max,32] copy: row s < n_off is row s of x_edge_h [n_off,32] (may be NULL when n_off == 0), row s >= n_off is
 *     row src_rows[s - n_off] of x_cache_h [*,32] (the pre-pass's save_x_h).  Same results as the compact calls on the gathered rows.
 * ------------------------------------------------------------------------------------------------- */
int f2n_field_fwd_ex(void* stream, int n, int n_volumes, const void* table_h, const int32_t* prim_pool,
                     const int32_t* local_idx, const int32_t* local_size, const float* bias_pool,
                     const float* level_scale, const float* pts_warped, const int32_t* volume_idx, int vol_stride,
                     const void* mlp_params_h, float* out_feat_f32, float* out_f0, void* save_x_h, void* out_feat_h);
int f2n_field_fwd_fused_ex(void* stream, int n, int n_volumes, const void* table_h, const int32_t* prim_pool, const int32_t* local_idx,
                           const int32_t* local_size, const float* bias_pool, const float* level_scale, const float* pts_warped,
                           const int32_t* volume_idx, int vol_stride, const void* mlp_params_h, float* out_feat_f32 /*or NULL*/,
                           float* out_f0 /*or NULL*/, void* save_x_h /*or NULL*/, void* out_feat_h /*or NULL*/);
int f2n_field_mlp_planes_ex(void* stream, int n, const void* planes_h, const void* mlp_params_h, float* out_feat_f32,
                            float* out_f0, void* save_x_h, void* out_feat_h);
int f2n_shade_fwd_feat(void* stream, int n_max, const int32_t* n_dev, const int32_t* src_rows, const void* feat_cache_h,
                       const float* dirs, const float* app_emb, const int32_t* sample_emb_idx, const void* color_params_h,
                       float* out_f0, void* save_shade_x_h, float* rgb, int n_extra, const void* feat_extra_h, float* feat_extra);
int f2n_field_bwd_dyn_rows(void* stream, int n_max, const int32_t* n_dev, int n_off, int n_volumes, const int32_t* prim_pool,
                           const int32_t* local_idx, const int32_t* local_size, const float* bias_pool, const float* level_scale,
                           const float* pts_warped, const int32_t* volume_idx, int vol_stride, const void* mlp_params_h,
                           const void* x_edge_h, const void* x_cache_h, const int32_t* src_rows, const float* dfeat, float loss_scale,
                           float* dparams_f32_scaled, void* grad_table_h, int level_entries, int defer_reduce);
int f2n_field_bwd_step_tail_rows(void* stream, void* tail_stream /* or NULL */, int n_max, const int32_t* n_dev, int n_off, int n_volumes,
                                 const int32_t* prim_pool, const int32_t* local_idx, const int32_t* local_size, const float* bias_pool,
                                 const float* level_scale, const float* pts_warped, const int32_t* volume_idx, int vol_stride,
                                 const void* mlp_params_h, const void* x_edge_h, const void* x_cache_h, const int32_t* src_rows,
                                 const float* dfeat, float loss_scale, float* dparams_f32_scaled, void* grad_table_h, int level_entries,
                                 const F2nStepTail* tail, int* table_stepped_by_owners /* out, or NULL */);
/* ---------------------------------------------------------------------------------------------------
 * The gather's planes as the pre-pass cache (same ABI version: additions only).  The large-batch pre-pass gathers the hash features
 * as h16 planes [8][plane_rows][4] (f2n_hash_gather_planes_*: plane p holds features 4p..4p+3 of every row); with save_x_h = NULL
 * f2n_field_mlp_planes_ex writes no row-major copy of them, and the field backward of the same step reads the planes themselves.
 *   f2n_field_bwd_dyn_planes / f2n_field_bwd_step_tail_planes: the _rows calls with a different saved input.  x_planes_h is the
 *     plane base ALREADY offset to the survivors' first row (by 4 halves per row), plane_rows the row count of one plane: row
 *     s >= n_off is the 8 halves at ((g * plane_rows + src_rows[s - n_off]) * 4) followed by the 8 halves at
 *     (((4 + g) * plane_rows + src_rows[s - n_off]) * 4), g = 0..3 -- the pre-pass MLP's own read of that row.  Row s < n_off is
 *     row s of x_edge_h [n_off,32] as in the _rows calls, or -- x_edge_planes_h not NULL: the same planes offset to the edge
 *     samples' first row -- row s of those planes (x_edge_h is then ignored).  Both bases are 8-byte aligned.  Everything behind
 *     the load is the _rows calls' code: same weight gradients, dL/dx planes, mask words and gradient table.
 * ------------------------------------------------------------------------------------------------- */
int f2n_field_bwd_dyn_planes(void* stream, int n_max, const int32_t* n_dev, int n_off, int n_volumes, const int32_t* prim_pool,
                             const int32_t* local_idx, const int32_t* local_size, const float* bias_pool, const float* level_scale,
                             const float* pts_warped, const int32_t* volume_idx, int vol_stride, const void* mlp_params_h,
                             const void* x_edge_h /* or NULL */, const void* x_edge_planes_h /* or NULL */, const void* x_planes_h,
                             int plane_rows, const int32_t* src_rows, const float* dfeat, float loss_scale, float* dparams_f32_scaled,
                             void* grad_table_h, int level_entries, int defer_reduce);
int f2n_field_bwd_step_tail_planes(void* stream, void* tail_stream /* or NULL */, int n_max, const int32_t* n_dev, int n_off, int n_volumes,
                                   const int32_t* prim_pool, const int32_t* local_idx, const int32_t* local_size, const float* bias_pool,
                                   const float* level_scale, const float* pts_warped, const int32_t* volume_idx, int vol_stride,
                                   const void* mlp_params_h, const void* x_edge_h /* or NULL */, const void* x_edge_planes_h /* or NULL */,
                                   const void* x_planes_h, int plane_rows, const int32_t* src_rows, const float* dfeat, float loss_scale,
                                   float* dparams_f32_scaled, void* grad_table_h, int level_entries, const F2nStepTail* tail,
                                   int* table_stepped_by_owners /* out, or NULL */);
/* h16 gradient table produced by f2n_hash_bwd / f2n_field_bwd (true gradient = float(grad_h) * grad_scale,
 * grad_scale = 1/128): fuses the fp16->fp32 cast, the /128 (Hash3DAnchored.cu:232), Adam, the fp32->fp16
 * refresh of the table (Hash3DAnchored.cu:186) and the re-zeroing of the gradient (:222) in one pass. */
int f2n_adam_step_h16grad(void* stream, int n, float* param, void* grad_h, float grad_scale, float* exp_avg,
                          float* exp_avg_sq, int step, float lr, double beta1, double beta2, float eps,
                          float weight_decay, void* param_h, int zero_grad, const int32_t* skip_flag /*device, or NULL*/);
/* skip_flag (both steps): when *skip_flag != 0 on the device the update is dropped -- parameters and moments stay,
 * an h16 gradient table is still cleared when zero_grad is set.  This is the `continue` of ExpRunner.cpp:131-134
 * without a host round trip between the finiteness check and the optimiser. */

/* ---------------------------------------------------------------------------------------------------
 * Training loss -- replaces the ~30 ATen element-wise / reduction ops (and their autograd mirror images) of
 * ExpRunner::Train (ExpRunner.cpp:95-120) by one pass that returns the loss terms AND their gradients:
 *   color = mean sqrt((pred-gt)^2 + 1e-4), disp = mean disparity^2, var = mean sqrt(sampled_var + 1e-2),
 *   tv = mean (edge_feats[:,0,:] - edge_feats[:,1,:])^2, loss = color + var_w*var + disp_w*disp + tv_w*tv.
 * out_losses [8] = {loss, color, var, disp, tv, mse, 0, 0}.  Gradients of `loss`: dcolors [R,3], ddisparity [R],
 * dvar [R], dedge_feats [E,2,feat_dim]; any gradient pointer may be NULL, and disparity / sampled_var /
 * edge_feats may be NULL (term = 0), as on the reference's no-sample early return (Renderer.cpp:83-97).
 * ------------------------------------------------------------------------------------------------- */
int f2n_train_loss(void* stream, int n_rays, const float* pred_colors /*[R,3]*/, const float* gt_colors /*[R,3]*/,
                   const float* disparity /*[R]*/, const float* sampled_var /*[R]*/, int n_edge, int feat_dim,
                   const float* edge_feats /*[E,2,feat_dim]*/, float var_w, float disp_w, float tv_w,
                   float* out_losses /*[8]*/, float* dcolors, float* ddisparity, float* dvar, float* dedge_feats);

/* f2n_composite_fwd -> f2n_train_loss -> f2n_composite_bwd in ONE launch (the streaming training step; round 4): every ray is
 * walked forward, its loss terms and their gradients are formed in registers (they are element-wise per ray: ExpRunner.cpp:95-120),
 * and the same row walks it backward with the totals still at hand.  Outputs as the three calls': colors [R,3], weights [M], drgb
 * [M,3], df0 (stride df0_stride) -- bit-identical -- plus dedge_feats (TV gradient) and out_losses [8] = {loss, colour, var,
 * disparity, tv, mse, 0, 0}: zeroed by the launch and completed by the reduction of its per-block partial sums -- at once
 * (defer_reduce = 0) or by the step's f2n_reduce_deferred (defer_reduce = 1).  The reported loss VALUES sum pre-scaled terms
 * (mean = sum of x / n instead of (sum of x) / n): equal to f2n_train_loss's to rounding, not bit for bit. */
int f2n_composite_train(void* stream, int n_rays, const int32_t* pts_start_end, const float* f0, int f0_stride, const float* dt,
                        const float* t, const float* rgb, const float* bg, const float* gt_colors, float var_w, float disp_w, float tv_w,
                        float grad_scaling_progress, int n_edge, int feat_dim, const float* edge_feats /*[E,2,feat_dim] or NULL*/,
                        float* dedge_feats /*or NULL*/, float* colors, float* weights, float* drgb, float* df0, int df0_stride,
                        float* out_losses /*[8]*/, int defer_reduce);

/* Gradient finiteness check of the two MLPs (Field/TCNNWP.cpp:234-240), device side:
 * flags[0] = a has a non-finite value, flags[1] = b has one, flags[2] = either (the optimiser's skip_flag). */
int f2n_nonfinite_flags(void* stream, int n_a, const float* a, int n_b, const float* b, int32_t* flags /*[3]*/);
/* The same, with the three flags also written to `mirror` (DEVICE pointer to MAPPED HOST memory, or NULL): the host-side
 * reaction of TCNNWP.cpp:236-240 (halve the loss scale, drop the iteration) reads them there behind an event, without a copy
 * launch behind the optimiser. */
int f2n_nonfinite_flags_ex(void* stream, int n_a, const float* a, int n_b, const float* b, int32_t* flags /*[3]*/,
                           int32_t* mirror /*mapped host [3] or NULL*/);

/* ---------------------------------------------------------------------------------------------------
 * World-space queries and meshes (additive; the ABI version is unchanged).  csrc/octree.hip.
 * ------------------------------------------------------------------------------------------------- */
/* Fills the seam the reference leaves empty: Field::Query(coords) is `CHECK(false) << "Not implemented"` (Field/Field.h:14).
 * Point location: descend from node 0 (PersSampler.cpp:82), child slot st = 4 (x >= cx) + 2 (y >= cy) + (z >= cz) (the offset order
 * of ConstructTreeNode, :397-401), stop at a node with no children.  A point is EMPTY when it lies outside the root cube (closed
 * bounds), falls into a child slot that is -1, or reaches a leaf with trans_idx < 0 -- exactly the nodes
 * FindRayOctreeIntersectionKernel never lists (PersSampler.cu:54-152).  Non-empty: out_pts_warped = f2n_warp(transes[trans_idx], p),
 * anchors = (trans_idx, leaf, 0), the layout of f2n_ray_march_fill.  Empty: warped (0, 0, 0), anchors (-1, -1, 0). */
int f2n_oct_locate_warp(void* stream, int n, const float* pts_world /*[n,3]*/, const void* tree_nodes, const void* transes,
                        float* out_pts_warped /*[n,3]*/, int32_t* out_anchors /*[n,3]*/);
/* The same for the points of an implicit grid: point (ix, iy, iz), iz in [first_z, first_z + n_z), is lo[k] + step * (float) i_k
 * (rounded twice, never an FMA), rows x fastest: output row (iz - first_z) * nx * ny + iy * nx + ix.  lo is HOST data.
 * No reference counterpart (the reference has no grid query). */
int f2n_oct_locate_warp_grid(void* stream, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int first_z, int n_z,
                             const void* tree_nodes, const void* transes, float* out_pts_warped /*[nx*ny*n_z,3]*/,
                             int32_t* out_anchors /*[nx*ny*n_z,3]*/);
/* Compaction of the non-empty located points, count -> f2n_segment_scan -> fill: counts[i] = (anchors[i,0] >= 0), start_end from the
 * scan, total[0] = their number; point i goes to row start_end[i,0] of out_pts / out_vol (= trans_idx) / out_src (= i, or NULL).
 * No reference counterpart. */
int f2n_located_compact(void* stream, int n, const int32_t* anchors /*[n,3]*/, const float* pts_warped /*[n,3]*/, int32_t* counts /*[n]*/,
                        int32_t* start_end /*[n,2]*/, int32_t* total /*[1]*/, float* out_pts /*[n,3]*/, int32_t* out_vol /*[n]*/,
                        int32_t* out_src /*[n] or NULL*/);
/* density[i] = exp(f0[start_end[i,0]] - 3) for the non-empty points (TruncExp of Renderer.cpp:101-104), exactly 0 for the empty ones;
 * f0 = the field's density pre-activation of the compacted points.  No reference counterpart. */
int f2n_density_scatter(void* stream, int n, const int32_t* anchors /*[n,3]*/, const int32_t* start_end /*[n,2]*/, const float* f0,
                        float* density /*[n]*/);
/* Iso-surface of ANY float32 grid g [nz, ny, nx] (x fastest) by marching tetrahedra on the Kuhn split (six tetrahedra per cell
 * around its (0,0,0)-(1,1,1) diagonal; no ambiguous case, watertight).  No reference counterpart (the reference ships no mesh export).
 *   A corner is inside iff g > level.  Every crossing edge gets ONE vertex, owned by its lower corner; the edge is one of the 7 types
 *   {+x, +y, +z, +xy, +xz, +yz, +xyz} = 0..6.  Vertex order: (owner corner index, type).  Face order: (cell index, tet 0..5 for the
 *   axis orders xyz, xzy, yxz, yzx, zxy, zyx, triangle).  Tet vertices are numbered 0..3 along (0, a, a|b, 7).  One corner i alone on
 *   its side, j < k < l the others: triangle (ij, ik, il); corners i < j inside, k < l outside: triangles (ik, il, jl), (ik, jl, jk)
 *   -- each with its second and third vertex swapped where needed so that its normal points from inside to outside.
 *   Position p_a + t (p_b - p_a), t = (level - g_a) / (g_b - g_a), a = the lower endpoint, p = lo + step * index as above.
 * f2n_mesh_count: edge_mask [N] (bit t: the edge of type t crosses), the per-corner vertex counts and per-cell face counts and their
 *   scans (N = nx*ny*nz corners, C = (nx-1)(ny-1)(nz-1) cells); totals[0] = vertices, totals[1] = faces -- the only values a caller
 *   needs on the host (to size the outputs).  Any grid with N <= 2^31 - 1 is accepted (F2N_ERR_INVALID_ARG above, e.g. 1291^3; a cubic
 *   box at resolution 1024 has N = 1025^3 > 2^30): corner and cell indices and the offsets into the [N,2] / [C,2] scans are 64-bit,
 *   f2n_segment_scan's as stated there.
 * f2n_mesh_emit: verts [totals[0],3] f32, faces [totals[1],3] int32.  lo is HOST data. */
int f2n_mesh_count(void* stream, int nx, int ny, int nz, const float* grid, float level, uint8_t* edge_mask /*[N]*/,
                   int32_t* vert_counts /*[N]*/, int32_t* vert_start_end /*[N,2]*/, int32_t* face_counts /*[C]*/,
                   int32_t* face_start_end /*[C,2]*/, int32_t* totals /*[2]*/);
int f2n_mesh_emit(void* stream, int nx, int ny, int nz, const float* grid, float level, const float* lo /*host [3]*/, float step,
                  const uint8_t* edge_mask, const int32_t* vert_start_end, const int32_t* face_start_end, float* verts, int32_t* faces);
/* f2n_density_scatter with a colour: density[i] = exp(f0[k] - 3) (the same expression, the same bits) and rgb[i] = rgb_rows[k],
 * k = start_end[i,0], for the non-empty points; density 0 and rgb (0, 0, 0) exactly for the empty ones (anchors[i,0] < 0).
 * f0 [m] / rgb_rows [m,3] = the field's density pre-activation and the shader's output (no appearance embedding: what the inference
 * path computes per sample) for the m compacted points of f2n_located_compact; both may be NULL when every point is empty.
 * No reference counterpart. */
int f2n_radiance_scatter(void* stream, int n, const int32_t* anchors /*[n,3]*/, const int32_t* start_end /*[n,2]*/, const float* f0,
                         const float* rgb_rows, float* density /*[n]*/, float* rgb /*[n,3]*/);
/* Unit normals at n points from ANY float32 grid g [nz, ny, nx] (x fastest; nx, ny, nz >= 2), step > 0, lo HOST data.  No reference
 * counterpart.
 *   Corner gradient G[c], component k: (g[c + e_k] - g[c - e_k]) / (2 step) in the interior; on the two border planes of axis k the
 *   one-sided difference over step ((g[1] - g[0]) / step at index 0, (g[n-1] - g[n-2]) / step at index n_k - 1).
 *   Point p: u_k = (p_k - lo_k) / step clamped to [0, n_k - 1] (NaN -> 0), cell c_k = min(floor(u_k), n_k - 2), f_k = u_k - c_k;
 *   g(p) = the trilinear blend of the eight G of that cell, a (1 - f) + b f along x, then y, then z (continuous across cells: a
 *   vertex on a cell face has no ambiguous case).  G is never materialised: 24 corner reads of g per point and component.
 *   out = -g(p) / |g(p)| (density grows inwards, f2n_mesh_emit winds outwards); (0, 0, 0) where |g(p)| is 0 or not finite. */
int f2n_grid_normals(void* stream, int n, const float* pts /*[n,3]*/, const float* grid, int nx, int ny, int nz,
                     const float* lo /*host [3]*/, float step, float* out /*[n,3]*/);
/* Connected components of a triangle mesh: labels[v] = the SMALLEST vertex index of v's component, two vertices being connected when
 * a face uses both; a vertex no face uses is its own component.  The labels are a unique fixpoint: nothing depends on scheduling.
 * A parent array (labels itself) starts as the identity; a round lets every face hook the larger roots of its three vertices under
 * the smallest (atomicMin) and then points every vertex at its root; rounds repeat until one hooks nothing.  `changed` is a DEVICE
 * word of scratch that a round sets; this call READS IT BACK after every round, so it synchronises the stream and returns with the
 * labels complete.  *rounds (HOST, or NULL) receives the number of rounds, the confirming one included (0 without faces).
 * A face with an index outside [0, n_verts) connects nothing.  F2N_ERR_UNSUPPORTED after 4096 rounds (no mesh gets near).
 * No reference counterpart. */
int f2n_mesh_components(void* stream, int n_verts, int n_faces, const int32_t* faces /*[F,3]*/, int32_t* labels /*[V]*/,
                        int32_t* changed /*[1]*/, int* rounds /*host [1] or NULL*/);
/* Removal of the components with fewer than min_faces faces, count -> f2n_segment_scan -> emit as f2n_mesh_count / f2n_mesh_emit.
 * f2n_mesh_filter_count: comp_faces[l] = number of faces whose vertices carry label l (integer atomics: order-free); face_keep[f] =
 *   (comp_faces[label of f] >= min_faces); vert_keep[v] = (a kept face uses v) -- so a vertex no face uses is never kept, whatever
 *   min_faces; the scans of both; totals[0] = kept vertices, totals[1] = kept faces: the only values a caller needs on the host.
 *   A face with an index outside [0, n_verts) is never kept.
 * f2n_mesh_filter_emit: kept vertices and faces IN THEIR ORIGINAL RELATIVE ORDER: out_verts [totals[0],3], vert_src [totals[0]] =
 *   the original index of every kept vertex, out_faces [totals[1],3] re-indexed (vert_start_end[v,0] of each corner).
 * No reference counterpart. */
int f2n_mesh_filter_count(void* stream, int n_verts, int n_faces, const int32_t* faces /*[F,3]*/, const int32_t* labels /*[V]*/,
                          int min_faces, int32_t* comp_faces /*[V]*/, int32_t* vert_keep /*[V]*/, int32_t* vert_start_end /*[V,2]*/,
                          int32_t* face_keep /*[F]*/, int32_t* face_start_end /*[F,2]*/, int32_t* totals /*[2]*/);
int f2n_mesh_filter_emit(void* stream, int n_verts, int n_faces, const float* verts /*[V,3]*/, const int32_t* faces /*[F,3]*/,
                         const int32_t* vert_keep, const int32_t* vert_start_end, const int32_t* face_keep, const int32_t* face_start_end,
                         float* out_verts, int32_t* vert_src, int32_t* out_faces);
/* The analytic gradient of the density pre-activation f0 = (W2 relu(W1 x))[0] with respect to the WARPED position w of n points, for the
 * shipped field shape (32 -> 64 -> 16): x = the h16 hash features of the points ([n,32], what f2n_field_fwd saves in save_x_h).
 *   df0/dx = W1^T (m . W2[0,:]), m_j = 1 where the fp32 pre-activation (W1 x)_j of the h16 x is > 0, else 0;
 *   df0/dw = sum_l (scale_l / 2) sum_c df0/dx_{l,c} d(blend_{l,c})/d(a, b, c): the derivative of the eight weights of the level's cell
 *   (the one floorf chose: on a cell face the one-sided derivative of that cell; q < 0 saturates as in the forward) with respect to
 *   the fractions, corner bit 2 = x, 1 = y, 0 = z.
 * Every input is an exact h16 value; all arithmetic is fp32 in a fixed order (levels in pairs, pairs in order): no h16 rounding, no
 * loss scale, no atomics, the same bits on every call.  out_dx [n,32] f32 (or NULL) receives df0/dx, out_df0_dw [n,3] f32 df0/dw.
 * The world-space gradient of sigma = exp(f0 - 3) is sigma J^T df0/dw (f2n_density_grad_scatter).  No reference counterpart. */
int f2n_field_density_grad(void* stream, int n, int n_volumes, const void* table_h, const int32_t* prim_pool, const int32_t* local_idx,
                           const int32_t* local_size, const float* bias_pool, const float* level_scale, const float* pts_warped,
                           const int32_t* volume_idx, int vol_stride, const void* mlp_params_h, const void* x_h /*[n,32] h16*/,
                           float* out_dx /*[n,32] f32 or NULL*/, float* out_df0_dw /*[n,3] f32*/);
/* The second half of the above on its own: df0/dw from ANY df0/dx [n,32] f32 (16-byte aligned), for field shapes the fused entry does
 * not cover -- there dx comes from f2n_mlp_bwd(dy = e_0, loss_scale = 1) and carries that kernel's h16 roundings. */
int f2n_hash_pos_grad(void* stream, int n, int n_volumes, const void* table_h, const int32_t* prim_pool, const int32_t* local_idx,
                      const int32_t* local_size, const float* bias_pool, const float* level_scale, const float* pts_warped,
                      const int32_t* volume_idx, int vol_stride, const float* dx /*[n,32] f32*/, float* out_df0_dw /*[n,3] f32*/);
/* f2n_density_scatter with the gradient: per point i with k = start_end[i,0], out_density[i] = exp(f0[k] - 3) (the same expression, the
 * same bits) and out_grad[i] = out_density[i] * J^T df0_dw[k], J = f2n_warp_jac of transes[anchors[i,0]] at pts_world[i]; exact zeros
 * for the empty points (anchors[i,0] < 0).  out_normal [n,3] (or NULL) = -out_grad / |out_grad| by the rule of f2n_grid_normals:
 * (0, 0, 0) where |out_grad| is 0 or not finite.  f0 / df0_dw may be NULL when every point is empty.  No reference counterpart. */
int f2n_density_grad_scatter(void* stream, int n, const float* pts_world /*[n,3]*/, const int32_t* anchors /*[n,3]*/,
                             const int32_t* start_end /*[n,2]*/, const void* transes, const float* f0, const float* df0_dw /*[m,3]*/,
                             float* out_density /*[n]*/, float* out_grad /*[n,3]*/, float* out_normal /*[n,3] or NULL*/);

/* Geometry buffers of rendered rays, from the weights f2n_composite_fwd wrote.  Per sample i of ray r (s = pts_start_end[r,0] <= i <
 * e = pts_start_end[r,1]): x_i = rays_o[r] + t[i] * rays_d[r] (the point the march warped, the same two roundings),
 * g_i = J^T df0_dw[i] with J = f2n_warp_jac of transes[anchors[i,0]] at x_i, n_i = -g_i / |g_i| -- the expressions of
 * f2n_density_grad_scatter, bit for bit; (0, 0, 0) where |g_i| is 0 or not finite (or anchors[i,0] < 0).  Per ray, every sum fp32, left
 * to right, one term after the other:
 *   out_opacity[r] = sum w_i;  out_normal[r] = N / |N| with N = sum w_i n_i componentwise, (0, 0, 0) where |N| is 0 or not finite;
 *   out_surf_idx[r] = the first (global) sample index i whose inclusive running sum of w reaches tau (>= tau), with
 *   out_surf_t = t[i], out_surf_point = x_i, out_surf_normal = n_i; if there is none (or the ray has no sample): -1 and zeros.
 * out_sample_grad / out_sample_normal [M,3] (each may be NULL) receive g_i / n_i.  tau must lie in (0, 1].  No atomics: the outputs
 * are a function of the inputs alone.  No reference counterpart. */
int f2n_composite_geometry(void* stream, int n_rays, const int32_t* pts_start_end /*[R,2]*/, const float* weights /*[M], f2n_composite_fwd's*/,
                           const float* t /*[M]*/, const float* rays_o /*[R,3]*/, const float* rays_d /*[R,3]*/,
                           const int32_t* anchors /*[M,3]*/, const void* transes, const float* df0_dw /*[M,3]*/, float tau,
                           float* out_opacity /*[R]*/, float* out_normal /*[R,3]*/, int32_t* out_surf_idx /*[R]*/, float* out_surf_t /*[R]*/,
                           float* out_surf_point /*[R,3]*/, float* out_surf_normal /*[R,3]*/, float* out_sample_grad /*[M,3] or NULL*/,
                           float* out_sample_normal /*[M,3] or NULL*/);

/* ---------------------------------------------------------------------------------------------------
 * TSDF fusion of depth maps (additive; the ABI version is unchanged).  No reference counterpart.
 * ------------------------------------------------------------------------------------------------- */
/* Adds n_views depth maps into the running sums S [N] (sum of w d) and W [N] (sum of w) of the implicit grid of
 * f2n_oct_locate_warp_grid: N = nx ny nz points (64 bits), x fastest, p_k = lo[k] + step * (float) i_k (rounded twice, never an FMA);
 * lo is HOST data.  csrc/dataset.hip.
 *   poses [V,3,4] camera-to-world (R | o), intri [V,3,3] in units of depth-map pixels (fx = [0], cx = [2], fy = [4], cy = [5]),
 *   dist_params [V,4], depth [V,h,w] = the Euclidean distance from the camera centre to the surface along the pixel's ray (no surface
 *   where the value is not > 0: zero, negative, NaN), conf [V,h,w] or NULL (weight 1), trunc > 0 and finite.
 * One thread owns one voxel and walks the views in index order; every operation below is ONE fp32 rounding, in this order:
 *    1. q = p - o_v                                            (componentwise)
 *    2. c_j = R[0][j] q_0 + (R[1][j] q_1 + R[2][j] q_2)        (c = R^T q: three products, then f2n_sum3's order)
 *    3. s = -c_2; skip the view unless s > 0
 *    4. u = c_0 / s, v = (-c_1) / s                            (the inverse of the ray direction (u, -v, -1) of f2n_img2world_rays)
 *    5. (du, dv) = the distortion of f2n_img2world_rays' camera model at (u, v):  r2 = u u + v v, radial = k1 r2 + (k2 r2) r2,
 *       du = (u radial + (2 p1) (u v)) + p2 (r2 + 2 (u u)), dv = (v radial + (2 p2) (u v)) + p1 (r2 + 2 (v v))
 *    6. x = fx (u + du) + cx, y = fy (v + dv) + cy
 *    7. b = floor(x), a = floor(y); skip unless 0 <= a < h and 0 <= b < w (NaN skips)   -- the NEAREST pixel: no interpolation
 *       across depth discontinuities
 *    8. D = depth[v,a,b]; skip unless D > 0
 *    9. wgt = conf ? conf[v,a,b] : 1; skip unless wgt > 0
 *   10. sdf = D - sqrt(q_0 q_0 + (q_1 q_1 + q_2 q_2)); skip if sdf < -trunc
 *   11. d = sdf / trunc; d = d < 1 ? d : 1
 *   12. S += wgt d;  W += wgt
 * S and W are read once and written once per launch; there are no atomics, so the outputs are a function of the inputs alone, and
 * integrating the views [0, k) and then [k, V) into the same state gives the bits of one call over [0, V).
 * n_views == 0 or N == 0: F2N_OK, nothing is touched.  F2N_ERR_INVALID_ARG: a negative size, h or w outside [1, 2^24], trunc not
 * positive and finite, a NULL pointer other than conf. */
int f2n_tsdf_integrate(void* stream, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int n_views,
                       const float* poses /*[V,3,4]*/, const float* intri /*[V,3,3]*/, const float* dist_params /*[V,4]*/,
                       const float* depth /*[V,h,w]*/, const float* conf /*[V,h,w] or NULL*/, int h, int w, float trunc,
                       float* S /*[N]*/, float* W /*[N]*/);
/* The signed distance of the sums, POSITIVE INSIDE (the mesher's convention "inside iff g > level"), and where it is known:
 *   valid[i] = (W[i] >= min_weight && W[i] > 0);  g[i] = valid[i] ? (-S[i]) / W[i] : 0.   min_weight must not be NaN.  csrc/octree.hip. */
int f2n_tsdf_finalize(void* stream, int64_t n, const float* S, const float* W, float min_weight, float* g /*[n]*/, uint8_t* valid /*[n]*/);
/* f2n_mesh_count with a mask of the corners that carry a value (valid [N], non-zero = valid): the same outputs, for the UNCHANGED
 * f2n_mesh_emit.  A cell has faces only if all eight of its corners are valid.  The edge of offset o owned by corner c keeps its bit
 * only if it crosses the level AND at least one cell c - d inside the grid has eight valid corners, d running over the subsets of the
 * axes that o does not have -- exactly the cells whose Kuhn tetrahedra use that edge.  So every emitted vertex is used by a face, every
 * face comes from a fully observed cell, and the surface is open where observation ends.  With valid all non-zero every output equals
 * f2n_mesh_count's bit for bit.  csrc/octree.hip. */
int f2n_mesh_count_masked(void* stream, int nx, int ny, int nz, const float* grid, float level, const uint8_t* valid /*[N]*/,
                          uint8_t* edge_mask /*[N]*/, int32_t* vert_counts /*[N]*/, int32_t* vert_start_end /*[N,2]*/,
                          int32_t* face_counts /*[C]*/, int32_t* face_start_end /*[C,2]*/, int32_t* totals /*[2]*/);

/* ---------------------------------------------------------------------------------------------------
 * Sparse mesh extraction on bricks (additive; the ABI version is unchanged): the iso-surface of f2n_mesh_count / f2n_mesh_emit,
 * bit for bit, from the parts of a grid that can hold something -- the grid itself is never materialised.  No reference
 * counterpart.  csrc/octree.hip; tests/mesh_sparse_ref.py restates the definitions in numpy.
 * ------------------------------------------------------------------------------------------------- */
/* The VIRTUAL GRID is that of f2n_oct_locate_warp_grid: n[k] points per axis (2 <= n[k] <= F2N_BRICK_MAX_POINTS), point i =
 * p_k(i_k) = lo[k] + step * (float) i_k (rounded twice, never an FMA).  lo is HOST data.
 * BRICKS of B^3 cells, B in {4, 8, 16} (any other B: F2N_ERR_INVALID_ARG): nb[k] = ceil((n[k] - 1) / B) bricks per axis, linear id
 *   b = (b_z nb[1] + b_y) nb[0] + b_x (x fastest); nb[0] nb[1] nb[2] must be below 2^31 (F2N_ERR_UNSUPPORTED otherwise).
 *   Brick b READS the (B + 1)^3 corners b B + l, l in [0, B]^3, as one row of (B + 1)^3 values, local x fastest: (l_z (B + 1) + l_y)
 *   (B + 1) + l_x.  A corner with i_k > n[k] - 1 DOES NOT EXIST (its value is never read); no edge or cell that uses it exists.
 *   Brick b OWNS the cells with l in [0, B)^3 and the corners with l in [0, B)^3 -- the last brick of an axis (b_k = nb[k] - 1) also
 *   those with l_k = B: the grid's border plane when n[k] - 1 is a multiple of B, which no other brick reaches.  Every existing corner
 *   and cell has exactly one owner, and the owner's row holds both endpoints of every edge the corner owns and all eight corners of
 *   the cell.
 * KEYS (int64): corner (i_z n_y + i_y) n_x + i_x;  vertex 8 corner + type (owner corner and edge type 0..6 of f2n_mesh_count);
 *   cell (i_z (n_y - 1) + i_y) (n_x - 1) + i_x;  face 16 cell + ordinal, ordinal = the position of the triangle among its cell's faces
 *   in f2n_mesh_emit's order (tet, triangle), 0..11.  Sorted by key, vertices and faces are in f2n_mesh_emit's order. */
#define F2N_BRICK_MAX_POINTS (1 << 19)
/* flags [nb_z nb_y nb_x] uint8, a pure function of (tree_nodes, lo, step, n, B): flags[b] = 1 iff the CLOSED box of brick b,
 *   blo_k = p_k(b_k B) .. bhi_k = p_k(min(b_k B + B, n[k] - 1)), can hold a non-empty point:
 *   root test -- with h = side_len * .5f of node 0 (f2n_oct_locate_warp's expressions), bhi_k >= center_k - h and blo_k <= center_k + h
 *   for every axis, else 0;
 *   descent from node 0 -- a node with a child enters child slot 4 s_x + 2 s_y + s_z when that slot is >= 0 and for every axis
 *   (s_k = 0 and blo_k < c_k) or (s_k = 1 and bhi_k >= c_k), c = the node's centre; a node WITHOUT children ends its branch, with flag 1
 *   if its trans_idx >= 0.  Nodes below depth 31 are not entered (f2n_oct_locate_warp reports their points empty).
 *   The flag is 1 iff some branch ends so.  This is conservative for the point rule p_k >= c_k of f2n_oct_locate_warp: a point of the
 *   box follows one of the branches its box follows, so every non-empty grid point lies in rows of flagged bricks only. */
int f2n_brick_mark(void* stream, const void* tree_nodes, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int B,
                   uint8_t* flags /*[nb_z*nb_y*nb_x]*/);
/* f2n_oct_locate_warp_grid for the corners of the n_bricks listed bricks: output row j (B + 1)^3 + l = local corner l of brick
 * brick_ids[j] (n_bricks (B + 1)^3 <= 2^31 - 1).  A corner that does not exist (or a brick id outside the grid) gets anchors
 * (-1, -1, 0) and warped (0, 0, 0), as an empty point. */
int f2n_oct_locate_warp_bricks(void* stream, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int B, int n_bricks,
                               const int32_t* brick_ids /*[n_bricks]*/, const void* tree_nodes, const void* transes,
                               float* out_pts_warped /*[n_bricks*(B+1)^3,3]*/, int32_t* out_anchors /*[n_bricks*(B+1)^3,3]*/);
/* The iso-surface of ANY values [n_bricks, (B + 1)^3] float32 of the listed bricks, count -> scan -> emit as f2n_mesh_count /
 * f2n_mesh_emit; one workgroup per brick, the brick's row staged in LDS; the inside test, edge types, tetrahedra, winding and vertex
 * position are f2n_mesh_emit's own device functions.
 * f2n_brick_mesh_count: vert_counts[j] / face_counts[j] = the vertices of the corners / the faces of the cells that brick j owns.
 * f2n_brick_mesh_emit: vert_start / face_start [n_bricks] int64 = the exclusive prefix sums of the counts (plus any offset of the
 *   caller's); brick j writes vert_keys, verts [.,3] from row vert_start[j] and face_keys, face_vert_keys [.,3] (the KEYS of a face's three
 *   vertices, wound as f2n_mesh_emit winds) from row face_start[j].  The order within a brick is fixed (local corner / cell index,
 *   then type / ordinal) but carries no meaning: keys are unique across bricks, and a caller sorts by them.
 * A brick id outside the grid owns nothing.  A face's vertex may be owned by another brick: the surface is complete only over a set
 * of bricks that holds the owner of every crossing edge of its cells (any set that holds every brick whose row has a value on
 * either side of the level does). */
int f2n_brick_mesh_count(void* stream, int nx, int ny, int nz, int B, int n_bricks, const int32_t* brick_ids /*[n_bricks]*/,
                         const float* values /*[n_bricks,(B+1)^3]*/, float level, int32_t* vert_counts /*[n_bricks]*/,
                         int32_t* face_counts /*[n_bricks]*/);
int f2n_brick_mesh_emit(void* stream, int nx, int ny, int nz, int B, int n_bricks, const int32_t* brick_ids /*[n_bricks]*/,
                        const float* values /*[n_bricks,(B+1)^3]*/, float level, const float* lo /*host [3]*/, float step,
                        const int64_t* vert_start /*[n_bricks]*/, const int64_t* face_start /*[n_bricks]*/, int64_t* vert_keys /*[nv]*/,
                        float* verts /*[nv,3]*/, int64_t* face_keys /*[nf]*/, int64_t* face_vert_keys /*[nf,3]*/);

/* ---------------------------------------------------------------------------------------------------
 * Sparse TSDF fusion on bricks (additive; the ABI version is unchanged): the mesh of f2n_tsdf_integrate -> f2n_tsdf_finalize ->
 * f2n_mesh_count_masked -> f2n_mesh_emit, bit for bit, from the bricks that saw a surface -- S, W, g and valid exist for one batch of
 * brick rows at a time.  No reference counterpart.  csrc/dataset.hip (mark, integrate), csrc/octree.hip (masked brick mesher);
 * tests/tsdf_sparse_ref.py restates the definitions in numpy.
 * The VIRTUAL GRID, the BRICKS (B in {4, 8, 16}, nb, linear ids, rows of (B + 1)^3 corners local x fastest, corners that DO NOT EXIST,
 * ownership) and the KEYS are those of "Sparse mesh extraction on bricks" above; views, depth, conf, trunc and the twelve steps are
 * those of f2n_tsdf_integrate.
 * A (grid point, view) pair is a HIT when the view passes steps 1-9 for the point, !(sdf < -trunc) (step 10) and sdf < 0: the point is
 * seen, and lies at most trunc behind that view's surface.  g > 0 at a valid point needs S < 0, which needs a hit; so every cell of the
 * masked mesh with a face, and every crossing edge with a vertex, has a corner with a hit, and its owner brick holds that corner in its
 * row: the bricks flagged by f2n_tsdf_brick_mark hold the owner of every face and every vertex of the dense TSDF mesh (level 0).
 * ------------------------------------------------------------------------------------------------- */
/* flags [nb_z nb_y nb_x] uint8: flags[b] = 1 iff some EXISTING corner of brick b's row has a hit in some view, else 0 -- exactly, not
 * a superset: steps 1-10 with the roundings, comparisons and NaN behaviour of f2n_tsdf_integrate (the same device function), then
 * sdf < 0 (false for NaN).  One workgroup per brick, views in groups in the outer loop with a block-wide vote after each group; no
 * atomics, a flag is written once.  The work is that of a dense integration, O(grid points x views): the pass saves memory, not
 * arithmetic.  n_views == 0: F2N_OK, nothing is touched.  F2N_ERR_INVALID_ARG: B outside {4, 8, 16}, n[k] outside
 * [2, F2N_BRICK_MAX_POINTS], a negative size, h or w outside [1, 2^24], trunc not positive and finite, a NULL pointer other than conf;
 * F2N_ERR_UNSUPPORTED: 2^31 bricks or more. */
int f2n_tsdf_brick_mark(void* stream, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int B, int n_views,
                        const float* poses /*[V,3,4]*/, const float* intri /*[V,3,3]*/, const float* dist_params /*[V,4]*/,
                        const float* depth /*[V,h,w]*/, const float* conf /*[V,h,w] or NULL*/, int h, int w, float trunc,
                        uint8_t* flags /*[nb_z*nb_y*nb_x]*/);
/* f2n_tsdf_integrate for the corners of the n_bricks listed bricks: S, W [n_bricks, (B + 1)^3] rows (n_bricks (B + 1)^3 <= 2^31 - 1),
 * row j (B + 1)^3 + l = local corner l of brick brick_ids[j], updated IN PLACE by the twelve steps, views in index order, one thread
 * per row entry, no atomics: the entry of an existing corner gets the bits the dense entry point gives that grid point from the same
 * state, and the views [0, k) then [k, V) give the bits of one call.  A corner that does not exist, and every corner of a brick id
 * outside the grid, is left untouched.  n_views == 0 or n_bricks == 0: F2N_OK, nothing is touched.  Error codes as
 * f2n_tsdf_brick_mark.  f2n_tsdf_finalize is flat over n and serves the rows unchanged. */
int f2n_tsdf_integrate_bricks(void* stream, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int B, int n_bricks,
                              const int32_t* brick_ids /*[n_bricks]*/, int n_views, const float* poses /*[V,3,4]*/,
                              const float* intri /*[V,3,3]*/, const float* dist_params /*[V,4]*/, const float* depth /*[V,h,w]*/,
                              const float* conf /*[V,h,w] or NULL*/, int h, int w, float trunc, float* S /*[n_bricks,(B+1)^3]*/,
                              float* W /*[n_bricks,(B+1)^3]*/);
/* f2n_brick_mesh_count / f2n_brick_mesh_emit with valid [n_bricks, (B + 1)^3] uint8 rows (non-zero = the corner carries a value; the
 * entry of a corner that does not exist is never read); the same device functions.  A cell has faces only if its eight corners are
 * valid.  A corner's owned edge yields a vertex iff it crosses the level AND both endpoints are valid -- a SUPERSET of
 * f2n_mesh_count_masked's rule, which also asks for an observed cell around the edge (cells on the low side, which a row does not
 * hold): every vertex a face names is emitted, and a caller that drops the vertices no face names after the key sort is left with
 * f2n_mesh_count_masked's set.  With valid all non-zero every output equals the unmasked entry point's bit for bit.  Error codes as the
 * unmasked entry points, plus F2N_ERR_INVALID_ARG for valid == NULL. */
int f2n_brick_mesh_count_masked(void* stream, int nx, int ny, int nz, int B, int n_bricks, const int32_t* brick_ids /*[n_bricks]*/,
                                const float* values /*[n_bricks,(B+1)^3]*/, const uint8_t* valid /*[n_bricks,(B+1)^3]*/, float level,
                                int32_t* vert_counts /*[n_bricks]*/, int32_t* face_counts /*[n_bricks]*/);
int f2n_brick_mesh_emit_masked(void* stream, int nx, int ny, int nz, int B, int n_bricks, const int32_t* brick_ids /*[n_bricks]*/,
                               const float* values /*[n_bricks,(B+1)^3]*/, const uint8_t* valid /*[n_bricks,(B+1)^3]*/, float level,
                               const float* lo /*host [3]*/, float step, const int64_t* vert_start /*[n_bricks]*/,
                               const int64_t* face_start /*[n_bricks]*/, int64_t* vert_keys /*[nv]*/, float* verts /*[nv,3]*/,
                               int64_t* face_keys /*[nf]*/, int64_t* face_vert_keys /*[nf,3]*/);

/* ---------------------------------------------------------------------------------------------------
 * View-colour fusion: the colours the views observed, blended onto surface points (additive; the ABI version is unchanged).  No
 * reference counterpart.  csrc/dataset.hip; tests/view_colors_ref.py restates the definitions in numpy.
 * ------------------------------------------------------------------------------------------------- */
/* Adds the observations of n_views views to the running sums acc [n,C] (sum of weight x colour), wsum [n] (sum of weight) and count [n]
 * (int32: the views that contributed) of n surface points.  points [n,3]; normals [n,3] or NULL: OUTWARD, as the exporters produce
 * them; a row that is all zero or has a component that is not finite means "no normal", and so does NULL.
 * The views are those of f2n_tsdf_integrate: poses [V,3,4], intri [V,3,3] in units of map pixels, dist_params [V,4], depth [V,h,w] (the
 * Euclidean distance to the surface; no surface where the value is not > 0), conf [V,h,w] or NULL (= 1); image [V,h,w,C] float32 on
 * the pixel grid of depth, C in [1, 4].
 * One thread owns one point p and walks the views in index order; every operation below is ONE fp32 rounding, never an FMA:
 *    1. steps 1-6 of f2n_tsdf_integrate unchanged (the same device function): q = p - o_v, c = R^T q, s = -c_2 (skip the view unless
 *       s > 0), u, v, the distortion, x, y;  r = f2n_norm3(q) = sqrt(q_0 q_0 + (q_1 q_1 + q_2 q_2))
 *    2. facing: with a normal n, cosv = (n_0 (-q_0) + (n_1 (-q_1) + n_2 (-q_2))) / r; skip unless cosv > cos_min (NaN skips);
 *       facing = cosv.  Without a normal, facing = 1 and no view is skipped here.
 *    3. taps: xs = x - 0.5, ys = y - 0.5, b0 = floor(xs), a0 = floor(ys), fx = xs - b0, fy = ys - a0; the four taps (a0 + i, b0 + j) in
 *       the order (i, j) = (0,0), (0,1), (1,0), (1,1) with the bilinear weights b = (i ? fy : 1 - fy) (j ? fx : 1 - fx) (a subtraction each,
 *       then the product).  A tap with a0 + i outside [0, h) or b0 + j outside [0, w) (compared as floats; NaN is outside) DOES NOT
 *       EXIST -- there is no observation beyond the image border, nothing is clamped.  An existing tap with D = its depth and cf = its
 *       conf (or 1) is VALID iff D > 0, cf > 0, !(D - r < -tol) and !(D - r > tol): the point lies on that pixel's visible surface
 *       within tol -- a point the view sees occluded is not valid, nor is one floating in front of what the view sees.  A tap's
 *       validity depends on its own depth only: colours do not bleed across a silhouette.
 *    4. weight: om_k = b_k cf_k of the valid taps; om = ((0 + om_k) + ...) over the valid taps in tap order; skip the view unless om > 0
 *    5. col_c = ((0 + om_k image_k,c) + ...) over the valid taps in tap order (image is read for valid taps only);
 *       acc_c += facing col_c;  wsum += facing om;  count += 1
 * acc, wsum and count are read once and written once per launch; there are no atomics, so the outputs are a function of the inputs
 * alone, and the views [0, k) followed by [k, V) into the same state give the bits of one call over [0, V).
 * The weighting is a CHOICE, not a measurement: confidence (the rendered opacity, where the maps are rendered) times the cosine of the
 * viewing angle, and a weighted mean over all views that see the point rather than the pick of a best view.
 * n == 0 or n_views == 0: F2N_OK, nothing is touched.  F2N_ERR_INVALID_ARG: a negative size, C outside [1, 4], h or w outside
 * [1, 2^24], tol not positive and finite, cos_min NaN, a NULL pointer other than normals and conf. */
int f2n_view_colors_accumulate(void* stream, int64_t n, const float* points /*[n,3]*/, const float* normals /*[n,3] or NULL*/,
                               int n_views, const float* poses /*[V,3,4]*/, const float* intri /*[V,3,3]*/,
                               const float* dist_params /*[V,4]*/, const float* depth /*[V,h,w]*/, const float* conf /*[V,h,w] or NULL*/,
                               const float* image /*[V,h,w,C]*/, int C, int h, int w, float tol, float cos_min, float* acc /*[n,C]*/,
                               float* wsum /*[n]*/, int32_t* count /*[n]*/);
/* The blended colour of the sums and where it is known: known[i] = (count[i] >= min_views && wsum[i] > 0);
 *   rgb[i,c] = known[i] ? acc[i,c] / wsum[i] : 0.   F2N_ERR_INVALID_ARG: n < 0, C outside [1, 4], a NULL pointer (n > 0). */
int f2n_view_colors_finalize(void* stream, int64_t n, int C, const float* acc /*[n,C]*/, const float* wsum /*[n]*/,
                             const int32_t* count /*[n]*/, int min_views, float* rgb /*[n,C]*/, uint8_t* known /*[n]*/);

/* ---------------------------------------------------------------------------------------------------
 * Mesh simplification by vertex clustering with quadric-error placement (additive; the ABI version is unchanged).  Lindstrom 2000
 * with Garland-Heckbert plane quadrics.  No reference counterpart.  csrc/octree.hip.
 * ------------------------------------------------------------------------------------------------- */
/* The cluster grid: origin lo (HOST [3], finite), cell size `cell` (finite, > 0), dims (HOST [3], each in [1, 2^20]).  Every call below
 * returns F2N_ERR_INVALID_ARG for a grid outside these ranges, a negative size or a NULL pointer it needs.  All fp32 operations are ONE
 * rounding each, never an FMA; "fp64" likewise.
 *   cell of a point p:   u_k = (p_k - lo_k) / cell;  i_k = min(max(floor(u_k), 0), dims_k - 1)        (clamped as floats, then cast)
 *   centre of cell i:    c_k = lo_k + ((float) i_k + 0.5) * cell
 *   local coordinates:   q_k = min(max((p_k - c_k) / cell, -0.5), 0.5)   -- the clamp only acts on the last bit of a vertex on its
 *                        cell's border and on vertices that the grid does not cover (which the dims clamp pulled into a border cell)
 *   quant(x) = __double2ll_rn((double) x * 2^40)    (round to nearest even; the product is exact)
 * f2n_mesh_cluster_keys: keys[v] = ((int64) i_z * dims_y + i_y) * dims_x + i_x, or -1 for a vertex with a coordinate that is not finite.
 *
 * The caller numbers the occupied keys in ascending order: cluster ids 0..C-1, cluster_keys [C] int64 = those keys, cluster_of [V] int32
 * = the id of every vertex's key, -1 for key -1 (a sorted unique with its inverse: plumbing, not a kernel here).
 *
 * f2n_mesh_cluster_accumulate: acc [C,16] int64, ZEROED BY THE CALLER, receives exact integer sums (64-bit integer atomics that wrap):
 *   slots 0..5 = sum of quant(w n_i n_j) for (i,j) = xx, xy, xz, yy, yz, zz;  6..8 = sum of quant(w d n_i);  9 = sum of quant(w d d);
 *   10 = sum of quant(w);  11 = corner records;  12..14 = sum of quant(q_k) over the cluster's vertices;  15 = its vertex count.
 *   Per vertex v with cluster_of[v] >= 0: q of p_v in its own cell -> slots 12..15 of its cluster.
 *   Per face (a, b, c), all fp32:  e1 = (p_b - p_a) / cell, e2 = (p_c - p_a) / cell (componentwise: a subtraction, a division);
 *     n = (e1_y e2_z - e1_z e2_y, e1_z e2_x - e1_x e2_z, e1_x e2_y - e1_y e2_x);  l = sqrt((n_x n_x + n_y n_y) + n_z n_z);
 *     the face contributes nothing if an index is outside [0, V), a corner has cluster_of < 0, or l is zero or not finite.
 *     w = min(l * 0.5, 16);  u_k = n_k / l;  wu_k = w * u_k;  A_ij = wu_i * u_j.
 *     For each corner x of the face, with q = the local coordinates of p_x in ITS OWN cell:  d = -((u_x q_x + u_y q_y) + u_z q_z);
 *     wd = w * d;  b_k = wd * u_k;  cc = wd * d;  quant of (A_xx..A_zz, b_x, b_y, b_z, cc, w) and a 1 go to slots 0..11 of the corner's
 *     cluster.  |q_k| <= 0.5 bounds |d| by 0.87 and every summand by 16 (1 + 2^-20).
 *   Lanes of a wave that add to the same cluster are summed first (integers: the order is immaterial), one row segment of atomics per
 *   cluster and wave.  The sums are integers, so acc does not depend on face order, vertex numbering, scheduling or run.
 *   Guard: if a cluster holds more than 2^18 corner records or more than 2^18 vertices, the call returns F2N_ERR_UNSUPPORTED (below
 *   that, 2^18 * 16 (1 + 2^-20) * 2^40 < 2^63: no sum wraps).  `flag` is one DEVICE word of scratch; the call READS IT BACK, so it
 *   synchronises the stream.
 *
 * f2n_mesh_cluster_place: out_verts [C,3] f32, one thread per cluster, fp64 in this order (s = 2^-40, exact):
 *   cnt = (double) acc[15];  m_k = ((double) acc[12+k] * s) / cnt;  W = (double) acc[10] * s;  A.. = (double) acc[0..5] * s;
 *   b_k = (double) acc[6+k] * s.   If W > 0:  g = lambda * W;  M = A with g added to xx, yy, zz;  r_k = g * m_k - b_k;
 *     the cofactors  C00 = Myy Mzz - Myz Myz,  C01 = Mxz Myz - Mxy Mzz,  C02 = Mxy Myz - Mxz Myy,  C11 = Mxx Mzz - Mxz Mxz,
 *                    C12 = Mxy Mxz - Mxx Myz,  C22 = Mxx Myy - Mxy Mxy;    det = Mxx C00 + (Mxy C01 + Mxz C02);
 *     t_x = C00 r_x + (C01 r_y + C02 r_z),  t_y = C01 r_x + (C11 r_y + C12 r_z),  t_z = C02 r_x + (C12 r_y + C22 r_z);  q*_k = t_k / det.
 *     M is symmetric positive definite (A is a sum of w u u^T), so there is no rank decision and no threshold; only if the rounded
 *     det is not a positive finite number (sums of a few 2^-40 quanta) does q* fall back to m, as it does for W = 0.
 *   q*_k = min(max(q*_k, -0.5), 0.5);  out_k = c_k + cell * (float) q*_k   (c = the centre of the cell of cluster_keys[c], fp32).
 *   lambda (a double, >= 0 and finite) ties the minimiser to the mean of the cluster's vertices where the planes leave it free.
 *
 * f2n_mesh_cluster_faces: out_faces [F,3] int32 = the corners' cluster ids rotated so that the smallest comes first (orientation
 *   kept), or (-1, -1, -1) for a dropped face: an index outside [0, V), a cluster id of -1, or two equal ids.  The caller merges equal
 *   rows and sorts them lexicographically (a unique over rows: plumbing), so a face and its reversed twin both survive -- a wall
 *   thinner than a cell becomes a two-sided sheet, not a hole -- and then drops the clusters no face uses, keeping their order
 *   (f2n_mesh_filter_count with all labels 0 and min_faces 1, f2n_mesh_filter_emit). */
int f2n_mesh_cluster_keys(void* stream, int n_verts, const float* verts /*[V,3]*/, const float* lo /*host [3]*/, float cell,
                          const int32_t* dims /*host [3]*/, int64_t* keys /*[V]*/);
int f2n_mesh_cluster_accumulate(void* stream, int n_verts, int n_faces, const float* verts /*[V,3]*/, const int32_t* faces /*[F,3]*/,
                                const int32_t* cluster_of /*[V]*/, int n_clusters, const float* lo /*host [3]*/, float cell,
                                const int32_t* dims /*host [3]*/, int64_t* acc /*[C,16], zeroed*/, int32_t* flag /*[1]*/);
int f2n_mesh_cluster_place(void* stream, int n_clusters, const int64_t* acc /*[C,16]*/, const int64_t* cluster_keys /*[C]*/,
                           const float* lo /*host [3]*/, float cell, const int32_t* dims /*host [3]*/, double lambda,
                           float* out_verts /*[C,3]*/);
int f2n_mesh_cluster_faces(void* stream, int n_verts, int n_faces, const int32_t* faces /*[F,3]*/, const int32_t* cluster_of /*[V]*/,
                           int32_t* out_faces /*[F,3]*/);

/* ---------------------------------------------------------------------------------------------------
 * Ray casting against a triangle mesh (additive; the ABI version is unchanged).  The Woop-Benthin-Wald watertight test with the edge
 * functions in fp64.  No reference counterpart.  csrc/octree.hip.
 * ------------------------------------------------------------------------------------------------- */
/* A ray is x = o + t d; d need not be unit length and t counts in units of d.  Its window (t_min, t_max) is bounds[r] or (0, +inf) for
 * bounds == NULL.  For ray r and face (a, b, c) with vertices A, B, C every operation is ONE rounding of the stated width, never an FMA:
 *   1. kz = the axis of the largest |d_k|, the first among equals in the order x, y, z (kz = 0; |d_1| > |d_kz|: kz = 1; |d_2| > |d_kz|:
 *      kz = 2); kx = (kz + 1) % 3, ky = (kz + 2) % 3, swapped when d_kz < 0.  A ray with a component of d that is not finite, or with
 *      d_kz == 0, hits nothing.
 *   2. fp32: Sx = d_kx / d_kz, Sy = d_ky / d_kz, Sz = 1 / d_kz.
 *   3. per vertex P, fp32: q = P - o;  x = q_kx - Sx q_kz;  y = q_ky - Sy q_kz;  z = Sz q_kz.
 *   4. fp64: U = Cx By - Cy Bx;  V = Ax Cy - Ay Cx;  W = Bx Ay - By Ax  (the products of two floats are exact: every sign is exact).
 *   5. inside iff (U, V, W all >= 0 or all <= 0) and det = (U + V) + W != 0  (a NaN is outside).
 *   6. fp64: T = (U Az + V Bz) + W Cz;  t = (float) (T / det);  accepted iff t_min < t < t_max (a NaN fails).
 *   7. bary = ((float) (U / det), (float) (V / det), (float) (W / det)).
 *   8. the ray's result is its accepted face of the smallest t, of the lowest index among equal t: out_t, out_face, out_bary [R,3];
 *      no accepted face: face = -1, t = 0, bary = 0.
 * Consequences: two faces that share an edge see the same two transformed vertices and edge functions of exactly opposite sign, so
 * no ray passes between them; a degenerate face (det == 0) and a face with a vertex that is not finite (t is a NaN) are never hit.
 * The outputs of a ray are a function of that ray and the face list alone: not of the grid, its cell size, the rays' order or the
 * schedule (no atomics: one lane owns one ray).
 *
 * The acceleration grid: origin lo (HOST [3]), cell size `cell`, dims (HOST [3]) as for f2n_mesh_cluster_keys, and additionally
 * dims_x dims_y dims_z <= 2^27 (F2N_ERR_INVALID_ARG beyond).  i_k(p) = min(max(floor((p - lo_k) / cell), 0), dims_k - 1) (two fp32
 * roundings, clamped as floats) is the cell of a coordinate; guard = cell * 2^-4.
 *   f2n_mesh_raycast_count: counts [F] int32 = the number of cells that list face f: the box i_k(min_k - guard) .. i_k(max_k + guard) per
 *     axis (min / max over its three vertices, one fp32 rounding each); 0 for a face with a vertex that is not finite.  A face index
 *     outside [0, V): F2N_ERR_INVALID_ARG.  `flag` is one DEVICE word of scratch; the call READS IT BACK, so it synchronises the stream.
 *   The caller forms offsets [F] int64 = the exclusive prefix sum of counts (plumbing), E = their total.
 *   f2n_mesh_raycast_fill: keys [E] int64; face f writes (((int64) z dims_y + y) dims_x + x) * F + f for its cells (z, then y, then x
 *     ascending) from keys[offsets[f]] on.  No atomics: keys is a function of the inputs.
 *   The caller sorts keys ascending, cell_faces [E] int32 = key % F, cell_start [ncells + 1] int32 = the first position whose key is
 *     >= cell * F (a searchsorted: plumbing).  E must fit an int32.
 * f2n_mesh_raycast with cell_start == NULL (lo, cell, dims, cell_faces are then not read) is the BRUTE-FORCE mode: every ray tests every
 * face (a block stages 256 faces at a time in LDS).  Otherwise one lane per ray walks the grid's layers along kz in the ray's
 * direction; in layer L (planes z0 = lo_kz + L cell, z1 = lo_kz + (L + 1) cell; "in" the one the ray meets first) with q = z - o_kz:
 *     t_in = Sz q_in, t_out = Sz q_out;  margin = |Sz| guard
 *     stop if t_in - margin > t_max, or if a face is held and its t < t_in - margin;  skip the layer if t_out + margin < t_min
 *     x_in = o_kx + Sx q_in, x_out = o_kx + Sx q_out (likewise y): the cells i_kx(min(x_in, x_out) - guard) .. i_kx(max + guard) times the
 *     same range in ky are tested, every face of their lists by the steps above.
 *   Domain (DESIGN.md section 3 gives the argument): every face vertex lies inside the grid box, and M = the largest absolute value among
 *   the coordinates of lo, lo + dims cell and the ray origins is at most 2^15 cell.  Within it the traversal tests every face that the
 *   brute-force mode could return, ties of equal t included, so the two modes agree bit for bit.  The box part of the domain is checked
 *   here (F2N_ERR_UNSUPPORTED); the origins are device data and are the caller's to check (the host layer does, with one reduction).
 * A face index outside [0, V): F2N_ERR_INVALID_ARG (out_face[0] is the flag word of that check before the rays are cast; the call READS
 * IT BACK, so it synchronises the stream).  n_rays == 0: F2N_OK, nothing is touched.  F == 0: every ray misses. */
int f2n_mesh_raycast_count(void* stream, int n_verts, int n_faces, const float* verts /*[V,3]*/, const int32_t* faces /*[F,3]*/,
                           const float* lo /*host [3]*/, float cell, const int32_t* dims /*host [3]*/, int32_t* counts /*[F]*/,
                           int32_t* flag /*[1]*/);
int f2n_mesh_raycast_fill(void* stream, int n_verts, int n_faces, const float* verts /*[V,3]*/, const int32_t* faces /*[F,3]*/,
                          const float* lo /*host [3]*/, float cell, const int32_t* dims /*host [3]*/, const int64_t* offsets /*[F]*/,
                          int64_t* keys /*[E]*/);
int f2n_mesh_raycast(void* stream, int n_verts, int n_faces, const float* verts /*[V,3]*/, const int32_t* faces /*[F,3]*/,
                     const float* lo /*host [3]*/, float cell, const int32_t* dims /*host [3]*/, const int32_t* cell_start /*[ncells+1] or NULL*/,
                     const int32_t* cell_faces /*[E]*/, int n_rays, const float* rays_o /*[R,3]*/, const float* rays_d /*[R,3]*/,
                     const float* bounds /*[R,2] or NULL*/, float* out_t /*[R]*/, int32_t* out_face /*[R]*/, float* out_bary /*[R,3]*/);

/* ---------------------------------------------------------------------------------------------------
 * Closest point on a triangle mesh (additive; the ABI version is unchanged): the region walk of Ericson, "Real-Time Collision
 * Detection" 5.1.5, in fp64 over the ray caster's face grid.  No reference counterpart.  csrc/octree.hip; tests/mesh_distance_ref.py
 * restates it in numpy.
 * ------------------------------------------------------------------------------------------------- */
/* For point p and face (a, b, c) with vertices A, B, C, all converted to fp64, every operation ONE fp64 rounding, never an FMA, a dot
 * product being (x x' + y y') + z z':
 *   1. ab = B - A, ac = C - A;  d1 = ab.(p - A), d2 = ac.(p - A);  d3 = ab.(p - B), d4 = ac.(p - B);  d5 = ab.(p - C), d6 = ac.(p - C).
 *   2. the weights (u, v, w) of (A, B, C) by the FIRST of these tests that holds (a NaN fails every one of them):
 *        vertex A: d1 <= 0 and d2 <= 0: (1, 0, 0);   vertex B: d3 >= 0 and d4 <= d3: (0, 1, 0);   vertex C: d6 >= 0 and d5 <= d6: (0, 0, 1);
 *        with vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, g = d4 - d3, k = d5 - d6:
 *        edge AB: vc <= 0, d1 >= 0, d3 <= 0: v = d1 / (d1 - d3), (1 - v, v, 0);
 *        edge AC: vb <= 0, d2 >= 0, d6 <= 0: w = d2 / (d2 - d6), (1 - w, 0, w);
 *        edge BC: va <= 0, g >= 0, k >= 0:   w = g / (g + k), (0, 1 - w, w);
 *        interior: s = (va + vb) + vc, v = vb / s, w = vc / s, u = (1 - v) - w.
 *   3. q = (u A + v B) + w C per coordinate;  e = p - q;  d2 = (e_x e_x + e_y e_y) + e_z e_z.
 *   4. the point's result is its face of the smallest d2, of the lowest index among equal d2; a d2 that is NaN or +inf never wins (a
 *      face with a vertex that is not finite, a degenerate face whose walk divides 0 by 0; a degenerate face whose walk stays finite
 *      gives the true distance to one of its points and may win).  out_dist = (float) sqrt(d2) (fp64 sqrt, correctly rounded),
 *      out_face, out_bary [N,3] = ((float) u, (float) v, (float) w).
 *   5. nothing wins, out_dist > max_dist, or p has a coordinate that is not finite: face = -1, dist = +inf, bary = 0.
 * The outputs of a point are a function of that point, max_dist and the face list alone: not of the grid, its cell size, the points'
 * order or the schedule (no atomics: one lane owns one point).
 *
 * cell_start == NULL (lo, cell, dims, cell_faces are then not read) is the BRUTE-FORCE mode: every point tests every face (a block stages
 * 256 faces at a time in LDS).  Otherwise (lo, cell, dims, cell_start, cell_faces) is the grid of f2n_mesh_raycast_count / _fill above and
 * one lane per point walks Chebyshev shells around the point's own cell c_k = i_k(p_k): shell r = the cells of the clamped box
 * [max(c - r, 0), min(c + r, dims - 1)] that are not in box r - 1; every face of their lists is tested by steps 1-4.  After shell r, in
 * fp32 with one rounding per operation:
 *     LB = the minimum over the OPEN sides of the box of the distance from p to the side's plane:
 *       low side of axis k, open iff c_k - r > 0:            p_k - (lo_k + (float) (c_k - r) cell)
 *       high side of axis k, open iff c_k + r < dims_k - 1:  (lo_k + (float) (c_k + r + 1) cell) - p_k
 *     no side open: stop (every cell has been tested);  stop iff (a face is held and (float) sqrt(d2) < LB) or LB > max_dist.
 *   A term is negative for a point outside the grid on that side, which keeps the walk going.
 *   Domain (DESIGN.md section 3 gives the argument): every finite vertex lies inside the grid box, and M = the largest absolute value
 *   among the coordinates of lo, lo + dims cell and the points is at most 2^15 cell.  Within it a face that no cell of the box lists lies
 *   at least guard = cell 2^-4 beyond an open plane, which pays for the roundings of LB and of dist: the walk tests every face that the
 *   brute-force mode could return, ties included, so the two modes agree bit for bit.  The box part of the domain (F2N_ERR_UNSUPPORTED)
 *   and the vertices (F2N_ERR_UNSUPPORTED for a finite vertex outside [lo_k - guard, lo_k + dims_k cell + guard]) are checked here; the
 *   points are device data and are the caller's to check (the host layer does, with one reduction).
 * max_dist must be >= 0 (+inf: no cut-off), F2N_ERR_INVALID_ARG otherwise.  A face index outside [0, V): F2N_ERR_INVALID_ARG.
 * out_face[0] and out_dist[0] are the flag words of the two checks before the points are processed; the call READS THEM BACK, so it
 * synchronises the stream.  n_points == 0: F2N_OK, nothing is touched.  F == 0: every point misses. */
int f2n_mesh_closest_point(void* stream, int n_verts, int n_faces, const float* verts /*[V,3]*/, const int32_t* faces /*[F,3]*/,
                           const float* lo /*host [3]*/, float cell, const int32_t* dims /*host [3]*/,
                           const int32_t* cell_start /*[ncells+1] or NULL*/, const int32_t* cell_faces /*[E]*/, int n_points,
                           const float* points /*[N,3]*/, float max_dist, float* out_dist /*[N]*/, int32_t* out_face /*[N]*/,
                           float* out_bary /*[N,3]*/);

/* ---------------------------------------------------------------------------------------------------
 * Area-uniform surface samples of a triangle mesh (additive; the ABI version is unchanged): stratified over the faces' areas, drawn
 * by the keyed Philox4x32-10.  No reference counterpart.  csrc/octree.hip; tests/mesh_distance_ref.py restates it in numpy.
 * ------------------------------------------------------------------------------------------------- */
/* f2n_mesh_face_weights: per face, fp64 from the fp32 coordinates, one rounding per operation: p = B - A, q = C - A,
 *   n = (p_y q_z - p_z q_y, p_z q_x - p_x q_z, p_x q_y - p_y q_x), area2 [F] = sqrt((n_x n_x + n_y n_y) + n_z n_z) (twice the area;
 *   correctly rounded); 0 for a face with an index outside [0, V) or a vertex that is not finite.  With weights != NULL also
 *   weights [F] int64 = (int64) floor(area2 / quantum) (quantum > 0 and finite, F2N_ERR_INVALID_ARG otherwise).  Either output may be NULL.
 * The caller's plumbing: quantum = max_f area2_f 2^-31 (a max is order-free; the largest weight is 2^31), cum [F] int64 = the inclusive
 *   prefix sum of the weights, T = cum[F - 1] (exact).  T == 0 (no face with an area) is the caller's error to report.
 * f2n_mesh_sample_surface: sample j of n, one lane each, a pure function of (mesh, n, key, j):
 *   x = Philox4x32-10 of counter (j, 0, 0, 0) under `key` (low word, high word), key = seed ^ purpose as host/KeyedDraws.h forms keys;
 *   fp64: target = min((int64) floor(((double) j + (x0 + 0.5) 2^-32) / (double) n * (double) T), T - 1);
 *   face = the first f with cum[f] > target (a binary search; a face of weight 0 is never drawn);
 *   fp64: s = sqrt((x1 + 0.5) 2^-32), r = (x2 + 0.5) 2^-32;  bary = ((float) (1 - s), (float) (s (1 - r)), (float) (s r));
 *   point = (b0 A + b1 B) + b2 C per coordinate in fp32 from the fp32 bary.
 *   Stratum j holds one target, so the number of samples on face f differs from n w_f / T by less than 2 (up to the fp64 roundings of
 *   the target, which move it by less than 2^-52 T).  cum must be non-decreasing with cum[F - 1] > 0; n > 0 with F == 0 or V == 0 is
 *   F2N_ERR_INVALID_ARG.  n == 0: F2N_OK, nothing is touched. */
int f2n_mesh_face_weights(void* stream, int n_verts, int n_faces, const float* verts /*[V,3]*/, const int32_t* faces /*[F,3]*/,
                          double quantum, double* area2 /*[F] or NULL*/, int64_t* weights /*[F] or NULL*/);
int f2n_mesh_sample_surface(void* stream, int n_verts, int n_faces, const float* verts /*[V,3]*/, const int32_t* faces /*[F,3]*/,
                            const int64_t* cum /*[F]*/, int n_samples, uint64_t key, float* out_points /*[n,3]*/, int32_t* out_face /*[n]*/,
                            float* out_bary /*[n,3]*/);

/* ---------------------------------------------------------------------------------------------------
 * Texture atlas of a triangle mesh (additive; the ABI version is unchanged): one right-triangle chart per face, two charts to a
 * square block of 2^k texels a side, blocks placed by the Morton decode of a prefix sum; the texel-to-surface map; a bilinear
 * lookup.  No reference counterpart.  csrc/octree.hip.  Every operation is ONE rounding of the stated width, never an FMA, and one
 * lane owns one output: nothing depends on the schedule.  tests/atlas_ref.py restates all of it in numpy.
 * ------------------------------------------------------------------------------------------------- */
/* f2n_atlas_classify: no reference counterpart.  Per face (a, b, c) with vertices A, B, C, all in fp64 from the fp32 coordinates:
 *   p = B - A, q = C - A, e = C - B (per coordinate: (double) x - (double) y);
 *   |AB|^2 = (p_x p_x + p_y p_y) + p_z p_z, likewise |BC|^2 from e and |CA|^2 from q;
 *   n = (p_y q_z - p_z q_y, p_z q_x - p_x q_z, p_x q_y - p_y q_x);  n2 = (n_x n_x + n_y n_y) + n_z n_z  (= (2 area)^2);
 *   l = sqrt(sqrt(n2)) * (double) density  (the leg, in texels, of the right isosceles triangle of the face's area);
 *   need = max(4, ceil(l) + 3);  log_s = the smallest k in [2, max_log] with 2^k >= need, max_log if there is none.
 *   rot in {0, 1, 2} = the face's corner opposite its longest edge (corner 0 faces BC, 1 faces CA, 2 faces AB), the first among
 *   equals in the order 0, 1, 2: r = 0; |CA|^2 > |BC|^2: r = 1; |AB|^2 > that maximum: r = 2.  Chart corner k (0: the right angle,
 *   1: along x, 2: along y) is the face's corner (rot + k) % 3: a cyclic shift, so the orientation is kept.
 *   A face with an index outside [0, V), a vertex that is not finite or n2 == 0 is DEGENERATE: log_s = 2, rot = 4 (bit 2 of rot is
 *   the flag, its rotation is 0).  It keeps a slot in the atlas and gets uv, but owns no texel.  It is never an error.
 * density must be positive and finite, 2 <= max_log <= 13: F2N_ERR_INVALID_ARG otherwise.
 *
 * The caller's plumbing between the calls (sort, prefix sums: host/RendererQuery.cpp MeshAtlas, capi.mesh_atlas):
 *   order: the faces sorted by the int64 key (max_log - log_s) F + f: classes descending, faces ascending within a class;
 *   positions 2j and 2j + 1 of a class share its block j, the first as the LOWER chart, the second as the UPPER one (a class with an
 *   odd count leaves its last upper slot empty); blocks are numbered through the classes in that order;
 *   slot [F] int32 = 2 block + upper;  block_log [B] int32;  block_faces [B,2] int32 (lower, upper; -1: empty);
 *   offsets [B + 1] int64 = the exclusive prefix sum of 4^block_log (sizes descend, so every offset is a multiple of its block's area);
 *   a block's origin (x0, y0) = the Morton decode of its offset (even bits -> x, odd bits -> y);
 *   size S = the smallest power of two with S^2 >= offsets[B], at least 4 (and at most 8192 = 2^13).
 * f2n_atlas_place: no reference counterpart.  uv [F,3,2] fp32 in the order of the face's own corners, image convention (x right, y
 *   down), = (origin + chart corner) / S, in fp32: the sum and the division by a power of two are exact.  With s = 2^log_s the
 *   chart corners in texels from the origin are  lower: (0.5, 0.5), (s - 2.5, 0.5), (0.5, s - 2.5);  upper: (s - 0.5, s - 0.5),
 *   (2.5, s - 0.5), (s - 0.5, 2.5): legs of s - 3 texels between texel centres.  The bilinear footprint of the lower chart lies in the
 *   texels i + j <= s - 2 of the block, that of the upper chart in i + j >= s; the diagonal i + j = s - 1 is a gutter of the lower one.
 *   A face whose slot is negative or names no block gets zeros.  size must be a power of two in [4, 8192]: F2N_ERR_INVALID_ARG.
 * f2n_atlas_texels: no reference counterpart.  One lane per texel (x, y) of the rows [row_begin, row_end) (a wave owns an 8 x 8 tile);
 *   the other rows are not touched.  m = the Morton code of (x, y); no block if m >= offsets[B], else block = the last one with
 *   offsets[block] <= m (a binary search), s = 2^block_log, i = x - x0, j = y - y0.  Lower chart iff i + j <= s - 1, with
 *   (u, v) = ((float) i / (float) (s - 3), (float) j / (float) (s - 3)); else upper, from (s - 1 - i, s - 1 - j) likewise.
 *   Raw weights of the chart corners, fp32: w0 = (1 - u) - v, w1 = u, w2 = v; the face's corner j carries w of chart corner
 *   (j - rot) mod 3: (b0, b1, b2).  clamp == 1 and some b < 0 (a gutter texel): b_k = max(b_k, 0), sum = (b0 + b1) + b2, b_k = b_k / sum;
 *   with no negative weight, and for clamp == 0 always, the weights stay raw (gutter texels then extrapolate, so that bilinear
 *   filtering reproduces a linear function of position everywhere inside a chart).
 *   tex_face [S,S] int32 = the face, or -1 with zero weights and position where there is no block, an empty slot, a slot whose face
 *   index is outside [0, F) or a degenerate face;  tex_bary [S,S,3] = (b0, b1, b2), the weights tex_pos was blended with;
 *   tex_pos [S,S,3]: per coordinate (b0 A + b1 B) + b2 C in fp32 (three products, two sums).
 *   clamp other than 0 / 1, rows outside [0, S]: F2N_ERR_INVALID_ARG.
 * f2n_texture_sample: no reference counterpart.  out [N,C] = the bilinear lookup of tex [S,S,C] (row y, column x) at uv [N,2] = (x, y)
 *   with texel centres at (i + 0.5) / S, clamped to the edge; S in [1, 32768] need not be a power of two, C in [1, 64].  fp32:
 *   fx = min(max(u S - 0.5, 0), S - 1) (a product, a difference), x0 = floor(fx), x1 = min(x0 + 1, S - 1), ax = fx - x0, cx = 1 - ax;
 *   likewise fy, y0, y1, ay, cy from v;  out = ((t00 (cx cy) + t10 (ax cy)) + t01 (cx ay)) + t11 (ax ay) with t10 = tex[y0][x1],
 *   t01 = tex[y1][x0].  A row whose u or v is not finite gives zeros. */
int f2n_atlas_classify(void* stream, int n_verts, int n_faces, const float* verts /*[V,3]*/, const int32_t* faces /*[F,3]*/, float density,
                       int max_log, int32_t* log_s /*[F]*/, int32_t* rot /*[F]*/);
int f2n_atlas_place(void* stream, int n_faces, int n_blocks, int size, const int32_t* log_s /*[F]*/, const int32_t* rot /*[F]*/,
                    const int32_t* slot /*[F]*/, const int64_t* offsets /*[B+1]*/, float* uv /*[F,3,2]*/);
int f2n_atlas_texels(void* stream, int n_verts, int n_faces, const float* verts /*[V,3]*/, const int32_t* faces /*[F,3]*/, int n_blocks,
                     int size, const int64_t* offsets /*[B+1]*/, const int32_t* block_log /*[B]*/, const int32_t* block_faces /*[B,2]*/,
                     const int32_t* rot /*[F]*/, int clamp, int row_begin, int row_end, int32_t* tex_face /*[S,S]*/,
                     float* tex_bary /*[S,S,3]*/, float* tex_pos /*[S,S,3]*/);
int f2n_texture_sample(void* stream, int size, int channels, const float* tex /*[S,S,C]*/, int64_t n, const float* uv /*[N,2]*/,
                       float* out /*[N,C]*/);

/* ---------------------------------------------------------------------------------------------------
 * SSIM of two images (additive; the ABI version is unchanged): the reference's rgb_ssim (scripts/eval.py:29-75, the mip-NeRF definition),
 * "valid" mode, in fp64 with a fixed order of operations and an exact integer sum for the mean.  csrc/dataset.hip; tests/ssim_ref.py
 * restates it in numpy.
 * ------------------------------------------------------------------------------------------------- */
/* f2n_ssim_window (HOST only, no launch; scripts/eval.py:40-45): out [fs] doubles, every operation one fp64 rounding:
 *   hw = fs / 2 (integer), shift = (2 hw - fs + 1) / 2 (0 for an odd fs, 0.5 for an even one), u_i = ((i - hw) + shift) / sigma,
 *   e_i = exp(-0.5 (u_i u_i)) (the C library's exp), s = the sum of e_i in ascending i from 0, out_i = e_i / s.
 *   The window is symmetric: out_i == out_(fs-1-i).  fs in [1, 33] of either parity, sigma > 0 and finite: F2N_ERR_INVALID_ARG otherwise.
 *   Its own entry point so that every binding passes the same doubles to f2n_image_ssim.
 * f2n_image_ssim (scripts/eval.py:47-73): a, b [H,W,C] fp32 on the device, window [fs] doubles on the HOST (they travel as kernel
 *   arguments), stats [C][2] int64 on the device, map [H-fs+1, W-fs+1, C] doubles on the device or NULL.  Per channel, with
 *   x = (double) a, y = (double) b, everything in fp64, never an FMA:
 *   1. five planes x, y, x x, y y, x y (a product of two floats is exact in fp64);
 *   2. each plane z is blurred down the columns first, V[i][j] = B_k z[i + k][j], then along the rows, B(z)[i][j] = B_k V[i][j + k]
 *      (the order of the reference's two convolve2d calls), where B_k t_k is: acc = 0; for k = 0 .. fs-1 ascending: acc = acc + w[k] t_k,
 *      each product and each sum rounded once.  The window is symmetric, so this correlation IS the reference's convolution;
 *   3. mu0 = B(x), mu1 = B(y);  mu00 = mu0 mu0, mu11 = mu1 mu1, mu01 = mu0 mu1;
 *      s00 = B(x x) - mu00, s11 = B(y y) - mu11, s01 = B(x y) - mu01;  s00 = (s00 < 0 ? 0 : s00), s11 likewise (a NaN stays a NaN);
 *      t = sqrt(s00 s11) (IEEE), m = (t < |s01| ? t : |s01|), s01 = (s01 < 0 ? -m : m);
 *      v = ((2 mu01 + c1) (2 s01 + c2)) / (((mu00 + mu11) + c1) ((s00 + s11) + c2)) (IEEE division);
 *   4. map[i][j][c] = v if map != NULL;
 *   5. v finite: stats[c][0] += llrint(v 2^36) (round half to even; |v| <= 1 by the clip of step 3), stats[c][1] += 1.  A v that is not
 *      finite (a NaN or inf pixel under the window) adds to neither and is written to the map as it is.  The sums are exact int64 sums.
 *   Properties: a == b gives v == 1.0 exactly at every output (numerator and denominator are then the same two factors);  stats and map are
 *   functions of the two images, the window, c1 and c2 alone: not of the grid, the tile size or the order in which blocks run;  whether
 *   the map is requested does not change stats.  The caller's mean of channel c is stats[c][0] / (2^36 stats[c][1]).
 *   The call zeroes stats itself on `stream` before the launch.  C in [1, 4], 1 <= fs <= min(H, W, 33), (H-fs+1)(W-fs+1) <= 2^26:
 *   F2N_ERR_INVALID_ARG otherwise, as for a NULL a, b, window or stats.
 * f2n_ssim_tile (HOST only): the kernel's output tile (rows, columns), for tests that want shapes at its edges. */
int f2n_ssim_window(int filter_size, double sigma, double* out /*host [fs]*/);
int f2n_image_ssim(void* stream, int height, int width, int channels, const float* a /*[H,W,C]*/, const float* b /*[H,W,C]*/,
                   const double* window /*host [fs]*/, int filter_size, double c1, double c2, double* map_or_null /*[H-fs+1,W-fs+1,C]*/,
                   int64_t* stats /*device [C][2]*/);
void f2n_ssim_tile(int* tile_h /*host*/, int* tile_w /*host*/);

/* ---------------------------------------------------------------------------------------------------
 * Mesh refinement (additive; the ABI version is unchanged): the vertex one-ring, Taubin smoothing, the projection of points onto a
 * level set of ln(sigma), face quality.  No reference counterpart.  csrc/octree.hip.  Every fp32 and every fp64 operation below is ONE
 * rounding, never an FMA; the kernels use + - * / sqrt only.  Every call returns F2N_ERR_INVALID_ARG for a negative size or a NULL
 * pointer it needs, and F2N_OK without touching anything when it has no element to work on.
 * ------------------------------------------------------------------------------------------------- */
/* The one-ring of every vertex as a CSR.  A face is VALID if its three indices lie in [0, V) and are pairwise distinct; any other face
 * contributes nothing.
 * f2n_mesh_ring_keys: keys [F,6] int64.  A valid face (a, b, c) writes the directed edges a V + b, b V + a, b V + c, c V + b, c V + a,
 *   a V + c (int64 products) in this order, any other face six times -1.  F <= (2^31 - 1) / 6.
 * The caller sorts all keys ascending, drops the -1s and run-length encodes the rest (plumbing, not a kernel here): edge_keys [E] int64
 *   = the distinct keys ascending, edge_uses [E] int64 = how often each occurs = the number of valid faces on the undirected edge
 *   (a face holds an edge once, in both directions).  A sort makes the result independent of the order of the faces.
 * f2n_mesh_ring_fill: one thread per vertex v.  ring_start_end [V,2] int32 = the range of edge_keys within [v V, (v + 1) V) (two binary
 *   searches); ring [E] int32: ring[j] = edge_keys[j] - v V for j in that range -- the neighbours of v ascending, each once;
 *   pinned [V] uint8 = 1 if the range is empty (no valid face uses v) or any edge of the range has edge_uses != 2 (v lies on a boundary
 *   or non-manifold edge), else 0;  edge_counts [2] int32 on the DEVICE, zeroed by the call on `stream`: [0] = the undirected edges
 *   with edge_uses == 1, [1] = those with edge_uses >= 3, each counted at its lower end (integer atomics: order-free).
 * f2n_mesh_smooth: one pass, one thread per vertex, out_verts [V,3] != verts.  A vertex is COPIED THROUGH bit for bit if it is pinned,
 *   its range is empty (or not within [0, n_ring]), one of its own coordinates is not finite, or a ring entry is outside [0, V) or
 *   names a vertex with a coordinate that is not finite.  Otherwise per component, in fp64:  s = 0;  for j in ring order: s = s + (double) x_j;
 *   m = s / (double) count;  d = m - (double) p;  t = factor * d;  out = (float) ((double) p + t).  factor is a finite double.
 *   A Taubin lambda|mu pair is this call twice (lambda, then mu) between two buffers.
 * f2n_mesh_move_clamp: the trust region, in place on pts [n,3] against p0 [n,3], fp32:  u_k = x_k - p0_k;
 *   l = sqrt((u_x u_x + u_y u_y) + u_z u_z);  if l > max_move:  k = max_move / l;  x_k = p0_k + u_k * k.  Otherwise (a NaN l included) the
 *   point keeps its bits.  The sums p0_k + u_k k round to the coordinates' own grid, which can leave x just outside the ball, so the
 *   result is measured again and pulled in, at most F2N_MOVE_CLAMP_ROUNDS times in all:  w_k = x_k - p0_k;  lw = sqrt((w_x w_x + w_y w_y)
 *   + w_z w_z);  lw > max_move:  k = (k * (max_move / lw)) * (1 - 2^-21);  x_k = p0_k + u_k * k again.  A round that ends with
 *   lw <= max_move ends the loop: then |x - p0| <= max_move as fp32 measures it (within max_move (1 + 2^-22) exactly).  Where an ulp of
 *   the coordinates is coarser than about max_move 2^-17 the rounds can run out with x one rounding outside.  max_move > 0 (+inf allowed). */
#define F2N_MOVE_CLAMP_ROUNDS 16
int f2n_mesh_ring_keys(void* stream, int n_verts, int n_faces, const int32_t* faces /*[F,3]*/, int64_t* keys /*[F,6]*/);
int f2n_mesh_ring_fill(void* stream, int n_verts, int n_edges, const int64_t* edge_keys /*[E]*/, const int64_t* edge_uses /*[E]*/,
                       int32_t* ring_start_end /*[V,2]*/, int32_t* ring /*[E]*/, uint8_t* pinned /*[V]*/, int32_t* edge_counts /*device [2]*/);
int f2n_mesh_smooth(void* stream, int n_verts, int n_ring, const float* verts /*[V,3]*/, const int32_t* ring_start_end /*[V,2]*/,
                    const int32_t* ring /*[E]*/, const uint8_t* pinned /*[V]*/, double factor, float* out_verts /*[V,3]*/);
int f2n_mesh_move_clamp(void* stream, int n, const float* p0 /*[n,3]*/, float max_move, float* pts /*[n,3], in place*/);

/* f2n_level_step: the per-iteration update of a damped Newton projection onto { h = 0 }, h(p) = ln sigma(p) - ln level, along
 * grad h = grad sigma / sigma.  The caller evaluates the field; the kernel never takes a logarithm and keeps no state of its own.
 * Per point i (one thread): p0 [n,3] the start;  cand [n,3] IN: the candidate c the caller just evaluated, OUT: the next one;
 * sigma [n], grad [n,3], h [n]: the field at c and h_c = log(sigma_c) - log(level) as the caller formed it;  state, in/out:
 * best [n,3] = b, h_best [n], g_best [n,3], scale [n] = a, status [n] int32 (bits below), evals [n] int32.  All fp32:
 *   0. not first and status has EMPTY or CONVERGED:  cand = b;  nothing else changes.
 *   1. g_k = grad_k / sigma (IEEE);  q = (g_x g_x + g_y g_y) + g_z g_z;  EVALUABLE = sigma > 0 and sigma, h_c, g_x, g_y, g_z finite
 *      and q != 0.
 *   2. first:  evals = 1;  b = c;  h_best = h_c;  a = 1;  status = 0;  g_best = g if EVALUABLE, else g_best = 0 and status = EMPTY
 *      (the point never moves: b = c = where the caller started it).
 *      not first:  evals = evals + 1;  ACCEPT = EVALUABLE and |h_c| <= |h_best|;  ACCEPT: b = c, h_best = h_c, g_best = g;
 *      otherwise a = a * 0.5.
 *   3. not EMPTY and |h_best| <= tol:  status |= CONVERGED.
 *   4. EMPTY, CONVERGED or propose == 0:  cand = b.  Otherwise  q_b = (g_best_x^2 + g_best_y^2) + g_best_z^2;  t = -((a * h_best) / q_b);
 *      d_k = t * g_best_k;  l = sqrt((d_x d_x + d_y d_y) + d_z d_z);  if l > max_step:  k = max_step / l, d_k = d_k * k,
 *      status |= STEP_CLAMPED;  c'_k = b_k + d_k;  then the trust region of f2n_mesh_move_clamp on c' against p0 with max_move, which sets
 *      MOVE_CLAMPED when it acts;  a c' with a coordinate that is not finite is replaced by b;  cand = c'.
 * So b is always a position at which the caller evaluated the field, and |h_best| never grows.  The clamp bits are sticky: they say
 * that a candidate of this point was clamped, not that the accepted one was.  tol >= 0, max_step > 0, max_move > 0 (+inf allowed). */
#define F2N_LEVEL_EMPTY 1
#define F2N_LEVEL_CONVERGED 2
#define F2N_LEVEL_STEP_CLAMPED 4
#define F2N_LEVEL_MOVE_CLAMPED 8
int f2n_level_step(void* stream, int n, int first, int propose, const float* p0 /*[n,3]*/, const float* sigma /*[n]*/,
                   const float* grad /*[n,3]*/, const float* h /*[n]*/, float tol, float max_step, float max_move, float* cand /*[n,3]*/,
                   float* best /*[n,3]*/, float* h_best /*[n]*/, float* g_best /*[n,3]*/, float* scale /*[n]*/, int32_t* status /*[n]*/,
                   int32_t* evals /*[n]*/);

/* f2n_mesh_face_quality: quality [F] fp64 per face, from the fp32 coordinates in fp64:  p = B - A, q = C - A, r = C - B;
 *   n = (p_y q_z - p_z q_y, p_z q_x - p_x q_z, p_x q_y - p_y q_x);  area2 = sqrt((n_x n_x + n_y n_y) + n_z n_z);
 *   l1 = (p_x p_x + p_y p_y) + p_z p_z, l2 and l3 likewise of q and r;  L = (l1 + l2) + l3;
 *   quality = L > 0 ? (K * area2) / L : 0, K = F2N_FACE_QUALITY_K = the double nearest 2 sqrt(3)  -- that is 4 sqrt(3) A / (sum of the
 *   squared edge lengths): 1 for an equilateral face, towards 0 for a sliver.  0 for a face that is not VALID (above); NaN for a valid
 *   face with a coordinate that is not finite. */
#define F2N_FACE_QUALITY_K 3.4641016151377544
int f2n_mesh_face_quality(void* stream, int n_verts, int n_faces, const float* verts /*[V,3]*/, const int32_t* faces /*[F,3]*/,
                          double* quality /*[F]*/);

#ifdef __cplusplus
}
#endif
#endif /* F2N_ABI_H */
