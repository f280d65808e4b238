// PersOctree::ProcOctree on gfx950 (PtsSampler/PersSampler.cpp:120-330): pruning of dead leaves, path compression,
// renumbering and subdivision of the occupancy octree WITHOUT the reference's device -> host -> device round trip of the
// node array (which stalls every data-parallel replica at each milestone / compaction).
//
// The reference code is a sequence of index-ordered loops over std::vector<TreeNode>; each has an order-free
// characterisation, which is what the kernels compute (equality with the sequential result is checked bit for bit in
// tests/test_gpu_e2e.py::test_proc_octree_matches_restatement, whose comparator is pinned to the reference's own code
// compiled for the CPU, tests/test_oracle_vs_ref.py):
//   compact loop (:139-178)   a node survives iff its subtree holds a leaf with trans_idx >= 0: valid leaves mark their
//                             ancestor chain; dead children are unhooked, childless interior nodes become (dead) leaves;
//   path compression (:181-215) every non-root interior node with exactly one child is spliced out; a node's new parent is
//                             its nearest ancestor that is not spliced, a child slot points at the first non-spliced node
//                             down the single-child chain below it (child counts do not change while splicing, and parents
//                             precede children in index order, so the sequential loop produces exactly this);
//   renumbering (:217-252)    exclusive prefix sum over the kept flags (f2n_segment_scan) + gather;
//   subdivision (:255-318)    the depth-first renumbering is a preorder position: 1 + the sizes of the elder siblings'
//                             subtrees, summed along the ancestor chain, where a subdivided leaf counts 9 nodes.
// Trees have at most a few 1e5 nodes and <= 24 levels; every kernel is one thread per node with an ancestor walk.
#include "f2n_dev.h"
#include "rows_dev.h"  // (F2N_DENSITY_SHIFT: the world-space queries at the end)

#define F2N_INIT_NODE_STAT 1000  // PersSampler.h:10

// alive[u] = 1 for every node whose subtree contains a valid leaf (benign races: all writers store 1).
__global__ void oct_mark_alive_kernel(int n, const F2nTreeNode* __restrict__ nodes, int32_t* __restrict__ alive) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  const F2nTreeNode& nd = nodes[u];
  if (!nd.is_leaf_node || nd.trans_idx < 0) return;
  int v = u;
  while (v >= 0 && alive[v] == 0) {  // (an already marked ancestor has marked the rest of the chain, or is doing so)
    alive[v] = 1;
    v = nodes[v].parent;
  }
}

// Applies the compact loop's fixed point to a working copy: childs of dead nodes unhooked, dead interior nodes (never the
// root) flagged as leaves, and the number of children left per node.
__global__ void oct_prune_kernel(int n, const int32_t* __restrict__ alive, F2nTreeNode* __restrict__ work, int32_t* __restrict__ n_child) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  F2nTreeNode& nd = work[u];
  int cnt = 0;
#pragma unroll
  for (int st = 0; st < 8; st++) {
    const int c = nd.childs[st];
    if (c >= 0) {
      // only LEAVES that are dead are unhooked by :141-151, interior nodes once they have turned into leaves (:153-172):
      // in the fixed point that is every child whose subtree holds no valid leaf
      if (alive[c] == 0) nd.childs[st] = -1;
      else cnt++;
    }
  }
  n_child[u] = cnt;
  if (u >= 1 && cnt == 0 && !nd.is_leaf_node) nd.is_leaf_node = 1;  // (its trans_idx is < 0: an interior node never carries a warp)
}

// Path compression.  spliced(v): interior, not the root, exactly one child.  Reads the pruned copy `work`, writes `out`.
__device__ __forceinline__ bool f2n_oct_spliced(const F2nTreeNode* __restrict__ work, const int32_t* __restrict__ n_child, int v) {
  return !work[v].is_leaf_node && work[v].parent >= 0 && n_child[v] == 1;
}

__global__ void oct_compress_kernel(int n, const F2nTreeNode* __restrict__ work, const int32_t* __restrict__ n_child,
                                    F2nTreeNode* __restrict__ out, int32_t* __restrict__ keep) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  F2nTreeNode nd = work[u];
  const bool dead_leaf = nd.is_leaf_node && nd.trans_idx < 0;
  if (!dead_leaf) {
    if (f2n_oct_spliced(work, n_child, u)) {  // :209-210 "the flag to remove it"
      nd.trans_idx = -1;
      nd.is_leaf_node = 1;
    } else {
      int v = nd.parent;  // nearest ancestor that stays
      while (v >= 0 && f2n_oct_spliced(work, n_child, v)) v = work[v].parent;
      nd.parent = v;
      if (!nd.is_leaf_node) {
#pragma unroll
        for (int st = 0; st < 8; st++) {
          int c = nd.childs[st];
          while (c >= 0 && f2n_oct_spliced(work, n_child, c)) {  // down the single-child chain
            int only = -1;
#pragma unroll
            for (int k = 0; k < 8; k++)
              if (work[c].childs[k] >= 0) only = work[c].childs[k];
            c = only;
          }
          nd.childs[st] = c;
        }
      }
    }
  }
  out[u] = nd;
  keep[u] = (!nd.is_leaf_node || nd.trans_idx >= 0) ? 1 : 0;  // :219-224
}

// Renumbering: new_pos[2u] = exclusive prefix of keep (f2n_segment_scan layout [n,2]).
__global__ void oct_gather_kept_kernel(int n, const F2nTreeNode* __restrict__ src, const int32_t* __restrict__ keep,
                                       const int32_t* __restrict__ new_pos, const int32_t* __restrict__ w_stats,
                                       const int32_t* __restrict__ a_stats, const int32_t* __restrict__ visit,
                                       F2nTreeNode* __restrict__ dst, int32_t* __restrict__ dst_w, int32_t* __restrict__ dst_a,
                                       int32_t* __restrict__ dst_visit) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n || keep[u] == 0) return;
  F2nTreeNode nd = src[u];
  if (nd.parent >= 0) nd.parent = new_pos[2 * nd.parent];
#pragma unroll
  for (int st = 0; st < 8; st++)
    if (nd.childs[st] >= 0) nd.childs[st] = new_pos[2 * nd.childs[st]];
  const int k = new_pos[2 * u];
  dst[k] = nd;
  dst_w[k] = w_stats[u];
  dst_a[k] = a_stats[u];
  dst_visit[k] = visit[u];
}

// Subdivision, pass 1: subtree sizes in the new numbering (a leaf that splits counts 9 nodes), bottom-up one depth at a
// time -- plain loads and stores (ancestor-chain atomics would pile ~1e5 same-address atomics onto the root).
__global__ void oct_depth_kernel(int n, const F2nTreeNode* __restrict__ nodes, int32_t* __restrict__ depth) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  int d = 0;
  for (int v = nodes[u].parent; v >= 0; v = nodes[v].parent) d++;
  depth[u] = d;
}
__global__ void oct_size_level_kernel(int n, int level, const F2nTreeNode* __restrict__ nodes, const int32_t* __restrict__ depth,
                                      const int32_t* __restrict__ visit, int brute_force, int32_t* __restrict__ size) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n || depth[u] != level) return;
  const F2nTreeNode& nd = nodes[u];
  int sz = 1;
  if (nd.is_leaf_node) {
    if (brute_force || visit[u] > 4) sz = 9;  // :279
  } else {
#pragma unroll
    for (int st = 0; st < 8; st++)
      if (nd.childs[st] >= 0) sz += size[nd.childs[st]];  // written by the previous (deeper) launch
  }
  size[u] = sz;
}

// Subdivision, pass 2: preorder position of every node, and the nodes themselves in the new numbering.
__global__ void oct_subdivide_emit_kernel(int n, const F2nTreeNode* __restrict__ nodes, const int32_t* __restrict__ visit, int brute_force,
                                          const int32_t* __restrict__ size, const int32_t* __restrict__ w_stats,
                                          const int32_t* __restrict__ a_stats, int32_t* __restrict__ new_idx,
                                          F2nTreeNode* __restrict__ dst, int32_t* __restrict__ dst_w, int32_t* __restrict__ dst_a) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  auto position = [&](int x) {
    int pos = 0;
    int c = x;
    for (int p = nodes[x].parent; p >= 0; c = p, p = nodes[p].parent) {
      pos += 1;  // the parent itself precedes its subtree
#pragma unroll
      for (int st = 0; st < 8; st++) {
        const int s = nodes[p].childs[st];
        if (s == c) break;
        if (s >= 0) pos += size[s];
      }
    }
    return pos;
  };
  const int me = position(u);
  new_idx[u] = me;
  F2nTreeNode nd = nodes[u];
  const int old_parent = nd.parent;
  nd.parent = old_parent >= 0 ? position(old_parent) : -1;
  const bool split = nd.is_leaf_node && (brute_force || visit[u] > 4);
  if (!nd.is_leaf_node) {
    int next = me + 1;  // children follow their parent in slot order (:305-311)
#pragma unroll
    for (int st = 0; st < 8; st++) {
      const int s = nd.childs[st];
      if (s >= 0) {
        nd.childs[st] = next;
        next += size[s];
      }
    }
    dst[me] = nd;
    dst_w[me] = w_stats[u];
    dst_a[me] = a_stats[u];
  } else if (!split) {
    dst[me] = nd;
    dst_w[me] = w_stats[u];
    dst_a[me] = a_stats[u];
  } else {  // :280-303
    F2nTreeNode pr = nd;
#pragma unroll
    for (int st = 0; st < 8; st++) {
      const float off[3] = {float((st >> 2) & 1) - .5f, float((st >> 1) & 1) - .5f, float(st & 1) - .5f};
      F2nTreeNode ch;
      for (int k = 0; k < 3; k++) ch.center[k] = nd.center[k] + nd.side_len * .5f * off[k];
      ch.side_len = nd.side_len * .5f;
      ch.parent = me;
      for (int k = 0; k < 8; k++) ch.childs[k] = -1;
      ch.is_leaf_node = 1;
      ch.pad0[0] = ch.pad0[1] = ch.pad0[2] = 0;
      ch.trans_idx = nd.trans_idx;
      ch.pad1[0] = ch.pad1[1] = ch.pad1[2] = ch.pad1[3] = 0;
      dst[me + 1 + st] = ch;
      dst_w[me + 1 + st] = w_stats[u];
      dst_a[me + 1 + st] = a_stats[u];
      pr.childs[st] = me + 1 + st;
    }
    pr.is_leaf_node = 0;
    pr.trans_idx = -1;
    dst[me] = pr;
    dst_w[me] = F2N_INIT_NODE_STAT;
    dst_a[me] = F2N_INIT_NODE_STAT;
  }
}

extern "C" {

int f2n_oct_prune_compress(void* stream, int n_nodes, const void* tree_nodes, void* work_nodes, void* out_nodes, int32_t* alive,
                           int32_t* n_child, int32_t* keep) {
  if (n_nodes < 0) return F2N_ERR_INVALID_ARG;
  if (n_nodes == 0) return F2N_OK;
  hipStream_t st = (hipStream_t) stream;
  const dim3 grid(f2n_div_up(n_nodes, 256)), block(256);
  if (hipMemsetAsync(alive, 0, sizeof(int32_t) * (size_t) n_nodes, st) != hipSuccess) return f2n_launch_status();
  if (hipMemcpyAsync(work_nodes, tree_nodes, sizeof(F2nTreeNode) * (size_t) n_nodes, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return f2n_launch_status();
  hipLaunchKernelGGL(oct_mark_alive_kernel, grid, block, 0, st, n_nodes, (const F2nTreeNode*) tree_nodes, alive);
  hipLaunchKernelGGL(oct_prune_kernel, grid, block, 0, st, n_nodes, alive, (F2nTreeNode*) work_nodes, n_child);
  hipLaunchKernelGGL(oct_compress_kernel, grid, block, 0, st, n_nodes, (const F2nTreeNode*) work_nodes, n_child,
                     (F2nTreeNode*) out_nodes, keep);
  return f2n_launch_status();
}

int f2n_oct_gather_kept(void* stream, int n_nodes, const void* nodes, const int32_t* keep, const int32_t* new_pos,
                        const int32_t* w_stats, const int32_t* a_stats, const int32_t* visit_cnt, void* dst_nodes, int32_t* dst_w,
                        int32_t* dst_a, int32_t* dst_visit) {
  if (n_nodes < 0) return F2N_ERR_INVALID_ARG;
  if (n_nodes == 0) return F2N_OK;
  hipLaunchKernelGGL(oct_gather_kept_kernel, dim3(f2n_div_up(n_nodes, 256)), dim3(256), 0, (hipStream_t) stream, n_nodes,
                     (const F2nTreeNode*) nodes, keep, new_pos, w_stats, a_stats, visit_cnt, (F2nTreeNode*) dst_nodes, dst_w, dst_a,
                     dst_visit);
  return f2n_launch_status();
}

#define F2N_OCT_MAX_DEPTH 40  // the reference's own DFS walks at most 24 levels (PersSampler.cu:7)
int f2n_oct_subtree_sizes(void* stream, int n_nodes, const void* nodes, const int32_t* visit_cnt, int brute_force, int32_t* depth,
                          int32_t* size) {
  if (n_nodes < 0) return F2N_ERR_INVALID_ARG;
  if (n_nodes == 0) return F2N_OK;
  hipStream_t st = (hipStream_t) stream;
  const dim3 grid(f2n_div_up(n_nodes, 256)), block(256);
  hipLaunchKernelGGL(oct_depth_kernel, grid, block, 0, st, n_nodes, (const F2nTreeNode*) nodes, depth);
  for (int level = F2N_OCT_MAX_DEPTH - 1; level >= 0; level--)
    hipLaunchKernelGGL(oct_size_level_kernel, grid, block, 0, st, n_nodes, level, (const F2nTreeNode*) nodes, depth, visit_cnt,
                       brute_force, size);
  return f2n_launch_status();
}

int f2n_oct_subdivide(void* stream, int n_nodes, const void* nodes, const int32_t* visit_cnt, int brute_force, const int32_t* size,
                      const int32_t* w_stats, const int32_t* a_stats, int32_t* new_idx, void* dst_nodes, int32_t* dst_w, int32_t* dst_a) {
  if (n_nodes < 0) return F2N_ERR_INVALID_ARG;
  if (n_nodes == 0) return F2N_OK;
  hipLaunchKernelGGL(oct_subdivide_emit_kernel, dim3(f2n_div_up(n_nodes, 256)), dim3(256), 0, (hipStream_t) stream, n_nodes,
                     (const F2nTreeNode*) nodes, visit_cnt, brute_force, size, w_stats, a_stats, new_idx, (F2nTreeNode*) dst_nodes, dst_w,
                     dst_a);
  return f2n_launch_status();
}

}  // extern "C"

// =====================================================================================================================
// World-space queries of a trained scene and iso-surface extraction (include/f2n_abi.h, "World-space queries and meshes").
//   locate:  a world point -> the octree leaf that holds it (the descent the ray walk of PersSampler.cu:54-152 never makes
//            for a single point) -> its perspective warp (f2n_warp), in the anchor layout of GetSamples
//   density: count -> f2n_segment_scan -> compact of the non-empty points, and the scatter of exp(f0 - 3) back to every point
//   mesh:    marching tetrahedra on the Kuhn split of every grid cell (six tetrahedra around the (0,0,0)-(1,1,1) diagonal)
//   bricks:  the same mesh from the bricks of B^3 cells that can hold something: a box-against-octree mark, the locate for the
//            corners of listed bricks, and the mesher per brick with 64-bit keys in the place of the dense scans
// =====================================================================================================================

#define F2N_OCT_MAX_DEPTH 32  // a descent longer than this is a corrupt tree: the point is reported empty

namespace {

// (F2N_ADD_RN / _SUB_RN / _MUL_RN / _DIV_RN: single roundings that the compiler may not contract into an FMA, f2n_dev.h)

// The grid point of index (ix, iy, iz): lo + step * i with two roundings (f2n_grid_coord, f2n_dev.h)
__device__ __forceinline__ float grid_coord(float lo, float step, int i) { return f2n_grid_coord(lo, step, i); }

// Leaf of the point p, or -1 when p lies outside the root cube, in a missing child slot, or in a leaf with trans_idx < 0
// (exactly the nodes the ray walk never lists).  *trans receives the leaf's trans_idx.
__device__ __forceinline__ int oct_locate(const F2nTreeNode* __restrict__ nodes, const float p[3], int* trans) {
  const F2nTreeNode& root = nodes[0];
  const float h = root.side_len * .5f;
#pragma unroll
  for (int k = 0; k < 3; k++)
    if (!(p[k] >= root.center[k] - h && p[k] <= root.center[k] + h)) return -1;  // (NaN: empty as well)
  int u = 0;
  for (int depth = 0; depth < F2N_OCT_MAX_DEPTH; depth++) {
    const F2nTreeNode& nd = nodes[u];
    bool any = false;
#pragma unroll
    for (int c = 0; c < 8; c++) any |= nd.childs[c] >= 0;
    if (!any) {  // a node with no children is a leaf (PersSampler.cu:98-110)
      *trans = nd.trans_idx;
      return nd.trans_idx >= 0 ? u : -1;
    }
    // child slot order of ConstructTreeNode (PersSampler.cpp:397-401): 4 * (x >= cx) + 2 * (y >= cy) + (z >= cz)
    const int st = 4 * (int) (p[0] >= nd.center[0]) + 2 * (int) (p[1] >= nd.center[1]) + (int) (p[2] >= nd.center[2]);
    int ch = nd.childs[0];  // (selected without indexing the record by a run-time value held in registers)
#pragma unroll
    for (int c = 1; c < 8; c++) ch = st == c ? nd.childs[c] : ch;
    if (ch < 0) return -1;
    u = ch;
  }
  return -1;
}

template <bool GRID>
__global__ void __launch_bounds__(256) oct_locate_warp_kernel(int n, const float* __restrict__ pts_world, float lo0, float lo1, float lo2,
                                                              float step, int nx, int ny, int first_z,
                                                              const F2nTreeNode* __restrict__ nodes,
                                                              const F2nTransInfo* __restrict__ transes, float* __restrict__ out_pts,
                                                              int32_t* __restrict__ out_anchors) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float p[3];
  if (GRID) {
    const int64_t plane = (int64_t) nx * ny;
    const int iz = first_z + (int) (i / plane);
    const int64_t r = i % plane;
    p[0] = grid_coord(lo0, step, (int) (r % nx));
    p[1] = grid_coord(lo1, step, (int) (r / nx));
    p[2] = grid_coord(lo2, step, iz);
  } else {
    p[0] = pts_world[i * 3 + 0];
    p[1] = pts_world[i * 3 + 1];
    p[2] = pts_world[i * 3 + 2];
  }
  int trans = -1;
  const int leaf = oct_locate(nodes, p, &trans);
  float w[3] = {0.f, 0.f, 0.f};
  if (leaf >= 0) f2n_warp(transes + trans, p, w);
  out_pts[i * 3 + 0] = w[0];
  out_pts[i * 3 + 1] = w[1];
  out_pts[i * 3 + 2] = w[2];
  out_anchors[i * 3 + 0] = leaf >= 0 ? trans : -1;
  out_anchors[i * 3 + 1] = leaf;
  out_anchors[i * 3 + 2] = 0;
}

__global__ void __launch_bounds__(256) located_count_kernel(int n, const int32_t* __restrict__ anchors, int32_t* __restrict__ counts) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) counts[i] = anchors[i * 3] >= 0 ? 1 : 0;
}

__global__ void __launch_bounds__(256) located_compact_kernel(int n, const int32_t* __restrict__ anchors, const float* __restrict__ pts,
                                                             const int32_t* __restrict__ start_end, float* __restrict__ out_pts,
                                                             int32_t* __restrict__ out_vol, int32_t* __restrict__ out_src) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int vol = anchors[i * 3];
  if (vol < 0) return;
  const int64_t k = start_end[i * 2];
  out_pts[k * 3 + 0] = pts[i * 3 + 0];
  out_pts[k * 3 + 1] = pts[i * 3 + 1];
  out_pts[k * 3 + 2] = pts[i * 3 + 2];
  out_vol[k] = vol;
  if (out_src != nullptr) out_src[k] = (int32_t) i;
}

__global__ void __launch_bounds__(256) density_scatter_kernel(int n, const int32_t* __restrict__ anchors, const int32_t* __restrict__ start_end,
                                                             const float* __restrict__ f0, float* __restrict__ density) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  density[i] = anchors[i * 3] >= 0 ? expf(f0[start_end[i * 2]] - F2N_DENSITY_SHIFT) : 0.f;  // TruncExp(f0 - 3), Renderer.cpp:101-104
}

// ---- marching tetrahedra ------------------------------------------------------------------------------------------------
// Corner offsets are 3-bit masks (x = 1, y = 2, z = 4).  Tetrahedron t of a cell, for the axis order (a, b, c) of row t:
// (0, a, a|b, 7).  Its orientation is the parity of the axis permutation.
__constant__ int8_t c_tet_axes[6][3] = {{1, 2, 4}, {1, 4, 2}, {2, 1, 4}, {2, 4, 1}, {4, 1, 2}, {4, 2, 1}};
__constant__ int8_t c_tet_even[6] = {1, 0, 0, 1, 1, 0};
// Edge type of an offset mask: +x, +y, +z, +xy, +xz, +yz, +xyz = 0..6 (-1: mask 0)
__constant__ int8_t c_edge_type[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
// Case of a tetrahedron by its inside mask (bit v: tet vertex v is inside): {kind, i, j, k, l, flip}.  kind 1: one corner i alone
// on its side (inside or outside), j < k < l the others -> triangle (ij, ik, il); kind 3: i < j inside, k < l outside -> triangles
// (ik, il, jl), (ik, jl, jk).  flip: those triangles face inward on a positively oriented tetrahedron and are reversed (second and
// third vertex swapped); a negatively oriented one reverses once more.  (Derived from the geometry of the (0, x, x|y, 7) tet.)
__constant__ int8_t c_tet_case[16][6] = {
    {0, 0, 1, 2, 3, 0},  // 0000
    {1, 0, 1, 2, 3, 0},  // 0001
    {1, 1, 0, 2, 3, 1},  // 0010
    {3, 0, 1, 2, 3, 0},  // 0011
    {1, 2, 0, 1, 3, 0},  // 0100
    {3, 0, 2, 1, 3, 1},  // 0101
    {3, 1, 2, 0, 3, 0},  // 0110
    {1, 3, 0, 1, 2, 0},  // 0111
    {1, 3, 0, 1, 2, 1},  // 1000
    {3, 0, 3, 1, 2, 0},  // 1001
    {3, 1, 3, 0, 2, 1},  // 1010
    {1, 2, 0, 1, 3, 1},  // 1011
    {3, 2, 3, 0, 1, 0},  // 1100
    {1, 1, 0, 2, 3, 0},  // 1101
    {1, 0, 1, 2, 3, 1},  // 1110
    {0, 0, 1, 2, 3, 0},  // 1111
};
__constant__ int8_t c_tri_count[4] = {0, 1, 1, 2};

__device__ __forceinline__ int64_t corner_index(int x, int y, int z, int nx, int ny) { return ((int64_t) z * ny + y) * nx + x; }

// The rules every mesher of this file shares (f2n_mesh_emit, f2n_brick_mesh_emit): a corner is inside iff g > level ...
__device__ __forceinline__ bool mesh_inside(float g, float level) { return g > level; }

// ... the vertex of the crossing edge a -> b (a = the lower endpoint) lies at p_a + t (p_b - p_a), t = (level - g_a) / (g_b - g_a) ...
__device__ __forceinline__ void mesh_edge_point(float level, float ga, float gb, const float pa[3], const float pb[3], float out[3]) {
  const float s = F2N_DIV_RN(F2N_SUB_RN(level, ga), F2N_SUB_RN(gb, ga));
#pragma unroll
  for (int k = 0; k < 3; k++) out[k] = F2N_ADD_RN(pa[k], F2N_MUL_RN(s, F2N_SUB_RN(pb[k], pa[k])));
}

// (masked meshing, f2n_mesh_count_masked) the cell whose lowest corner is (x, y, z) lies in the grid and all eight of its corners are valid
__device__ __forceinline__ bool cell_observed(int x, int y, int z, int nx, int ny, int nz, const uint8_t* __restrict__ valid) {
  if (x < 0 || y < 0 || z < 0 || x + 1 >= nx || y + 1 >= ny || z + 1 >= nz) return false;
  bool all = true;
#pragma unroll
  for (int o = 0; o < 8; o++) all = all && valid[corner_index(x + (o & 1), y + ((o >> 1) & 1), z + ((o >> 2) & 1), nx, ny)] != 0;
  return all;
}

// Vertex count pass: bit t of edge_mask[c] = edge of type t from corner c to a corner inside the grid crosses the level.
// MASKED: ... and one of the cells whose Kuhn tetrahedra use that edge is observed: the cells c - d, d over the subsets of the axes
// the edge's offset does not have.
template <bool MASKED>
__global__ void __launch_bounds__(256) mesh_vert_count_kernel(int nx, int ny, int nz, const float* __restrict__ g, float level,
                                                             const uint8_t* __restrict__ valid, uint8_t* __restrict__ edge_mask,
                                                             int32_t* __restrict__ counts) {
  const int64_t c = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (int64_t) nx * ny * nz) return;
  const int x = (int) (c % nx), y = (int) ((c / nx) % ny), z = (int) (c / ((int64_t) nx * ny));
  const bool in0 = mesh_inside(g[c], level);
  uint32_t m = 0;
#pragma unroll
  for (int o = 1; o < 8; o++) {
    const int dx = o & 1, dy = (o >> 1) & 1, dz = (o >> 2) & 1;
    if (x + dx >= nx || y + dy >= ny || z + dz >= nz) continue;
    const bool in1 = mesh_inside(g[corner_index(x + dx, y + dy, z + dz, nx, ny)], level);
    if (in0 == in1) continue;
    if (MASKED) {
      bool used = false;
#pragma unroll
      for (int d = 0; d < 8; d++) {
        if (d & o) continue;  // (only the axes the edge does not run along)
        used = used || cell_observed(x - (d & 1), y - ((d >> 1) & 1), z - ((d >> 2) & 1), nx, ny, nz, valid);
      }
      if (!used) continue;
    }
    m |= 1u << c_edge_type[o];
  }
  edge_mask[c] = (uint8_t) m;
  counts[c] = __popc(m);
}

__device__ __forceinline__ int cell_mask(int x, int y, int z, int nx, int ny, const float* __restrict__ g, float level) {
  int m = 0;
#pragma unroll
  for (int o = 0; o < 8; o++)
    m |= (mesh_inside(g[corner_index(x + (o & 1), y + ((o >> 1) & 1), z + ((o >> 2) & 1), nx, ny)], level) ? 1 : 0) << o;
  return m;  // bit o: cell corner of offset o is inside
}

__device__ __forceinline__ int tet_inside(int cm, int t) {
  const int a = c_tet_axes[t][0], ab = a | c_tet_axes[t][1];
  return ((cm >> 0) & 1) | (((cm >> a) & 1) << 1) | (((cm >> ab) & 1) << 2) | (((cm >> 7) & 1) << 3);
}

// ... the number of faces of a cell with the inside mask cm (bit o: the corner of offset o is inside) ...
__device__ __forceinline__ int cell_face_count(int cm) {
  int n = 0;
  if (cm != 0 && cm != 255)
    for (int t = 0; t < 6; t++) n += c_tri_count[c_tet_case[tet_inside(cm, t)][0]];
  return n;
}

// ... and its faces, in the order (tet, triangle), wound outwards: emit(v0, v1, v2) per face, each v = vertex_of(oa, ob), the id of
// the vertex on the edge between the cell corners of offsets oa and ob (one dominates the other on a Kuhn tetrahedron).
template <typename Id, typename VertexOf, typename Emit>
__device__ __forceinline__ void cell_faces(int cm, VertexOf vertex_of, Emit emit) {
  for (int t = 0; t < 6; t++) {
    const int a = c_tet_axes[t][0], ab = a | c_tet_axes[t][1];
    const int mask = tet_inside(cm, t);
    const int kind = c_tet_case[mask][0];
    if (kind == 0) continue;
    // tet vertex v -> cell corner offset (0, a, a|b, 7), without a private array
    auto off = [a, ab](int v) { return v == 0 ? 0 : v == 1 ? a : v == 2 ? ab : 7; };
    const int oi = off(c_tet_case[mask][1]), oj = off(c_tet_case[mask][2]), ok = off(c_tet_case[mask][3]),
              ol = off(c_tet_case[mask][4]);
    const bool flip = (c_tet_case[mask][5] != 0) != (c_tet_even[t] == 0);
    Id tri[2][3];
    int n_tri = 1;
    if (kind == 1) {
      tri[0][0] = vertex_of(oi, oj);
      tri[0][1] = vertex_of(oi, ok);
      tri[0][2] = vertex_of(oi, ol);
    } else {
      const Id vik = vertex_of(oi, ok);
      const Id vil = vertex_of(oi, ol);
      const Id vjl = vertex_of(oj, ol);
      const Id vjk = vertex_of(oj, ok);
      tri[0][0] = vik; tri[0][1] = vil; tri[0][2] = vjl;
      tri[1][0] = vik; tri[1][1] = vjl; tri[1][2] = vjk;
      n_tri = 2;
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
      if (q >= n_tri) break;
      emit(tri[q][0], flip ? tri[q][2] : tri[q][1], flip ? tri[q][1] : tri[q][2]);
    }
  }
}

template <bool MASKED>
__global__ void __launch_bounds__(256) mesh_face_count_kernel(int nx, int ny, int nz, const float* __restrict__ g, float level,
                                                             const uint8_t* __restrict__ valid, int32_t* __restrict__ counts) {
  const int cx = nx - 1, cy = ny - 1;
  const int64_t c = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (int64_t) cx * cy * (nz - 1)) return;
  const int x = (int) (c % cx), y = (int) ((c / cx) % cy), z = (int) (c / ((int64_t) cx * cy));
  const int cm = cell_mask(x, y, z, nx, ny, g, level);
  counts[c] = cm != 0 && cm != 255 && (!MASKED || cell_observed(x, y, z, nx, ny, nz, valid)) ? cell_face_count(cm) : 0;
}

__global__ void __launch_bounds__(256) mesh_vert_emit_kernel(int nx, int ny, int nz, const float* __restrict__ g, float level, float lo0,
                                                            float lo1, float lo2, float step, const uint8_t* __restrict__ edge_mask,
                                                            const int32_t* __restrict__ start_end, float* __restrict__ verts) {
  const int64_t c = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (int64_t) nx * ny * nz) return;
  const uint32_t m = edge_mask[c];
  if (m == 0) return;
  const int x = (int) (c % nx), y = (int) ((c / nx) % ny), z = (int) (c / ((int64_t) nx * ny));
  const float ga = g[c];
  const float pa[3] = {grid_coord(lo0, step, x), grid_coord(lo1, step, y), grid_coord(lo2, step, z)};
  int64_t v = start_end[c * 2];
#pragma unroll
  for (int o = 1; o < 8; o++) {
    const int t = c_edge_type[o];
    if (!((m >> t) & 1)) continue;
    // (the loop over o visits types 0, 1, 3, 2, 4, 5, 6: the slot is the rank of t among the set bits, not the visit order)
    const int64_t slot = v + __popc(m & ((1u << t) - 1u));
    const int dx = o & 1, dy = (o >> 1) & 1, dz = (o >> 2) & 1;
    const float gb = g[corner_index(x + dx, y + dy, z + dz, nx, ny)];
    const float pb[3] = {grid_coord(lo0, step, x + dx), grid_coord(lo1, step, y + dy), grid_coord(lo2, step, z + dz)};
    float p[3];
    mesh_edge_point(level, ga, gb, pa, pb, p);
#pragma unroll
    for (int k = 0; k < 3; k++) verts[slot * 3 + k] = p[k];
  }
}

// id of the vertex on the edge between cell corners of offsets oa and ob (one dominates the other on a Kuhn tetrahedron)
__device__ __forceinline__ int32_t edge_vertex(int x, int y, int z, int nx, int ny, int oa, int ob, const uint8_t* __restrict__ edge_mask,
                                               const int32_t* __restrict__ start_end) {
  const int lo = (oa & ob) == oa ? oa : ob;
  const int t = c_edge_type[oa ^ ob];
  const int64_t c = corner_index(x + (lo & 1), y + ((lo >> 1) & 1), z + ((lo >> 2) & 1), nx, ny);
  return start_end[c * 2] + __popc((uint32_t) edge_mask[c] & ((1u << t) - 1u));
}

__global__ void __launch_bounds__(256) mesh_face_emit_kernel(int nx, int ny, int nz, const float* __restrict__ g, float level,
                                                            const uint8_t* __restrict__ edge_mask, const int32_t* __restrict__ vert_se,
                                                            const int32_t* __restrict__ face_se, int32_t* __restrict__ faces) {
  const int cx = nx - 1, cy = ny - 1;
  const int64_t c = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (int64_t) cx * cy * (nz - 1)) return;
  if (face_se[c * 2] == face_se[c * 2 + 1]) return;
  const int x = (int) (c % cx), y = (int) ((c / cx) % cy), z = (int) (c / ((int64_t) cx * cy));
  const int cm = cell_mask(x, y, z, nx, ny, g, level);
  int64_t f = face_se[c * 2];
  cell_faces<int32_t>(
      cm, [&](int oa, int ob) { return edge_vertex(x, y, z, nx, ny, oa, ob, edge_mask, vert_se); },
      [&](int32_t v0, int32_t v1, int32_t v2) {
        faces[f * 3 + 0] = v0;
        faces[f * 3 + 1] = v1;
        faces[f * 3 + 2] = v2;
        f++;
      });
}

// ---- sparse meshing on bricks of B^3 cells (include/f2n_abi.h, "Sparse mesh extraction on bricks") -----------------------------
// The virtual grid is never materialised: a brick is its linear id (x fastest over nb = ceil((n - 1) / B) bricks per axis), its
// values are the (B + 1)^3 corners b B + l, l in [0, B]^3, local x fastest.
#define F2N_BRICK_MARK_THREADS 64

struct BrickGrid {
  float lo[3], step;
  int n[3], nb[3], B;
};

__device__ __forceinline__ void brick_coords(const BrickGrid& g, int64_t b, int bc[3]) {
  bc[0] = (int) (b % g.nb[0]);
  bc[1] = (int) ((b / g.nb[0]) % g.nb[1]);
  bc[2] = (int) (b / ((int64_t) g.nb[0] * g.nb[1]));
}

// flags[b] = the closed box of brick b meets a live leaf.  One thread per brick; the descent keeps (node, next child slot) per level
// in LDS, [level][thread] -- no private stack, no recursion.  Nodes deeper than F2N_OCT_MAX_DEPTH - 1 are not entered, as in oct_locate.
__global__ void __launch_bounds__(F2N_BRICK_MARK_THREADS) brick_mark_kernel(BrickGrid g, int64_t n_bricks,
                                                                           const F2nTreeNode* __restrict__ nodes,
                                                                           uint8_t* __restrict__ flags) {
  __shared__ int32_t s_node[F2N_OCT_MAX_DEPTH][F2N_BRICK_MARK_THREADS];
  __shared__ uint8_t s_next[F2N_OCT_MAX_DEPTH][F2N_BRICK_MARK_THREADS];
  const int t = threadIdx.x;
  const int64_t b = (int64_t) blockIdx.x * F2N_BRICK_MARK_THREADS + t;
  if (b >= n_bricks) return;
  int bc[3];
  brick_coords(g, b, bc);
  float blo[3], bhi[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int i0 = bc[k] * g.B, i1 = min(i0 + g.B, g.n[k] - 1);
    blo[k] = grid_coord(g.lo[k], g.step, i0);
    bhi[k] = grid_coord(g.lo[k], g.step, i1);
  }
  const F2nTreeNode& root = nodes[0];
  const float h = root.side_len * .5f;
  bool meets = true;
#pragma unroll
  for (int k = 0; k < 3; k++) meets = meets && bhi[k] >= root.center[k] - h && blo[k] <= root.center[k] + h;  // (NaN: no)
  uint8_t flag = 0;
  int d = meets ? 0 : -1;
  if (meets) {
    s_node[0][t] = 0;
    s_next[0][t] = 0;
  }
  while (d >= 0) {
    const int u = s_node[d][t];
    const int first = s_next[d][t];
    const F2nTreeNode* nd = nodes + u;
    // the child slots the box reaches: slot 4 sx + 2 sy + sz with (s_k = 0 and blo_k < c_k) or (s_k = 1 and bhi_k >= c_k)
    bool any = false;
    int want = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const bool have = nd->childs[c] >= 0;
      any |= have;
      bool in = have;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int s = (c >> (2 - k)) & 1;
        in = in && (s ? bhi[k] >= nd->center[k] : blo[k] < nd->center[k]);
      }
      want |= (in ? 1 : 0) << c;
    }
    if (!any) {  // a node without children
      if (nd->trans_idx >= 0) {
        flag = 1;
        break;
      }
      d--;
      continue;
    }
    want &= ~((1 << first) - 1);
    if (want == 0 || d + 1 >= F2N_OCT_MAX_DEPTH) {
      d--;
      continue;
    }
    const int c = __ffs(want) - 1;
    s_next[d][t] = (uint8_t) (c + 1);
    d++;
    s_node[d][t] = nd->childs[c];  // (read from memory by its run-time index: nothing private is indexed)
    s_next[d][t] = 0;
  }
  flags[b] = flag;
}

// oct_locate_warp_kernel<true> for the corners of listed bricks: row (j, l) = brick j of the list, local corner l (x fastest)
__global__ void __launch_bounds__(256) oct_locate_warp_bricks_kernel(BrickGrid g, int64_t n_total, int64_t n, const int32_t* __restrict__ brick_ids,
                                                                     const F2nTreeNode* __restrict__ nodes,
                                                                     const F2nTransInfo* __restrict__ transes, float* __restrict__ out_pts,
                                                                     int32_t* __restrict__ out_anchors) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int S = g.B + 1, P = S * S * S;
  const int64_t b = brick_ids[i / P];
  const int l = (int) (i % P);
  const int lc[3] = {l % S, (l / S) % S, l / (S * S)};
  bool exists = b >= 0 && b < n_total;
  float p[3] = {0.f, 0.f, 0.f};
  if (exists) {
    int bc[3];
    brick_coords(g, b, bc);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int ik = bc[k] * g.B + lc[k];
      exists = exists && ik <= g.n[k] - 1;
      p[k] = grid_coord(g.lo[k], g.step, ik);
    }
  }
  int trans = -1, leaf = -1;
  if (exists) leaf = oct_locate(nodes, p, &trans);
  float w[3] = {0.f, 0.f, 0.f};
  if (leaf >= 0) f2n_warp(transes + trans, p, w);
  out_pts[i * 3 + 0] = w[0];
  out_pts[i * 3 + 1] = w[1];
  out_pts[i * 3 + 2] = w[2];
  out_anchors[i * 3 + 0] = leaf >= 0 ? trans : -1;
  out_anchors[i * 3 + 1] = leaf;
  out_anchors[i * 3 + 2] = 0;
}

// One brick of the list per workgroup of 256 threads, its values in LDS.  MASKED (f2n_brick_mesh_count_masked / _emit_masked): the row
// of `valid` bytes is staged next to the values (s_ok); an edge needs both endpoints valid, a cell all eight corners.
template <int B>
struct BrickTile {
  static constexpr int S = B + 1, P = S * S * S, CELLS = B * B * B;
  int x0[3];    // the grid index of the local corner (0, 0, 0)
  bool last[3]; // the last brick of the axis: it owns the local plane B as well (the grid's border plane when n - 1 is a multiple of B)
  int n[3];

  __device__ __forceinline__ void init(int nx, int ny, int nz, int64_t b) {
    n[0] = nx, n[1] = ny, n[2] = nz;
    const int nb0 = (nx - 1 + B - 1) / B, nb1 = (ny - 1 + B - 1) / B, nb2 = (nz - 1 + B - 1) / B;
    const int bc[3] = {(int) (b % nb0), (int) ((b / nb0) % nb1), (int) (b / ((int64_t) nb0 * nb1))};
    const int nb[3] = {nb0, nb1, nb2};
    if (b < 0 || b >= (int64_t) nb0 * nb1 * nb2) n[0] = n[1] = n[2] = 0;  // (no such brick: it owns nothing)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      x0[k] = bc[k] * B;
      last[k] = bc[k] == nb[k] - 1;
    }
  }
  template <bool MASKED>
  __device__ __forceinline__ void stage(const float* __restrict__ values, const uint8_t* __restrict__ valid, float* s_val, uint8_t* s_ok) const {
    const float* src = values + (int64_t) blockIdx.x * P;
    for (int i = threadIdx.x; i < P; i += 256) s_val[i] = src[i];
    if (MASKED) {
      const uint8_t* ok = valid + (int64_t) blockIdx.x * P;
      for (int i = threadIdx.x; i < P; i += 256) s_ok[i] = ok[i];
    }
    __syncthreads();
  }
  static __device__ __forceinline__ int local(int lx, int ly, int lz) { return (lz * S + ly) * S + lx; }
  // bit t: the edge of type t owned by the local corner l crosses the level; 0 for a corner this brick does not own
  template <bool MASKED>
  __device__ __forceinline__ uint32_t corner_edges(const float* s_val, const uint8_t* s_ok, int l, float level) const {
    if (l >= P) return 0;
    const int lc[3] = {l % S, (l / S) % S, l / (S * S)};
#pragma unroll
    for (int k = 0; k < 3; k++)
      if ((lc[k] >= B && !last[k]) || x0[k] + lc[k] > n[k] - 1) return 0;
    if (MASKED && s_ok[l] == 0) return 0;
    const bool in0 = mesh_inside(s_val[l], level);
    uint32_t m = 0;
#pragma unroll
    for (int o = 1; o < 8; o++) {
      const int dx = o & 1, dy = (o >> 1) & 1, dz = (o >> 2) & 1;
      if (lc[0] + dx > B || lc[1] + dy > B || lc[2] + dz > B) continue;
      if (x0[0] + lc[0] + dx > n[0] - 1 || x0[1] + lc[1] + dy > n[1] - 1 || x0[2] + lc[2] + dz > n[2] - 1) continue;
      if (MASKED && s_ok[local(lc[0] + dx, lc[1] + dy, lc[2] + dz)] == 0) continue;
      if (in0 != mesh_inside(s_val[local(lc[0] + dx, lc[1] + dy, lc[2] + dz)], level)) m |= 1u << c_edge_type[o];
    }
    return m;
  }
  // the inside mask of the owned cell c (local index in [0, B)^3, x fastest), 0 for a cell outside the grid (MASKED: and for a cell with
  // a corner that is not valid); lc receives its local corner
  template <bool MASKED>
  __device__ __forceinline__ int cell_inside(const float* s_val, const uint8_t* s_ok, int c, float level, int lc[3]) const {
    lc[0] = c % B, lc[1] = (c / B) % B, lc[2] = c / (B * B);
    if (c >= CELLS) return 0;
#pragma unroll
    for (int k = 0; k < 3; k++)
      if (x0[k] + lc[k] + 1 > n[k] - 1) return 0;
    if (MASKED) {
      bool all = true;
#pragma unroll
      for (int o = 0; o < 8; o++) all = all && s_ok[local(lc[0] + (o & 1), lc[1] + ((o >> 1) & 1), lc[2] + ((o >> 2) & 1))] != 0;
      if (!all) return 0;
    }
    int m = 0;
#pragma unroll
    for (int o = 0; o < 8; o++)
      m |= (mesh_inside(s_val[local(lc[0] + (o & 1), lc[1] + ((o >> 1) & 1), lc[2] + ((o >> 2) & 1))], level) ? 1 : 0) << o;
    return m;
  }
};

// sum of v over the block's 256 threads (s_wave: 4 ints of LDS); every thread calls it
__device__ __forceinline__ int block_sum_256(int v, int* s_wave) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
  __syncthreads();  // (an earlier use of s_wave is over)
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  return s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// exclusive prefix sum of v in thread order over the block's 256 threads, *total = the block's sum; every thread calls it
__device__ __forceinline__ int block_scan_256(int v, int* s_wave, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc, d);
    if (lane >= d) inc += up;
  }
  __syncthreads();  // (an earlier use of s_wave is over)
  if (lane == 63) s_wave[w] = inc;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int s = s_wave[k];
    base += k < w ? s : 0;
    sum += s;
  }
  *total = sum;
  return base + inc - v;
}

template <int B, bool MASKED>
__global__ void __launch_bounds__(256) brick_mesh_count_kernel(int nx, int ny, int nz, const int32_t* __restrict__ brick_ids,
                                                              const float* __restrict__ values, const uint8_t* __restrict__ valid, float level,
                                                              int32_t* __restrict__ vert_counts, int32_t* __restrict__ face_counts) {
  using Tile = BrickTile<B>;
  __shared__ float s_val[Tile::P];
  __shared__ uint8_t s_ok[MASKED ? Tile::P : 1];
  __shared__ int s_wave[4];
  Tile tile;
  tile.init(nx, ny, nz, brick_ids[blockIdx.x]);
  tile.template stage<MASKED>(values, valid, s_val, s_ok);
  int nv = 0, nf = 0;
  for (int l = threadIdx.x; l < Tile::P; l += 256) nv += __popc(tile.template corner_edges<MASKED>(s_val, s_ok, l, level));
  for (int c = threadIdx.x; c < Tile::CELLS; c += 256) {
    int lc[3];
    nf += cell_face_count(tile.template cell_inside<MASKED>(s_val, s_ok, c, level, lc));
  }
  nv = block_sum_256(nv, s_wave);
  nf = block_sum_256(nf, s_wave);
  if (threadIdx.x == 0) {
    vert_counts[blockIdx.x] = nv;
    face_counts[blockIdx.x] = nf;
  }
}

// vertices: local corners in rounds of 256, a block scan per round; within a corner by edge type
template <int B, bool MASKED>
__global__ void __launch_bounds__(256) brick_vert_emit_kernel(int nx, int ny, int nz, const int32_t* __restrict__ brick_ids,
                                                             const float* __restrict__ values, const uint8_t* __restrict__ valid, float level, float lo0, float lo1, float lo2,
                                                             float step, const long long* __restrict__ vert_start,
                                                             long long* __restrict__ vert_keys, float* __restrict__ verts) {
  using Tile = BrickTile<B>;
  __shared__ float s_val[Tile::P];
  __shared__ uint8_t s_ok[MASKED ? Tile::P : 1];
  __shared__ int s_wave[4];
  Tile tile;
  tile.init(nx, ny, nz, brick_ids[blockIdx.x]);
  tile.template stage<MASKED>(values, valid, s_val, s_ok);
  const int S = Tile::S;
  long long v_base = vert_start[blockIdx.x];
  for (int l0 = 0; l0 < Tile::P; l0 += 256) {
    const int l = l0 + threadIdx.x;
    const uint32_t m = tile.template corner_edges<MASKED>(s_val, s_ok, l, level);
    int total;
    const long long v = v_base + block_scan_256(__popc(m), s_wave, &total);
    v_base += total;
    if (m == 0) continue;  // (m != 0: l < P and the corner is owned)
    const int lx = l % S, ly = (l / S) % S, lz = l / (S * S);
    const int x = tile.x0[0] + lx, y = tile.x0[1] + ly, z = tile.x0[2] + lz;
    const long long corner = corner_index(x, y, z, nx, ny);
    const float ga = s_val[l];
    const float pa[3] = {grid_coord(lo0, step, x), grid_coord(lo1, step, y), grid_coord(lo2, step, z)};
#pragma unroll
    for (int o = 1; o < 8; o++) {
      const int t = c_edge_type[o];
      if (!((m >> t) & 1)) continue;
      const long long slot = v + __popc(m & ((1u << t) - 1u));
      const int dx = o & 1, dy = (o >> 1) & 1, dz = (o >> 2) & 1;
      const float gb = s_val[Tile::local(lx + dx, ly + dy, lz + dz)];
      const float pb[3] = {grid_coord(lo0, step, x + dx), grid_coord(lo1, step, y + dy), grid_coord(lo2, step, z + dz)};
      float p[3];
      mesh_edge_point(level, ga, gb, pa, pb, p);
      vert_keys[slot] = 8 * corner + t;
#pragma unroll
      for (int k = 0; k < 3; k++) verts[slot * 3 + k] = p[k];
    }
  }
}

// faces: owned cells in rounds of 256, a block scan per round; a face names its vertices by their keys
template <int B, bool MASKED>
__global__ void __launch_bounds__(256) brick_face_emit_kernel(int nx, int ny, int nz, const int32_t* __restrict__ brick_ids,
                                                             const float* __restrict__ values, const uint8_t* __restrict__ valid, float level,
                                                             const long long* __restrict__ face_start, long long* __restrict__ face_keys,
                                                             long long* __restrict__ face_vert_keys) {
  using Tile = BrickTile<B>;
  __shared__ float s_val[Tile::P];
  __shared__ uint8_t s_ok[MASKED ? Tile::P : 1];
  __shared__ int s_wave[4];
  Tile tile;
  tile.init(nx, ny, nz, brick_ids[blockIdx.x]);
  tile.template stage<MASKED>(values, valid, s_val, s_ok);
  long long f_base = face_start[blockIdx.x];
  for (int c0 = 0; c0 < Tile::CELLS; c0 += 256) {
    int lc[3];
    const int cm = tile.template cell_inside<MASKED>(s_val, s_ok, c0 + threadIdx.x, level, lc);
    int total;
    long long f = f_base + block_scan_256(cell_face_count(cm), s_wave, &total);
    f_base += total;
    if (cm == 0 || cm == 255) continue;
    const int x = tile.x0[0] + lc[0], y = tile.x0[1] + lc[1], z = tile.x0[2] + lc[2];
    const long long cell = ((long long) z * (ny - 1) + y) * (nx - 1) + x;
    int ordinal = 0;
    cell_faces<long long>(
        cm,
        [&](int oa, int ob) {
          const int low = (oa & ob) == oa ? oa : ob;
          return 8 * (long long) corner_index(x + (low & 1), y + ((low >> 1) & 1), z + ((low >> 2) & 1), nx, ny) + c_edge_type[oa ^ ob];
        },
        [&](long long k0, long long k1, long long k2) {
          face_keys[f] = 16 * cell + ordinal;
          face_vert_keys[f * 3 + 0] = k0;
          face_vert_keys[f * 3 + 1] = k1;
          face_vert_keys[f * 3 + 2] = k2;
          f++;
          ordinal++;
        });
  }
}

// TSDF of the running sums of f2n_tsdf_integrate: positive inside (the mesher's convention), 0 and invalid where too little was seen
__global__ void __launch_bounds__(256) tsdf_finalize_kernel(int64_t n, const float* __restrict__ S, const float* __restrict__ W,
                                                           float min_weight, float* __restrict__ g, uint8_t* __restrict__ valid) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float w = W[i];
  const bool ok = w >= min_weight && w > 0.f;
  valid[i] = ok ? 1 : 0;
  g[i] = ok ? F2N_DIV_RN(-S[i], w) : 0.f;
}

}  // namespace

int f2n_oct_locate_warp(void* stream, int n, const float* pts_world, const void* tree_nodes, const void* transes, float* out_pts_warped,
                        int32_t* out_anchors) {
  if (n < 0 || (n > 0 && (pts_world == nullptr || tree_nodes == nullptr || transes == nullptr || out_pts_warped == nullptr ||
                          out_anchors == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  hipLaunchKernelGGL(oct_locate_warp_kernel<false>, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, pts_world, 0.f, 0.f,
                     0.f, 0.f, 1, 1, 0, (const F2nTreeNode*) tree_nodes, (const F2nTransInfo*) transes, out_pts_warped, out_anchors);
  return f2n_launch_status();
}

int f2n_oct_locate_warp_grid(void* stream, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int first_z, int n_z,
                             const void* tree_nodes, const void* transes, float* out_pts_warped, int32_t* out_anchors) {
  if (lo == nullptr || nx <= 0 || ny <= 0 || nz <= 0 || first_z < 0 || n_z < 0 || first_z + (int64_t) n_z > nz) return F2N_ERR_INVALID_ARG;
  const int64_t n = (int64_t) nx * ny * n_z;
  if (n > 0x7fffffff) return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  if (tree_nodes == nullptr || transes == nullptr || out_pts_warped == nullptr || out_anchors == nullptr) return F2N_ERR_INVALID_ARG;
  hipLaunchKernelGGL(oct_locate_warp_kernel<true>, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, (int) n, nullptr, lo[0],
                     lo[1], lo[2], step, nx, ny, first_z, (const F2nTreeNode*) tree_nodes, (const F2nTransInfo*) transes, out_pts_warped,
                     out_anchors);
  return f2n_launch_status();
}

int f2n_located_compact(void* stream, int n, const int32_t* anchors, const float* pts_warped, int32_t* counts, int32_t* start_end,
                        int32_t* total, float* out_pts, int32_t* out_vol, int32_t* out_src) {
  if (n < 0 || anchors == nullptr || pts_warped == nullptr || counts == nullptr || start_end == nullptr || total == nullptr ||
      out_pts == nullptr || out_vol == nullptr)
    return F2N_ERR_INVALID_ARG;
  if (n > 0) {
    hipLaunchKernelGGL(located_count_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, anchors, counts);
    int e = f2n_launch_status();
    if (e != F2N_OK) return e;
  }
  int e = f2n_segment_scan(stream, n, counts, start_end, total);
  if (e != F2N_OK || n == 0) return e;
  hipLaunchKernelGGL(located_compact_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, anchors, pts_warped,
                     start_end, out_pts, out_vol, out_src);
  return f2n_launch_status();
}

int f2n_density_scatter(void* stream, int n, const int32_t* anchors, const int32_t* start_end, const float* f0, float* density) {
  if (n < 0 || (n > 0 && (anchors == nullptr || start_end == nullptr || density == nullptr))) return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  hipLaunchKernelGGL(density_scatter_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, anchors, start_end, f0,
                     density);
  return f2n_launch_status();
}

static bool mesh_dims_ok(int nx, int ny, int nz) {
  return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t) nx * ny * nz <= 0x7fffffff;
}

template <bool MASKED>
static int mesh_count(void* stream, int nx, int ny, int nz, const float* grid, float level, const uint8_t* valid, uint8_t* edge_mask,
                      int32_t* vert_counts, int32_t* vert_start_end, int32_t* face_counts, int32_t* face_start_end, int32_t* totals) {
  if (!mesh_dims_ok(nx, ny, nz) || grid == nullptr || edge_mask == nullptr || vert_counts == nullptr || vert_start_end == nullptr ||
      face_counts == nullptr || face_start_end == nullptr || totals == nullptr || (MASKED && valid == nullptr))
    return F2N_ERR_INVALID_ARG;
  const int64_t n_corners = (int64_t) nx * ny * nz, n_cells = (int64_t) (nx - 1) * (ny - 1) * (nz - 1);
  hipLaunchKernelGGL(mesh_vert_count_kernel<MASKED>, dim3(f2n_div_up(n_corners, 256)), dim3(256), 0, (hipStream_t) stream, nx, ny, nz, grid,
                     level, valid, edge_mask, vert_counts);
  int e = f2n_launch_status();
  if (e != F2N_OK) return e;
  hipLaunchKernelGGL(mesh_face_count_kernel<MASKED>, dim3(f2n_div_up(n_cells, 256)), dim3(256), 0, (hipStream_t) stream, nx, ny, nz, grid,
                     level, valid, face_counts);
  if ((e = f2n_launch_status()) != F2N_OK) return e;
  if ((e = f2n_segment_scan(stream, (int) n_corners, vert_counts, vert_start_end, totals)) != F2N_OK) return e;
  return f2n_segment_scan(stream, (int) n_cells, face_counts, face_start_end, totals + 1);
}

int f2n_mesh_count(void* stream, int nx, int ny, int nz, const float* grid, float level, uint8_t* edge_mask, int32_t* vert_counts,
                   int32_t* vert_start_end, int32_t* face_counts, int32_t* face_start_end, int32_t* totals) {
  return mesh_count<false>(stream, nx, ny, nz, grid, level, nullptr, edge_mask, vert_counts, vert_start_end, face_counts, face_start_end,
                           totals);
}

int f2n_mesh_count_masked(void* stream, int nx, int ny, int nz, const float* grid, float level, const uint8_t* valid, uint8_t* edge_mask,
                          int32_t* vert_counts, int32_t* vert_start_end, int32_t* face_counts, int32_t* face_start_end, int32_t* totals) {
  return mesh_count<true>(stream, nx, ny, nz, grid, level, valid, edge_mask, vert_counts, vert_start_end, face_counts, face_start_end,
                          totals);
}

int f2n_tsdf_finalize(void* stream, int64_t n, const float* S, const float* W, float min_weight, float* g, uint8_t* valid) {
  if (n < 0 || n > (int64_t) 0x7fffffff * 256 || min_weight != min_weight) return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  if (S == nullptr || W == nullptr || g == nullptr || valid == nullptr) return F2N_ERR_INVALID_ARG;
  hipLaunchKernelGGL(tsdf_finalize_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, S, W, min_weight, g, valid);
  return f2n_launch_status();
}

int f2n_mesh_emit(void* stream, int nx, int ny, int nz, const float* grid, float level, const float* lo /*host [3]*/, float step,
                  const uint8_t* edge_mask, const int32_t* vert_start_end, const int32_t* face_start_end, float* verts, int32_t* faces) {
  if (!mesh_dims_ok(nx, ny, nz) || grid == nullptr || lo == nullptr || edge_mask == nullptr || vert_start_end == nullptr ||
      face_start_end == nullptr || verts == nullptr || faces == nullptr)
    return F2N_ERR_INVALID_ARG;
  const int64_t n_corners = (int64_t) nx * ny * nz, n_cells = (int64_t) (nx - 1) * (ny - 1) * (nz - 1);
  hipLaunchKernelGGL(mesh_vert_emit_kernel, dim3(f2n_div_up(n_corners, 256)), dim3(256), 0, (hipStream_t) stream, nx, ny, nz, grid, level,
                     lo[0], lo[1], lo[2], step, edge_mask, vert_start_end, verts);
  int e = f2n_launch_status();
  if (e != F2N_OK) return e;
  hipLaunchKernelGGL(mesh_face_emit_kernel, dim3(f2n_div_up(n_cells, 256)), dim3(256), 0, (hipStream_t) stream, nx, ny, nz, grid, level,
                     edge_mask, vert_start_end, face_start_end, faces);
  return f2n_launch_status();
}

// the brick grid of (n, B), or the status that refuses it
static int brick_grid(const float* lo, float step, int nx, int ny, int nz, int B, BrickGrid* g, int64_t* n_total) {
  if (nx < 2 || ny < 2 || nz < 2 || nx > F2N_BRICK_MAX_POINTS || ny > F2N_BRICK_MAX_POINTS || nz > F2N_BRICK_MAX_POINTS) return F2N_ERR_INVALID_ARG;
  if (B != 4 && B != 8 && B != 16) return F2N_ERR_INVALID_ARG;
  const int n[3] = {nx, ny, nz};
  for (int k = 0; k < 3; k++) {
    g->lo[k] = lo != nullptr ? lo[k] : 0.f;
    g->n[k] = n[k];
    g->nb[k] = (n[k] - 1 + B - 1) / B;
  }
  g->step = step;
  g->B = B;
  *n_total = (int64_t) g->nb[0] * g->nb[1] * g->nb[2];
  return *n_total > 0x7fffffff ? F2N_ERR_UNSUPPORTED : F2N_OK;
}

int f2n_brick_mark(void* stream, const void* tree_nodes, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int B,
                   uint8_t* flags) {
  if (tree_nodes == nullptr || lo == nullptr || flags == nullptr) return F2N_ERR_INVALID_ARG;
  BrickGrid g;
  int64_t n_total;
  const int e = brick_grid(lo, step, nx, ny, nz, B, &g, &n_total);
  if (e != F2N_OK) return e;
  hipLaunchKernelGGL(brick_mark_kernel, dim3(f2n_div_up(n_total, F2N_BRICK_MARK_THREADS)), dim3(F2N_BRICK_MARK_THREADS), 0,
                     (hipStream_t) stream, g, n_total, (const F2nTreeNode*) tree_nodes, flags);
  return f2n_launch_status();
}

int f2n_oct_locate_warp_bricks(void* stream, const float* lo /*host [3]*/, float step, int nx, int ny, int nz, int B, int n_bricks,
                               const int32_t* brick_ids, const void* tree_nodes, const void* transes, float* out_pts_warped,
                               int32_t* out_anchors) {
  if (lo == nullptr || n_bricks < 0) return F2N_ERR_INVALID_ARG;
  BrickGrid g;
  int64_t n_total;
  const int e = brick_grid(lo, step, nx, ny, nz, B, &g, &n_total);
  if (e != F2N_OK) return e;
  const int64_t n = (int64_t) n_bricks * (B + 1) * (B + 1) * (B + 1);
  if (n > 0x7fffffff) return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  if (brick_ids == nullptr || tree_nodes == nullptr || transes == nullptr || out_pts_warped == nullptr || out_anchors == nullptr)
    return F2N_ERR_INVALID_ARG;
  hipLaunchKernelGGL(oct_locate_warp_bricks_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, g, n_total, n, brick_ids,
                     (const F2nTreeNode*) tree_nodes, (const F2nTransInfo*) transes, out_pts_warped, out_anchors);
  return f2n_launch_status();
}

// valid == nullptr: the unmasked kernels (f2n_brick_mesh_count / _emit), else the masked ones
static int brick_mesh_count(void* stream, int nx, int ny, int nz, int B, int n_bricks, const int32_t* brick_ids, const float* values,
                            const uint8_t* valid, bool masked, float level, int32_t* vert_counts, int32_t* face_counts) {
  BrickGrid g;
  int64_t n_total;
  const int e = brick_grid(nullptr, 1.f, nx, ny, nz, B, &g, &n_total);
  if (e != F2N_OK) return e;
  if (n_bricks < 0) return F2N_ERR_INVALID_ARG;
  if (n_bricks == 0) return F2N_OK;
  if (brick_ids == nullptr || values == nullptr || vert_counts == nullptr || face_counts == nullptr || (masked && valid == nullptr))
    return F2N_ERR_INVALID_ARG;
#define F2N_BRICK_COUNT(BB, MM)                                                                                                          \
  hipLaunchKernelGGL((brick_mesh_count_kernel<BB, MM>), dim3(n_bricks), dim3(256), 0, (hipStream_t) stream, nx, ny, nz, brick_ids, values, \
                     valid, level, vert_counts, face_counts)
  if (masked) {
    if (B == 4) F2N_BRICK_COUNT(4, true);
    else if (B == 8) F2N_BRICK_COUNT(8, true);
    else F2N_BRICK_COUNT(16, true);
  } else {
    if (B == 4) F2N_BRICK_COUNT(4, false);
    else if (B == 8) F2N_BRICK_COUNT(8, false);
    else F2N_BRICK_COUNT(16, false);
  }
#undef F2N_BRICK_COUNT
  return f2n_launch_status();
}

static int brick_mesh_emit(void* stream, int nx, int ny, int nz, int B, int n_bricks, const int32_t* brick_ids, const float* values,
                           const uint8_t* valid, bool masked, float level, const float* lo /*host [3]*/, float step,
                           const int64_t* vert_start, const int64_t* face_start, int64_t* vert_keys, float* verts, int64_t* face_keys,
                           int64_t* face_vert_keys) {
  if (lo == nullptr) return F2N_ERR_INVALID_ARG;
  BrickGrid g;
  int64_t n_total;
  const int e = brick_grid(lo, step, nx, ny, nz, B, &g, &n_total);
  if (e != F2N_OK) return e;
  if (n_bricks < 0) return F2N_ERR_INVALID_ARG;
  if (n_bricks == 0) return F2N_OK;
  if (brick_ids == nullptr || values == nullptr || vert_start == nullptr || face_start == nullptr || vert_keys == nullptr ||
      verts == nullptr || face_keys == nullptr || face_vert_keys == nullptr || (masked && valid == nullptr))
    return F2N_ERR_INVALID_ARG;
#define F2N_BRICK_EMIT(BB, MM)                                                                                                             \
  do {                                                                                                                                     \
    hipLaunchKernelGGL((brick_vert_emit_kernel<BB, MM>), dim3(n_bricks), dim3(256), 0, (hipStream_t) stream, nx, ny, nz, brick_ids, values, \
                       valid, level, lo[0], lo[1], lo[2], step, (const long long*) vert_start, (long long*) vert_keys, verts);            \
    hipLaunchKernelGGL((brick_face_emit_kernel<BB, MM>), dim3(n_bricks), dim3(256), 0, (hipStream_t) stream, nx, ny, nz, brick_ids, values, \
                       valid, level, (const long long*) face_start, (long long*) face_keys, (long long*) face_vert_keys);                 \
  } while (0)
  if (masked) {
    if (B == 4) F2N_BRICK_EMIT(4, true);
    else if (B == 8) F2N_BRICK_EMIT(8, true);
    else F2N_BRICK_EMIT(16, true);
  } else {
    if (B == 4) F2N_BRICK_EMIT(4, false);
    else if (B == 8) F2N_BRICK_EMIT(8, false);
    else F2N_BRICK_EMIT(16, false);
  }
#undef F2N_BRICK_EMIT
  return f2n_launch_status();
}

int f2n_brick_mesh_count(void* stream, int nx, int ny, int nz, int B, int n_bricks, const int32_t* brick_ids, const float* values,
                         float level, int32_t* vert_counts, int32_t* face_counts) {
  return brick_mesh_count(stream, nx, ny, nz, B, n_bricks, brick_ids, values, nullptr, false, level, vert_counts, face_counts);
}

int f2n_brick_mesh_emit(void* stream, int nx, int ny, int nz, int B, int n_bricks, const int32_t* brick_ids, const float* values,
                        float level, const float* lo /*host [3]*/, float step, const int64_t* vert_start, const int64_t* face_start,
                        int64_t* vert_keys, float* verts, int64_t* face_keys, int64_t* face_vert_keys) {
  return brick_mesh_emit(stream, nx, ny, nz, B, n_bricks, brick_ids, values, nullptr, false, level, lo, step, vert_start, face_start, vert_keys,
                         verts, face_keys, face_vert_keys);
}

int f2n_brick_mesh_count_masked(void* stream, int nx, int ny, int nz, int B, int n_bricks, const int32_t* brick_ids, const float* values,
                                const uint8_t* valid, float level, int32_t* vert_counts, int32_t* face_counts) {
  return brick_mesh_count(stream, nx, ny, nz, B, n_bricks, brick_ids, values, valid, true, level, vert_counts, face_counts);
}

int f2n_brick_mesh_emit_masked(void* stream, int nx, int ny, int nz, int B, int n_bricks, const int32_t* brick_ids, const float* values,
                               const uint8_t* valid, float level, const float* lo /*host [3]*/, float step, const int64_t* vert_start,
                               const int64_t* face_start, int64_t* vert_keys, float* verts, int64_t* face_keys, int64_t* face_vert_keys) {
  return brick_mesh_emit(stream, nx, ny, nz, B, n_bricks, brick_ids, values, valid, true, level, lo, step, vert_start, face_start, vert_keys,
                         verts, face_keys, face_vert_keys);
}

// =====================================================================================================================
// Mesh attributes (include/f2n_abi.h, "World-space queries and meshes"): radiance at world points, normals from the density
// grid, connected components of a triangle mesh and the removal of the small ones.
//   radiance:   the scatter of the compacted (f0, rgb) rows back to every queried point, zeros for the empty ones
//   normals:    one thread per point: central differences at the eight corners of the point's cell, blended trilinearly
//   components: a parent array over the vertices; every face hooks the larger roots of its vertices under the smallest
//               (atomicMin), a pointer-jumping pass flattens the trees, rounds repeat until a round hooks nothing.
//               parent[v] <= v at all times and a parent is always a vertex of the same component, so the fixpoint --
//               every vertex points at the smallest index of its component -- does not depend on the schedule.
//   filter:     face counts per label -> keep flags -> f2n_segment_scan -> emit, order preserving
// =====================================================================================================================
namespace {

__global__ void __launch_bounds__(256) radiance_scatter_kernel(int n, const int32_t* __restrict__ anchors, const int32_t* __restrict__ start_end,
                                                              const float* __restrict__ f0, const float* __restrict__ rgb_rows,
                                                              float* __restrict__ density, float* __restrict__ rgb) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool hit = anchors[i * 3] >= 0;
  const int64_t k = hit ? start_end[i * 2] : 0;
  density[i] = hit ? expf(f0[k] - F2N_DENSITY_SHIFT) : 0.f;  // (the expression of density_scatter_kernel: the same bits)
#pragma unroll
  for (int c = 0; c < 3; c++) rgb[i * 3 + c] = hit ? rgb_rows[k * 3 + c] : 0.f;
}

// density_scatter_kernel with the analytic gradient: sigma (the same expression, the same bits) and sigma * J^T * df0/dw, J = the
// leaf's warp Jacobian at the world point; optionally the unit normal -grad / |grad| by the rule of grid_normals_kernel.
__global__ void __launch_bounds__(256) density_grad_scatter_kernel(int n, const float* __restrict__ pts_world, const int32_t* __restrict__ anchors,
                                                                  const int32_t* __restrict__ start_end, const F2nTransInfo* __restrict__ transes,
                                                                  const float* __restrict__ f0, const float* __restrict__ df0_dw,
                                                                  float* __restrict__ density, float* __restrict__ grad,
                                                                  float* __restrict__ normal) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = anchors[i * 3];
  float sigma = 0.f, gr[3] = {0.f, 0.f, 0.f};
  if (t >= 0) {
    const int64_t k = start_end[i * 2];
    sigma = expf(f0[k] - F2N_DENSITY_SHIFT);
    const float p[3] = {pts_world[i * 3], pts_world[i * 3 + 1], pts_world[i * 3 + 2]};
    const float g[3] = {df0_dw[k * 3], df0_dw[k * 3 + 1], df0_dw[k * 3 + 2]};
    float jg[3];
    f2n_warp_jac_t_mul(transes + t, p, g, jg);  // (shared with composite_geometry_kernel, render.hip)
#pragma unroll
    for (int c = 0; c < 3; c++) gr[c] = sigma * jg[c];
  }
  density[i] = sigma;
#pragma unroll
  for (int c = 0; c < 3; c++) grad[i * 3 + c] = gr[c];
  if (normal != nullptr) {
    float nr[3];
    f2n_unit3<true>(gr, nr);
#pragma unroll
    for (int c = 0; c < 3; c++) normal[i * 3 + c] = nr[c];
  }
}

// Component `axis` of the corner gradient G at corner (x, y, z): central difference over 2 step in the interior, the one-sided
// difference over step on the two border planes of that axis.
__device__ __forceinline__ float corner_gradient(const float* __restrict__ g, int x, int y, int z, int nx, int ny, int nz, int axis,
                                                 float step) {
  const int i = axis == 0 ? x : axis == 1 ? y : z;
  const int n = axis == 0 ? nx : axis == 1 ? ny : nz;
  const int64_t stride = axis == 0 ? 1 : axis == 1 ? (int64_t) nx : (int64_t) nx * ny;
  const int64_t c = corner_index(x, y, z, nx, ny);
  if (i == 0) return F2N_DIV_RN(F2N_SUB_RN(g[c + stride], g[c]), step);
  if (i == n - 1) return F2N_DIV_RN(F2N_SUB_RN(g[c], g[c - stride]), step);
  return F2N_DIV_RN(F2N_SUB_RN(g[c + stride], g[c - stride]), F2N_MUL_RN(2.f, step));
}

__device__ __forceinline__ float lerp_rn(float a, float b, float f) {  // a (1 - f) + b f, four roundings
  return F2N_ADD_RN(F2N_MUL_RN(a, F2N_SUB_RN(1.f, f)), F2N_MUL_RN(b, f));
}

__global__ void __launch_bounds__(256) grid_normals_kernel(int n, const float* __restrict__ pts, const float* __restrict__ g, int nx, int ny,
                                                          int nz, float lo0, float lo1, float lo2, float step, float* __restrict__ out) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float lo[3] = {lo0, lo1, lo2};
  const int dim[3] = {nx, ny, nz};
  int c[3];
  float f[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    float u = F2N_DIV_RN(F2N_SUB_RN(pts[i * 3 + k], lo[k]), step);
    u = fminf(fmaxf(u, 0.f), (float) (dim[k] - 1));  // (NaN -> 0: the cell stays inside the grid whatever the point)
    const int cell = (int) floorf(u);
    c[k] = cell < dim[k] - 2 ? cell : dim[k] - 2;
    f[k] = F2N_SUB_RN(u, (float) c[k]);
  }
  float grad[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    float G[8];
#pragma unroll
    for (int o = 0; o < 8; o++)
      G[o] = corner_gradient(g, c[0] + (o & 1), c[1] + ((o >> 1) & 1), c[2] + ((o >> 2) & 1), nx, ny, nz, k, step);
    // along x, then y, then z
    const float y0 = lerp_rn(lerp_rn(G[0], G[1], f[0]), lerp_rn(G[2], G[3], f[0]), f[1]);
    const float y1 = lerp_rn(lerp_rn(G[4], G[5], f[0]), lerp_rn(G[6], G[7], f[0]), f[1]);
    grad[k] = lerp_rn(y0, y1, f[2]);
  }
  const float len = sqrtf(F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(grad[0], grad[0]), F2N_MUL_RN(grad[1], grad[1])), F2N_MUL_RN(grad[2], grad[2])));
  const bool ok = len > 0.f && len < __builtin_huge_valf();  // (false for NaN as well)
#pragma unroll
  for (int k = 0; k < 3; k++) out[i * 3 + k] = ok ? -F2N_DIV_RN(grad[k], len) : 0.f;
}

// ---- connected components ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) comp_init_kernel(int n_verts, int32_t* parent) {
  const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n_verts) parent[v] = (int32_t) v;
}

// Root of v.  Other threads lower parents while this one walks: every value read is an ancestor-or-self of a smaller or equal
// index in the same component, and the walk strictly descends, so it ends at a vertex that was a root when it was read.
__device__ __forceinline__ int comp_root(const int32_t* parent, int v) {
  for (;;) {
    const int p = __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == v) return v;
    v = p;
  }
}

__device__ __forceinline__ bool face_in_range(const int32_t* __restrict__ faces, int64_t f, int n_verts, int* a, int* b, int* c) {
  *a = faces[f * 3 + 0];
  *b = faces[f * 3 + 1];
  *c = faces[f * 3 + 2];
  return *a >= 0 && *a < n_verts && *b >= 0 && *b < n_verts && *c >= 0 && *c < n_verts;
}

__global__ void __launch_bounds__(256) comp_hook_kernel(int n_faces, int n_verts, const int32_t* __restrict__ faces, int32_t* parent,
                                                       int32_t* changed) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int a, b, c;
  if (!face_in_range(faces, f, n_verts, &a, &b, &c)) return;
  const int ra = comp_root(parent, a), rb = comp_root(parent, b), rc = comp_root(parent, c);
  const int mab = ra < rb ? ra : rb, m = mab < rc ? mab : rc;
  if (ra == m && rb == m && rc == m) return;
  // (a root that another face has hooked in the meantime keeps the smaller of the two parents; the link this face wanted is
  // found missing by the next round, which is why rounds repeat until none hooks)
  if (ra != m) atomicMin(parent + ra, m);
  if (rb != m) atomicMin(parent + rb, m);
  if (rc != m) atomicMin(parent + rc, m);
  *changed = 1;  // (benign race: every writer stores 1)
}

__global__ void __launch_bounds__(256) comp_jump_kernel(int n_verts, int32_t* parent) {
  const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_verts) return;
  const int r = comp_root(parent, (int) v);
  if (r != (int) v) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- removal of small components -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) comp_size_kernel(int n_faces, int n_verts, const int32_t* __restrict__ faces,
                                                       const int32_t* __restrict__ labels, int32_t* comp_faces) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  int a, b, c, l = -1;
  if (f < n_faces && face_in_range(faces, f, n_verts, &a, &b, &c)) l = labels[a];
  bool todo = l >= 0 && l < n_verts;
  // One atomic per distinct label of a wave, not per face: neighbouring faces share their component, and a scene's main surface
  // would otherwise send millions of adds to one address (measured: 387 ms of a 256^3 extraction).
  const int lane = threadIdx.x & 63;
  for (;;) {
    const unsigned long long rem = __ballot(todo);
    if (rem == 0) break;
    const int leader = __ffsll((long long) rem) - 1;
    const int l0 = __shfl(l, leader);
    const bool same = todo && l == l0;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(comp_faces + l0, (int32_t) __popcll(m));
    todo = todo && !same;
  }
}

__global__ void __launch_bounds__(256) comp_keep_kernel(int n_faces, int n_verts, const int32_t* __restrict__ faces,
                                                       const int32_t* __restrict__ labels, const int32_t* __restrict__ comp_faces,
                                                       int min_faces, int32_t* vert_keep, int32_t* __restrict__ face_keep) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int a, b, c;
  bool keep = false;
  if (face_in_range(faces, f, n_verts, &a, &b, &c)) {
    const int l = labels[a];
    keep = l >= 0 && l < n_verts && comp_faces[l] >= min_faces;
  }
  face_keep[f] = keep ? 1 : 0;
  if (keep) vert_keep[a] = vert_keep[b] = vert_keep[c] = 1;  // (benign race: every writer stores 1)
}

__global__ void __launch_bounds__(256) filter_vert_emit_kernel(int n_verts, const float* __restrict__ verts, const int32_t* __restrict__ vert_keep,
                                                              const int32_t* __restrict__ vert_se, float* __restrict__ out_verts,
                                                              int32_t* __restrict__ vert_src) {
  const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_verts || vert_keep[v] == 0) return;
  const int64_t k = vert_se[v * 2];
#pragma unroll
  for (int c = 0; c < 3; c++) out_verts[k * 3 + c] = verts[v * 3 + c];
  vert_src[k] = (int32_t) v;
}

__global__ void __launch_bounds__(256) filter_face_emit_kernel(int n_faces, const int32_t* __restrict__ faces, const int32_t* __restrict__ face_keep,
                                                              const int32_t* __restrict__ face_se, const int32_t* __restrict__ vert_se,
                                                              int32_t* __restrict__ out_faces) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces || face_keep[f] == 0) return;  // (a kept face has its three indices in range: comp_keep_kernel)
  const int64_t k = face_se[f * 2];
#pragma unroll
  for (int c = 0; c < 3; c++) out_faces[k * 3 + c] = vert_se[(int64_t) faces[f * 3 + c] * 2];
}

}  // namespace

int f2n_radiance_scatter(void* stream, int n, const int32_t* anchors, const int32_t* start_end, const float* f0, const float* rgb_rows,
                         float* density, float* rgb) {
  if (n < 0 || (n > 0 && (anchors == nullptr || start_end == nullptr || density == nullptr || rgb == nullptr))) return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  hipLaunchKernelGGL(radiance_scatter_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, anchors, start_end, f0,
                     rgb_rows, density, rgb);
  return f2n_launch_status();
}

int f2n_density_grad_scatter(void* stream, int n, const float* pts_world, const int32_t* anchors, const int32_t* start_end,
                             const void* transes, const float* f0, const float* df0_dw, float* out_density, float* out_grad,
                             float* out_normal) {
  if (n < 0 || (n > 0 && (pts_world == nullptr || anchors == nullptr || start_end == nullptr || transes == nullptr || out_density == nullptr ||
                          out_grad == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  hipLaunchKernelGGL(density_grad_scatter_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, pts_world, anchors,
                     start_end, (const F2nTransInfo*) transes, f0, df0_dw, out_density, out_grad, out_normal);
  return f2n_launch_status();
}

int f2n_grid_normals(void* stream, int n, const float* pts, const float* grid, int nx, int ny, int nz, const float* lo /*host [3]*/,
                     float step, float* out) {
  if (n < 0 || !mesh_dims_ok(nx, ny, nz) || lo == nullptr || !(step > 0.f) || (n > 0 && (pts == nullptr || grid == nullptr || out == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  hipLaunchKernelGGL(grid_normals_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, pts, grid, nx, ny, nz, lo[0],
                     lo[1], lo[2], step, out);
  return f2n_launch_status();
}

#define F2N_COMP_MAX_ROUNDS 4096  // (a mesh takes a handful; a round that hooks lowers a parent, so the loop ends in any case)
int f2n_mesh_components(void* stream, int n_verts, int n_faces, const int32_t* faces, int32_t* labels, int32_t* changed, int* rounds) {
  if (n_verts < 0 || n_faces < 0 || (n_verts > 0 && labels == nullptr) || (n_faces > 0 && (faces == nullptr || changed == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (rounds != nullptr) *rounds = 0;
  if (n_verts == 0) return F2N_OK;
  hipStream_t st = (hipStream_t) stream;
  hipLaunchKernelGGL(comp_init_kernel, dim3(f2n_div_up(n_verts, 256)), dim3(256), 0, st, n_verts, labels);
  int e = f2n_launch_status();
  if (e != F2N_OK || n_faces == 0) return e;
  for (int round = 1; round <= F2N_COMP_MAX_ROUNDS; round++) {
    if (hipMemsetAsync(changed, 0, sizeof(int32_t), st) != hipSuccess) return f2n_launch_status();
    hipLaunchKernelGGL(comp_hook_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, st, n_faces, n_verts, faces, labels, changed);
    hipLaunchKernelGGL(comp_jump_kernel, dim3(f2n_div_up(n_verts, 256)), dim3(256), 0, st, n_verts, labels);
    if ((e = f2n_launch_status()) != F2N_OK) return e;
    int32_t flag = 0;
    if (hipMemcpyAsync(&flag, changed, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return f2n_launch_status();
    if (rounds != nullptr) *rounds = round;
    if (flag == 0) return F2N_OK;  // nothing hooked: the jump behind the previous round has flattened every tree
  }
  return F2N_ERR_UNSUPPORTED;
}

int f2n_mesh_filter_count(void* stream, int n_verts, int n_faces, const int32_t* faces, const int32_t* labels, int min_faces,
                          int32_t* comp_faces, int32_t* vert_keep, int32_t* vert_start_end, int32_t* face_keep, int32_t* face_start_end,
                          int32_t* totals) {
  if (n_verts < 0 || n_faces < 0 || totals == nullptr ||
      (n_verts > 0 && (labels == nullptr || comp_faces == nullptr || vert_keep == nullptr || vert_start_end == nullptr)) ||
      (n_faces > 0 && (n_verts == 0 || faces == nullptr || face_keep == nullptr || face_start_end == nullptr)))
    return F2N_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t) stream;
  if (n_verts > 0 && (hipMemsetAsync(comp_faces, 0, sizeof(int32_t) * (size_t) n_verts, st) != hipSuccess ||
                      hipMemsetAsync(vert_keep, 0, sizeof(int32_t) * (size_t) n_verts, st) != hipSuccess))
    return f2n_launch_status();
  int e;
  if (n_faces > 0) {
    const dim3 grid(f2n_div_up(n_faces, 256)), block(256);
    hipLaunchKernelGGL(comp_size_kernel, grid, block, 0, st, n_faces, n_verts, faces, labels, comp_faces);
    hipLaunchKernelGGL(comp_keep_kernel, grid, block, 0, st, n_faces, n_verts, faces, labels, comp_faces, min_faces, vert_keep, face_keep);
    if ((e = f2n_launch_status()) != F2N_OK) return e;
  }
  if ((e = f2n_segment_scan(stream, n_verts, vert_keep, vert_start_end, totals)) != F2N_OK) return e;
  return f2n_segment_scan(stream, n_faces, face_keep, face_start_end, totals + 1);
}

int f2n_mesh_filter_emit(void* stream, int n_verts, int n_faces, const float* verts, const int32_t* faces, const int32_t* vert_keep,
                         const int32_t* vert_start_end, const int32_t* face_keep, const int32_t* face_start_end, float* out_verts,
                         int32_t* vert_src, int32_t* out_faces) {
  if (n_verts < 0 || n_faces < 0 ||
      (n_verts > 0 && (verts == nullptr || vert_keep == nullptr || vert_start_end == nullptr || out_verts == nullptr || vert_src == nullptr)) ||
      (n_faces > 0 && (n_verts == 0 || faces == nullptr || face_keep == nullptr || face_start_end == nullptr || out_faces == nullptr)))
    return F2N_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t) stream;
  if (n_verts > 0)
    hipLaunchKernelGGL(filter_vert_emit_kernel, dim3(f2n_div_up(n_verts, 256)), dim3(256), 0, st, n_verts, verts, vert_keep, vert_start_end,
                       out_verts, vert_src);
  if (n_faces > 0)
    hipLaunchKernelGGL(filter_face_emit_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, st, n_faces, faces, face_keep, face_start_end,
                       vert_start_end, out_faces);
  return f2n_launch_status();
}

// =====================================================================================================================
// Mesh simplification (include/f2n_abi.h, "Mesh simplification by vertex clustering"): cluster keys, the exact fixed-point
// accumulation of the clusters' plane quadrics, the fp64 placement, the re-indexed faces.
//   accumulate: one thread per vertex / per face; the lanes of a wave that add to the same cluster are summed across the wave first
//               (wave_fold, over integers: any order gives the same sum), then lanes 0..N-1 add the N sums to the cluster's row
//               with one atomic instruction -- one 128-byte row segment per cluster and wave instead of N atomics per lane.
//   place:      one thread per cluster, the adjugate of the regularised 3x3 system in named scalars (no private array)
// =====================================================================================================================
namespace {

#define F2N_CLUSTER_SLOTS 16
#define F2N_CLUSTER_MAX_RECORDS (1 << 18)

struct ClusterGrid {
  float lo[3];
  float cell;
  int dims[3];
};

__device__ __forceinline__ bool finite3(const float* p) {
  const float inf = __builtin_huge_valf();
  return fabsf(p[0]) < inf && fabsf(p[1]) < inf && fabsf(p[2]) < inf;  // (false for NaN as well)
}

// cell index of coordinate p along axis k
__device__ __forceinline__ int cluster_cell(const ClusterGrid& g, int k, float p) {
  const float u = floorf(F2N_DIV_RN(F2N_SUB_RN(p, g.lo[k]), g.cell));
  return (int) fminf(fmaxf(u, 0.f), (float) (g.dims[k] - 1));
}

__device__ __forceinline__ float cluster_centre(const ClusterGrid& g, int k, int i) {
  return F2N_ADD_RN(g.lo[k], F2N_MUL_RN(F2N_ADD_RN((float) i, 0.5f), g.cell));
}

// local coordinates of p in its own cell
__device__ __forceinline__ void cluster_local(const ClusterGrid& g, const float* p, float* q) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float c = cluster_centre(g, k, cluster_cell(g, k, p[k]));
    q[k] = fminf(fmaxf(F2N_DIV_RN(F2N_SUB_RN(p[k], c), g.cell), -0.5f), 0.5f);
  }
}

__device__ __forceinline__ long long cluster_quant(float x) { return __double2ll_rn((double) x * 1099511627776.0); }

__global__ void __launch_bounds__(256) cluster_keys_kernel(int n_verts, const float* __restrict__ verts, ClusterGrid g,
                                                          long long* __restrict__ keys) {
  const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_verts) return;
  const float p[3] = {verts[v * 3], verts[v * 3 + 1], verts[v * 3 + 2]};
  long long key = -1;
  if (finite3(p))
    key = ((long long) cluster_cell(g, 2, p[2]) * g.dims[1] + cluster_cell(g, 1, p[1])) * g.dims[0] + cluster_cell(g, 0, p[0]);
  keys[v] = key;
}

// The wave's sums of val[0..N), N a power of two: lane l returns the sum of val[l % N] over all 64 lanes (every lane of the wave must
// call this).  Each of the first log2(N) steps halves what a lane carries -- the lanes of a pair keep one half of the values each
// and send the other, so after the step over lane bit D a lane holds the values whose index agrees with its lane number in the bits
// up to D -- and the remaining steps sum the one value left: N - 1 + (6 - log2 N) shuffles instead of 6 N.  Integers: any order
// gives the same sum.
template <int N, int D>
__device__ __forceinline__ long long wave_fold(long long (&val)[N], int lane) {
  if constexpr (N == 1) {
    long long s = val[0];
#pragma unroll
    for (int d = D; d < 64; d <<= 1) s += __shfl_xor(s, d);
    return s;
  } else {
    const bool up = (lane & D) != 0;
    long long half[N / 2];
#pragma unroll
    for (int j = 0; j < N / 2; j++) {
      const long long keep = up ? val[2 * j + 1] : val[2 * j], send = up ? val[2 * j] : val[2 * j + 1];
      half[j] = keep + __shfl_xor(send, D);
    }
    return wave_fold<N / 2, D * 2>(half, lane);
  }
}

// ... then lanes 0..N-1 add sum j to row[first + j] with one atomic instruction.  row is wave-uniform.
template <int N>
__device__ __forceinline__ void wave_sum_add(unsigned long long* row, int first, long long (&val)[N]) {
  const int lane = threadIdx.x & 63;
  const long long mine = wave_fold<N, 1>(val, lane);
  if (lane < N && mine != 0) atomicAdd(row + first + lane, (unsigned long long) mine);
}

__global__ void __launch_bounds__(256) cluster_vert_accumulate_kernel(int n_verts, const float* __restrict__ verts,
                                                                     const int32_t* __restrict__ cluster_of, int n_clusters,
                                                                     ClusterGrid g, unsigned long long* acc) {
  const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  int c = -1;
  long long qq[3] = {0, 0, 0};
  if (v < n_verts) {
    c = cluster_of[v];
    if (c >= 0 && c < n_clusters) {
      const float p[3] = {verts[v * 3], verts[v * 3 + 1], verts[v * 3 + 2]};
      float q[3];
      cluster_local(g, p, q);
#pragma unroll
      for (int k = 0; k < 3; k++) qq[k] = cluster_quant(q[k]);
    } else {
      c = -1;
    }
  }
  bool todo = c >= 0;
  for (;;) {  // (no lane leaves before the wave is done: the sums are taken over all 64 lanes)
    const unsigned long long rem = __ballot(todo);
    if (rem == 0) break;
    const int c0 = __shfl(c, __ffsll((long long) rem) - 1);
    const bool same = todo && c == c0;
    long long val[4] = {same ? qq[0] : 0, same ? qq[1] : 0, same ? qq[2] : 0, same ? 1 : 0};
    wave_sum_add<4>(acc + (int64_t) c0 * F2N_CLUSTER_SLOTS, 12, val);
    todo = todo && !same;
  }
}

__global__ void __launch_bounds__(256) cluster_face_accumulate_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                                     const int32_t* __restrict__ faces,
                                                                     const int32_t* __restrict__ cluster_of, int n_clusters,
                                                                     ClusterGrid g, unsigned long long* acc) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  int c[3] = {-1, -1, -1};
  long long qa[7] = {0, 0, 0, 0, 0, 0, 0};  // quant of A_xx, A_xy, A_xz, A_yy, A_yz, A_zz, w: shared by the face's three corners
  long long qb[3][4];                       // quant of b_x, b_y, b_z, cc per corner
#pragma unroll
  for (int x = 0; x < 3; x++)
#pragma unroll
    for (int k = 0; k < 4; k++) qb[x][k] = 0;
  int ia, ib, ic;
  if (f < n_faces && face_in_range(faces, f, n_verts, &ia, &ib, &ic)) {
    const int id[3] = {ia, ib, ic};
    float p[3][3];
    bool ok = true;
#pragma unroll
    for (int x = 0; x < 3; x++) {
      c[x] = cluster_of[id[x]];
      ok = ok && c[x] >= 0 && c[x] < n_clusters;
#pragma unroll
      for (int k = 0; k < 3; k++) p[x][k] = verts[(int64_t) id[x] * 3 + k];
    }
    float e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      e1[k] = F2N_DIV_RN(F2N_SUB_RN(p[1][k], p[0][k]), g.cell);
      e2[k] = F2N_DIV_RN(F2N_SUB_RN(p[2][k], p[0][k]), g.cell);
    }
    const float n[3] = {F2N_SUB_RN(F2N_MUL_RN(e1[1], e2[2]), F2N_MUL_RN(e1[2], e2[1])),
                        F2N_SUB_RN(F2N_MUL_RN(e1[2], e2[0]), F2N_MUL_RN(e1[0], e2[2])),
                        F2N_SUB_RN(F2N_MUL_RN(e1[0], e2[1]), F2N_MUL_RN(e1[1], e2[0]))};
    const float l = sqrtf(F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(n[0], n[0]), F2N_MUL_RN(n[1], n[1])), F2N_MUL_RN(n[2], n[2])));
    ok = ok && l > 0.f && l < __builtin_huge_valf();
    if (ok) {
      const float w = fminf(F2N_MUL_RN(l, 0.5f), 16.f);
      const float u[3] = {F2N_DIV_RN(n[0], l), F2N_DIV_RN(n[1], l), F2N_DIV_RN(n[2], l)};
      const float wu[3] = {F2N_MUL_RN(w, u[0]), F2N_MUL_RN(w, u[1]), F2N_MUL_RN(w, u[2])};
      qa[0] = cluster_quant(F2N_MUL_RN(wu[0], u[0]));
      qa[1] = cluster_quant(F2N_MUL_RN(wu[0], u[1]));
      qa[2] = cluster_quant(F2N_MUL_RN(wu[0], u[2]));
      qa[3] = cluster_quant(F2N_MUL_RN(wu[1], u[1]));
      qa[4] = cluster_quant(F2N_MUL_RN(wu[1], u[2]));
      qa[5] = cluster_quant(F2N_MUL_RN(wu[2], u[2]));
      qa[6] = cluster_quant(w);
#pragma unroll
      for (int x = 0; x < 3; x++) {
        float q[3];
        cluster_local(g, p[x], q);
        const float d = -F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(u[0], q[0]), F2N_MUL_RN(u[1], q[1])), F2N_MUL_RN(u[2], q[2]));
        const float wd = F2N_MUL_RN(w, d);
#pragma unroll
        for (int k = 0; k < 3; k++) qb[x][k] = cluster_quant(F2N_MUL_RN(wd, u[k]));
        qb[x][3] = cluster_quant(F2N_MUL_RN(wd, d));
      }
    } else {
      c[0] = c[1] = c[2] = -1;
    }
  }
  // One round per distinct cluster among the wave's pending corners (the three corners of a face together: neighbouring faces and
  // the corners of one face mostly share their cluster).  A lane with k corners in the round's cluster adds k times the face's
  // shared terms and the sum of those corners' own terms: integers, so this is what k single records would have added.
  bool t0 = c[0] >= 0, t1 = c[1] >= 0, t2 = c[2] >= 0;
  for (;;) {
    const unsigned long long rem = __ballot(t0 || t1 || t2);
    if (rem == 0) break;
    const int c0 = __shfl(t0 ? c[0] : t1 ? c[1] : c[2], __ffsll((long long) rem) - 1);
    const bool m0 = t0 && c[0] == c0, m1 = t1 && c[1] == c0, m2 = t2 && c[2] == c0;
    const long long k = (m0 ? 1 : 0) + (m1 ? 1 : 0) + (m2 ? 1 : 0);
    long long val[16];  // (12 sums, padded to a power of two)
#pragma unroll
    for (int j = 12; j < 16; j++) val[j] = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) val[j] = k * qa[j];
#pragma unroll
    for (int j = 0; j < 4; j++) val[6 + j] = (m0 ? qb[0][j] : 0) + (m1 ? qb[1][j] : 0) + (m2 ? qb[2][j] : 0);
    val[10] = k * qa[6];
    val[11] = k;
    wave_sum_add<16>(acc + (int64_t) c0 * F2N_CLUSTER_SLOTS, 0, val);
    t0 = t0 && !m0;
    t1 = t1 && !m1;
    t2 = t2 && !m2;
  }
}

__global__ void __launch_bounds__(256) cluster_guard_kernel(int n_clusters, const long long* __restrict__ acc, int32_t* flag) {
  const int64_t c = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_clusters) return;
  if (acc[c * F2N_CLUSTER_SLOTS + 11] > F2N_CLUSTER_MAX_RECORDS || acc[c * F2N_CLUSTER_SLOTS + 15] > F2N_CLUSTER_MAX_RECORDS)
    *flag = 1;  // (benign race: every writer stores 1)
}

__global__ void __launch_bounds__(256) cluster_place_kernel(int n_clusters, const long long* __restrict__ acc,
                                                           const long long* __restrict__ cluster_keys, ClusterGrid g, double lambda,
                                                           float* __restrict__ out) {
  const int64_t c = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_clusters) return;
  const long long* a = acc + c * F2N_CLUSTER_SLOTS;
  const double s = 1.0 / 1099511627776.0;  // 2^-40
  const double cnt = (double) a[15];
  const double mx = ((double) a[12] * s) / cnt, my = ((double) a[13] * s) / cnt, mz = ((double) a[14] * s) / cnt;
  const double W = (double) a[10] * s;
  double qx = mx, qy = my, qz = mz;
  if (W > 0.0) {
    const double gl = lambda * W;
    const double Mxx = (double) a[0] * s + gl, Mxy = (double) a[1] * s, Mxz = (double) a[2] * s;
    const double Myy = (double) a[3] * s + gl, Myz = (double) a[4] * s, Mzz = (double) a[5] * s + gl;
    const double rx = gl * mx - (double) a[6] * s, ry = gl * my - (double) a[7] * s, rz = gl * mz - (double) a[8] * s;
    const double C00 = Myy * Mzz - Myz * Myz, C01 = Mxz * Myz - Mxy * Mzz, C02 = Mxy * Myz - Mxz * Myy;
    const double C11 = Mxx * Mzz - Mxz * Mxz, C12 = Mxy * Mxz - Mxx * Myz, C22 = Mxx * Myy - Mxy * Mxy;
    const double det = Mxx * C00 + (Mxy * C01 + Mxz * C02);
    if (det > 0.0 && det < __builtin_huge_val()) {
      qx = (C00 * rx + (C01 * ry + C02 * rz)) / det;
      qy = (C01 * rx + (C11 * ry + C12 * rz)) / det;
      qz = (C02 * rx + (C12 * ry + C22 * rz)) / det;
    }
  }
  const long long key = cluster_keys[c];
  const int ix = (int) (key % g.dims[0]), iy = (int) ((key / g.dims[0]) % g.dims[1]), iz = (int) (key / ((long long) g.dims[0] * g.dims[1]));
  out[c * 3 + 0] = F2N_ADD_RN(cluster_centre(g, 0, ix), F2N_MUL_RN(g.cell, (float) fmin(fmax(qx, -0.5), 0.5)));
  out[c * 3 + 1] = F2N_ADD_RN(cluster_centre(g, 1, iy), F2N_MUL_RN(g.cell, (float) fmin(fmax(qy, -0.5), 0.5)));
  out[c * 3 + 2] = F2N_ADD_RN(cluster_centre(g, 2, iz), F2N_MUL_RN(g.cell, (float) fmin(fmax(qz, -0.5), 0.5)));
}

__global__ void __launch_bounds__(256) cluster_faces_kernel(int n_verts, int n_faces, const int32_t* __restrict__ faces,
                                                           const int32_t* __restrict__ cluster_of, int32_t* __restrict__ out) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int a, b, c;
  int r0 = -1, r1 = -1, r2 = -1;
  if (face_in_range(faces, f, n_verts, &a, &b, &c)) {
    const int ca = cluster_of[a], cb = cluster_of[b], cc = cluster_of[c];
    if (ca >= 0 && cb >= 0 && cc >= 0 && ca != cb && cb != cc && ca != cc) {
      if (ca < cb && ca < cc) {
        r0 = ca; r1 = cb; r2 = cc;
      } else if (cb < cc) {
        r0 = cb; r1 = cc; r2 = ca;
      } else {
        r0 = cc; r1 = ca; r2 = cb;
      }
    }
  }
  out[f * 3 + 0] = r0;
  out[f * 3 + 1] = r1;
  out[f * 3 + 2] = r2;
}

bool cluster_grid_ok(const float* lo, float cell, const int32_t* dims, ClusterGrid* g) {
  if (lo == nullptr || dims == nullptr || !(cell > 0.f) || !(cell < __builtin_huge_valf())) return false;
  for (int k = 0; k < 3; k++) {
    if (!(fabsf(lo[k]) < __builtin_huge_valf()) || dims[k] < 1 || dims[k] > (1 << 20)) return false;
    g->lo[k] = lo[k];
    g->dims[k] = dims[k];
  }
  g->cell = cell;
  return true;
}

}  // namespace

int f2n_mesh_cluster_keys(void* stream, int n_verts, const float* verts, const float* lo, float cell, const int32_t* dims, int64_t* keys) {
  ClusterGrid g;
  if (n_verts < 0 || !cluster_grid_ok(lo, cell, dims, &g) || (n_verts > 0 && (verts == nullptr || keys == nullptr))) return F2N_ERR_INVALID_ARG;
  if (n_verts == 0) return F2N_OK;
  hipLaunchKernelGGL(cluster_keys_kernel, dim3(f2n_div_up(n_verts, 256)), dim3(256), 0, (hipStream_t) stream, n_verts, verts, g,
                     (long long*) keys);
  return f2n_launch_status();
}

int f2n_mesh_cluster_accumulate(void* stream, int n_verts, int n_faces, const float* verts, const int32_t* faces, const int32_t* cluster_of,
                                int n_clusters, const float* lo, float cell, const int32_t* dims, int64_t* acc, int32_t* flag) {
  ClusterGrid g;
  if (n_verts < 0 || n_faces < 0 || n_clusters < 0 || !cluster_grid_ok(lo, cell, dims, &g) ||
      (n_verts > 0 && (verts == nullptr || cluster_of == nullptr)) || (n_faces > 0 && (n_verts == 0 || faces == nullptr)) ||
      (n_clusters > 0 && (acc == nullptr || flag == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n_clusters == 0) return F2N_OK;  // (no cluster: no vertex has one, nothing to add)
  hipStream_t st = (hipStream_t) stream;
  if (hipMemsetAsync(flag, 0, sizeof(int32_t), st) != hipSuccess) return f2n_launch_status();
  if (n_verts > 0)
    hipLaunchKernelGGL(cluster_vert_accumulate_kernel, dim3(f2n_div_up(n_verts, 256)), dim3(256), 0, st, n_verts, verts, cluster_of,
                       n_clusters, g, (unsigned long long*) acc);
  if (n_faces > 0)
    hipLaunchKernelGGL(cluster_face_accumulate_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, st, n_verts, n_faces, verts, faces,
                       cluster_of, n_clusters, g, (unsigned long long*) acc);
  hipLaunchKernelGGL(cluster_guard_kernel, dim3(f2n_div_up(n_clusters, 256)), dim3(256), 0, st, n_clusters, (const long long*) acc, flag);
  int e = f2n_launch_status();
  if (e != F2N_OK) return e;
  int32_t over = 0;
  if (hipMemcpyAsync(&over, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return f2n_launch_status();
  return over != 0 ? F2N_ERR_UNSUPPORTED : F2N_OK;
}

int f2n_mesh_cluster_place(void* stream, int n_clusters, const int64_t* acc, const int64_t* cluster_keys, const float* lo, float cell,
                           const int32_t* dims, double lambda, float* out_verts) {
  ClusterGrid g;
  if (n_clusters < 0 || !cluster_grid_ok(lo, cell, dims, &g) || !(lambda >= 0.0) || !(lambda < __builtin_huge_val()) ||
      (n_clusters > 0 && (acc == nullptr || cluster_keys == nullptr || out_verts == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n_clusters == 0) return F2N_OK;
  hipLaunchKernelGGL(cluster_place_kernel, dim3(f2n_div_up(n_clusters, 256)), dim3(256), 0, (hipStream_t) stream, n_clusters,
                     (const long long*) acc, (const long long*) cluster_keys, g, lambda, out_verts);
  return f2n_launch_status();
}

int f2n_mesh_cluster_faces(void* stream, int n_verts, int n_faces, const int32_t* faces, const int32_t* cluster_of, int32_t* out_faces) {
  if (n_verts < 0 || n_faces < 0 || (n_faces > 0 && (faces == nullptr || out_faces == nullptr || (n_verts > 0 && cluster_of == nullptr))))
    return F2N_ERR_INVALID_ARG;
  if (n_faces == 0) return F2N_OK;
  hipLaunchKernelGGL(cluster_faces_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, (hipStream_t) stream, n_verts, n_faces, faces,
                     cluster_of, out_faces);
  return f2n_launch_status();
}

// =====================================================================================================================
// Mesh ray casting (include/f2n_abi.h, "Ray casting against a triangle mesh"): the Woop-Benthin-Wald test with fp64 edge
// functions, a uniform grid of face lists built without atomics, and two drivers of the one test:
//   brute:    every ray tests every face; a block stages 256 faces at a time in LDS (every lane reads the same face: a broadcast)
//   traverse: one lane per ray walks the grid layer by layer along kz, the axis the test itself picked
// The axis permutation is done with selects (sel3): a private array under a runtime index would live in scratch memory.
// =====================================================================================================================
namespace {

#define F2N_RAYCAST_MAX_CELLS (1 << 27)
#define F2N_RAYCAST_TILE 256
#define F2N_RAYCAST_DOMAIN_CELLS 32768.f  // the traversal is proven for coordinates up to this many cells (f2n_abi.h)

__device__ __forceinline__ float sel3(int k, float a, float b, float c) { return k == 0 ? a : (k == 1 ? b : c); }
__device__ __forceinline__ int sel3i(int k, int a, int b, int c) { return k == 0 ? a : (k == 1 ? b : c); }

struct RayFrame {
  int kx, ky, kz;
  float ox, oy, oz;  // the origin, permuted
  float Sx, Sy, Sz;
  float t_min, t_max;
  bool ok;  // false: the ray hits nothing
};

struct RayHit {
  float t, b0, b1, b2;
  int face;
};

__device__ __forceinline__ RayFrame ray_frame(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                              const float* __restrict__ bounds, int64_t r) {
  const float o0 = rays_o[r * 3], o1 = rays_o[r * 3 + 1], o2 = rays_o[r * 3 + 2];
  const float d[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};  // (only constant indices below: registers)
  RayFrame f;
  int kz = 0;
  float m = fabsf(d[0]);
  if (fabsf(d[1]) > m) { kz = 1; m = fabsf(d[1]); }
  if (fabsf(d[2]) > m) kz = 2;
  int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const float dz = sel3(kz, d[0], d[1], d[2]);
  if (dz < 0.f) { const int s = kx; kx = ky; ky = s; }
  f.ok = finite3(d) && dz != 0.f;
  f.kx = kx; f.ky = ky; f.kz = kz;
  f.Sx = F2N_DIV_RN(sel3(kx, d[0], d[1], d[2]), dz);
  f.Sy = F2N_DIV_RN(sel3(ky, d[0], d[1], d[2]), dz);
  f.Sz = F2N_DIV_RN(1.f, dz);
  f.ox = sel3(kx, o0, o1, o2); f.oy = sel3(ky, o0, o1, o2); f.oz = sel3(kz, o0, o1, o2);
  f.t_min = bounds != nullptr ? bounds[r * 2] : 0.f;
  f.t_max = bounds != nullptr ? bounds[r * 2 + 1] : __builtin_huge_valf();
  return f;
}

// steps 3-8 of the contract for one face (p0, p1, p2: its vertices' x, y, z); keeps the nearer hit, the lower index among equals
__device__ __forceinline__ void ray_face(const RayFrame& f, int face, float a0, float a1, float a2, float b0, float b1, float b2, float c0,
                                         float c1, float c2, RayHit* h) {
#define F2N_RAY_VERT(P0, P1, P2, X, Y, Z)                                     \
  float X, Y, Z;                                                              \
  {                                                                           \
    const float qx = F2N_SUB_RN(sel3(f.kx, P0, P1, P2), f.ox);                \
    const float qy = F2N_SUB_RN(sel3(f.ky, P0, P1, P2), f.oy);                \
    const float qz = F2N_SUB_RN(sel3(f.kz, P0, P1, P2), f.oz);                \
    X = F2N_SUB_RN(qx, F2N_MUL_RN(f.Sx, qz));                                 \
    Y = F2N_SUB_RN(qy, F2N_MUL_RN(f.Sy, qz));                                 \
    Z = F2N_MUL_RN(f.Sz, qz);                                                 \
  }
  F2N_RAY_VERT(a0, a1, a2, Ax, Ay, Az)
  F2N_RAY_VERT(b0, b1, b2, Bx, By, Bz)
  F2N_RAY_VERT(c0, c1, c2, Cx, Cy, Cz)
#undef F2N_RAY_VERT
  const double U = (double) Cx * (double) By - (double) Cy * (double) Bx;
  const double V = (double) Ax * (double) Cy - (double) Ay * (double) Cx;
  const double W = (double) Bx * (double) Ay - (double) By * (double) Ax;
  if (!((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0))) return;  // (a NaN is outside)
  const double det = (U + V) + W;
  if (det == 0.0) return;
  const double T = (U * (double) Az + V * (double) Bz) + W * (double) Cz;
  const float t = (float) (T / det);
  if (!(t > f.t_min && t < f.t_max)) return;
  if (h->face >= 0 && !(t < h->t || (t == h->t && face < h->face))) return;
  h->t = t;
  h->face = face;
  h->b0 = (float) (U / det);
  h->b1 = (float) (V / det);
  h->b2 = (float) (W / det);
}

__device__ __forceinline__ void ray_store(const RayHit& h, int64_t r, float* __restrict__ out_t, int32_t* __restrict__ out_face,
                                          float* __restrict__ out_bary) {
  out_t[r] = h.t;
  out_face[r] = h.face;
  out_bary[r * 3] = h.b0;
  out_bary[r * 3 + 1] = h.b1;
  out_bary[r * 3 + 2] = h.b2;
}

__global__ void __launch_bounds__(256) raycast_check_faces_kernel(int n_verts, int n_faces, const int32_t* __restrict__ faces, int32_t* flag) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int a, b, c;
  if (!face_in_range(faces, f, n_verts, &a, &b, &c)) *flag = 1;  // (benign race: every writer stores 1)
}

__global__ void __launch_bounds__(F2N_RAYCAST_TILE) raycast_brute_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                                        const int32_t* __restrict__ faces, int n_rays,
                                                                        const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                                        const float* __restrict__ bounds, float* __restrict__ out_t,
                                                                        int32_t* __restrict__ out_face, float* __restrict__ out_bary) {
  __shared__ float tile[9][F2N_RAYCAST_TILE];
  const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = r < n_rays;
  RayFrame fr = ray_frame(rays_o, rays_d, bounds, live ? r : 0);
  RayHit h = {0.f, 0.f, 0.f, 0.f, -1};
  for (int base = 0; base < n_faces; base += F2N_RAYCAST_TILE) {
    const int mine = base + (int) threadIdx.x;
    int a, b, c;
    const bool ok = mine < n_faces && face_in_range(faces, mine, n_verts, &a, &b, &c);
    const float nan = __builtin_nanf("");  // (a face that is not there fails every test)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      tile[k][threadIdx.x] = ok ? verts[(int64_t) a * 3 + k] : nan;
      tile[3 + k][threadIdx.x] = ok ? verts[(int64_t) b * 3 + k] : nan;
      tile[6 + k][threadIdx.x] = ok ? verts[(int64_t) c * 3 + k] : nan;
    }
    __syncthreads();
    const int n = min(F2N_RAYCAST_TILE, n_faces - base);
    if (live && fr.ok)
      for (int j = 0; j < n; j++)
        ray_face(fr, base + j, tile[0][j], tile[1][j], tile[2][j], tile[3][j], tile[4][j], tile[5][j], tile[6][j], tile[7][j], tile[8][j], &h);
    __syncthreads();
  }
  if (live) ray_store(h, r, out_t, out_face, out_bary);
}

// cell index of coordinate p along an axis of origin lo and n cells (cluster_cell with the axis already selected): monotone in p
__device__ __forceinline__ int ray_cell(float lo, float cell, int n, float p) {
  const float u = floorf(F2N_DIV_RN(F2N_SUB_RN(p, lo), cell));
  return (int) fminf(fmaxf(u, 0.f), (float) (n - 1));
}

__device__ __forceinline__ float ray_guard(float cell) { return F2N_MUL_RN(cell, 0.0625f); }

// the cells [lo_i, hi_i] per axis that list face f (its bounding box dilated by the guard); false: the face is listed nowhere
__device__ __forceinline__ bool face_cells(const ClusterGrid& g, int n_verts, const float* __restrict__ verts,
                                           const int32_t* __restrict__ faces, int64_t f, int* i0, int* i1) {
  int a, b, c;
  if (!face_in_range(faces, f, n_verts, &a, &b, &c)) return false;
  const float* pa = verts + (int64_t) a * 3;
  const float* pb = verts + (int64_t) b * 3;
  const float* pc = verts + (int64_t) c * 3;
  if (!finite3(pa) || !finite3(pb) || !finite3(pc)) return false;
  const float guard = ray_guard(g.cell);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    i0[k] = ray_cell(g.lo[k], g.cell, g.dims[k], F2N_SUB_RN(fminf(fminf(pa[k], pb[k]), pc[k]), guard));
    i1[k] = ray_cell(g.lo[k], g.cell, g.dims[k], F2N_ADD_RN(fmaxf(fmaxf(pa[k], pb[k]), pc[k]), guard));
  }
  return true;
}

__global__ void __launch_bounds__(256) raycast_count_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                           const int32_t* __restrict__ faces, ClusterGrid g, int32_t* __restrict__ counts,
                                                           int32_t* flag) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int a, b, c;
  if (!face_in_range(faces, f, n_verts, &a, &b, &c)) *flag = 1;  // (benign race: every writer stores 1)
  int i0[3], i1[3];
  counts[f] = face_cells(g, n_verts, verts, faces, f, i0, i1) ? (i1[0] - i0[0] + 1) * (i1[1] - i0[1] + 1) * (i1[2] - i0[2] + 1) : 0;
}

__global__ void __launch_bounds__(256) raycast_fill_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                          const int32_t* __restrict__ faces, ClusterGrid g,
                                                          const long long* __restrict__ offsets, long long* __restrict__ keys) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int i0[3], i1[3];
  if (!face_cells(g, n_verts, verts, faces, f, i0, i1)) return;
  long long at = offsets[f];
  for (int z = i0[2]; z <= i1[2]; z++)
    for (int y = i0[1]; y <= i1[1]; y++)
      for (int x = i0[0]; x <= i1[0]; x++) keys[at++] = (((long long) z * g.dims[1] + y) * g.dims[0] + x) * n_faces + f;
}

__global__ void __launch_bounds__(256) raycast_traverse_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                              const int32_t* __restrict__ faces, ClusterGrid g,
                                                              const int32_t* __restrict__ cell_start, const int32_t* __restrict__ cell_faces,
                                                              int n_rays, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                              const float* __restrict__ bounds, float* __restrict__ out_t,
                                                              int32_t* __restrict__ out_face, float* __restrict__ out_bary) {
  const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const RayFrame fr = ray_frame(rays_o, rays_d, bounds, r);
  RayHit h = {0.f, 0.f, 0.f, 0.f, -1};
  if (fr.ok) {
    const float lox = sel3(fr.kx, g.lo[0], g.lo[1], g.lo[2]), loy = sel3(fr.ky, g.lo[0], g.lo[1], g.lo[2]);
    const float loz = sel3(fr.kz, g.lo[0], g.lo[1], g.lo[2]);
    const int nx = sel3i(fr.kx, g.dims[0], g.dims[1], g.dims[2]), ny = sel3i(fr.ky, g.dims[0], g.dims[1], g.dims[2]);
    const int nz = sel3i(fr.kz, g.dims[0], g.dims[1], g.dims[2]);
    const int s1 = g.dims[0], s2 = g.dims[0] * g.dims[1];
    const int sx = sel3i(fr.kx, 1, s1, s2), sy = sel3i(fr.ky, 1, s1, s2), sz = sel3i(fr.kz, 1, s1, s2);
    const float guard = ray_guard(g.cell), margin = F2N_MUL_RN(fabsf(fr.Sz), guard);
    const bool up = fr.Sz > 0.f;
    for (int step = 0; step < nz; step++) {
      const int L = up ? step : nz - 1 - step;
      const float z_lo = F2N_ADD_RN(loz, F2N_MUL_RN((float) L, g.cell)), z_hi = F2N_ADD_RN(loz, F2N_MUL_RN((float) (L + 1), g.cell));
      const float q_in = F2N_SUB_RN(up ? z_lo : z_hi, fr.oz), q_out = F2N_SUB_RN(up ? z_hi : z_lo, fr.oz);
      const float t_in = F2N_MUL_RN(fr.Sz, q_in), t_out = F2N_MUL_RN(fr.Sz, q_out);
      // every comparison is false for a NaN: the walk then goes on, which is the conservative side
      if (F2N_SUB_RN(t_in, margin) > fr.t_max) break;                   // the window ends before this layer
      if (h.face >= 0 && h.t < F2N_SUB_RN(t_in, margin)) break;         // no face of this or a later layer can be nearer, or as near
      if (F2N_ADD_RN(t_out, margin) < fr.t_min) continue;               // the window begins behind this layer
      const float x_in = F2N_ADD_RN(fr.ox, F2N_MUL_RN(fr.Sx, q_in)), x_out = F2N_ADD_RN(fr.ox, F2N_MUL_RN(fr.Sx, q_out));
      const float y_in = F2N_ADD_RN(fr.oy, F2N_MUL_RN(fr.Sy, q_in)), y_out = F2N_ADD_RN(fr.oy, F2N_MUL_RN(fr.Sy, q_out));
      const int ix0 = ray_cell(lox, g.cell, nx, F2N_SUB_RN(fminf(x_in, x_out), guard));
      const int ix1 = ray_cell(lox, g.cell, nx, F2N_ADD_RN(fmaxf(x_in, x_out), guard));
      const int iy0 = ray_cell(loy, g.cell, ny, F2N_SUB_RN(fminf(y_in, y_out), guard));
      const int iy1 = ray_cell(loy, g.cell, ny, F2N_ADD_RN(fmaxf(y_in, y_out), guard));
      for (int iy = iy0; iy <= iy1; iy++)
        for (int ix = ix0; ix <= ix1; ix++) {
          const int c = L * sz + iy * sy + ix * sx;
          const int e1 = cell_start[c + 1];
          for (int e = cell_start[c]; e < e1; e++) {
            const int f = cell_faces[e];
            int a, b, cc;
            if (f < 0 || f >= n_faces || !face_in_range(faces, f, n_verts, &a, &b, &cc)) continue;
            const float* pa = verts + (int64_t) a * 3;
            const float* pb = verts + (int64_t) b * 3;
            const float* pc = verts + (int64_t) cc * 3;
            ray_face(fr, f, pa[0], pa[1], pa[2], pb[0], pb[1], pb[2], pc[0], pc[1], pc[2], &h);
          }
        }
    }
  }
  ray_store(h, r, out_t, out_face, out_bary);
}

bool raycast_grid_ok(const float* lo, float cell, const int32_t* dims, ClusterGrid* g) {
  if (!cluster_grid_ok(lo, cell, dims, g)) return false;
  return (int64_t) dims[0] * dims[1] * dims[2] <= F2N_RAYCAST_MAX_CELLS;
}

}  // namespace

int f2n_mesh_raycast_count(void* stream, int n_verts, int n_faces, const float* verts, const int32_t* faces, const float* lo, float cell,
                           const int32_t* dims, int32_t* counts, int32_t* flag) {
  ClusterGrid g;
  if (n_verts < 0 || n_faces < 0 || !raycast_grid_ok(lo, cell, dims, &g) ||
      (n_faces > 0 && (n_verts == 0 || verts == nullptr || faces == nullptr || counts == nullptr || flag == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n_faces == 0) return F2N_OK;
  hipStream_t st = (hipStream_t) stream;
  if (hipMemsetAsync(flag, 0, sizeof(int32_t), st) != hipSuccess) return f2n_launch_status();
  hipLaunchKernelGGL(raycast_count_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, st, n_verts, n_faces, verts, faces, g, counts, flag);
  int e = f2n_launch_status();
  if (e != F2N_OK) return e;
  int32_t bad = 0;
  if (hipMemcpyAsync(&bad, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return f2n_launch_status();
  return bad != 0 ? F2N_ERR_INVALID_ARG : F2N_OK;
}

int f2n_mesh_raycast_fill(void* stream, int n_verts, int n_faces, const float* verts, const int32_t* faces, const float* lo, float cell,
                          const int32_t* dims, const int64_t* offsets, int64_t* keys) {
  ClusterGrid g;
  if (n_verts < 0 || n_faces < 0 || !raycast_grid_ok(lo, cell, dims, &g) ||
      (n_faces > 0 && (n_verts == 0 || verts == nullptr || faces == nullptr || offsets == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n_faces == 0 || keys == nullptr) return F2N_OK;  // (keys may be NULL when no face is listed anywhere)
  hipLaunchKernelGGL(raycast_fill_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, (hipStream_t) stream, n_verts, n_faces, verts, faces,
                     g, (const long long*) offsets, (long long*) keys);
  return f2n_launch_status();
}

int f2n_mesh_raycast(void* stream, int n_verts, int n_faces, const float* verts, const int32_t* faces, const float* lo, float cell,
                     const int32_t* dims, const int32_t* cell_start, const int32_t* cell_faces, int n_rays, const float* rays_o,
                     const float* rays_d, const float* bounds, float* out_t, int32_t* out_face, float* out_bary) {
  ClusterGrid g;
  if (n_verts < 0 || n_faces < 0 || n_rays < 0 || (cell_start != nullptr && !raycast_grid_ok(lo, cell, dims, &g)) ||
      (n_faces > 0 && (n_verts == 0 || verts == nullptr || faces == nullptr)) ||
      (n_rays > 0 && (rays_o == nullptr || rays_d == nullptr || out_t == nullptr || out_face == nullptr || out_bary == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (cell_start != nullptr)  // the part of the traversal's domain that is host data: the box within 2^15 cells of the origin of the frame
    for (int k = 0; k < 3; k++)
      if (!(fmaxf(fabsf(lo[k]), fabsf(lo[k] + (float) dims[k] * cell)) <= F2N_RAYCAST_DOMAIN_CELLS * cell)) return F2N_ERR_UNSUPPORTED;
  if (n_rays == 0) return F2N_OK;
  hipStream_t st = (hipStream_t) stream;
  if (n_faces > 0) {  // the index check, with out_face[0] as its flag word
    if (hipMemsetAsync(out_face, 0, sizeof(int32_t), st) != hipSuccess) return f2n_launch_status();
    hipLaunchKernelGGL(raycast_check_faces_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, st, n_verts, n_faces, faces, out_face);
    int32_t bad = 0;
    if (hipMemcpyAsync(&bad, out_face, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return f2n_launch_status();
    if (bad != 0) return F2N_ERR_INVALID_ARG;
  }
  const dim3 grid(f2n_div_up(n_rays, 256)), block(256);
  if (cell_start == nullptr || n_faces == 0)
    hipLaunchKernelGGL(raycast_brute_kernel, grid, block, 0, st, n_verts, n_faces, verts, faces, n_rays, rays_o, rays_d, bounds, out_t, out_face,
                       out_bary);
  else  // (cell_faces may be NULL when every list is empty: it is then never read)
    hipLaunchKernelGGL(raycast_traverse_kernel, grid, block, 0, st, n_verts, n_faces, verts, faces, g, cell_start, cell_faces, n_rays, rays_o,
                       rays_d, bounds, out_t, out_face, out_bary);
  return f2n_launch_status();
}

// =====================================================================================================================
// Mesh-to-mesh distance (include/f2n_abi.h, "Closest point on a triangle mesh" and "Area-uniform surface samples"): the
// fp64 region walk of Ericson 5.1.5 over the ray caster's face grid, and stratified Philox samples of the surface.
//   brute: every point tests every face; a block stages 256 faces at a time in LDS (the device-side oracle)
//   grid:  one lane per point walks Chebyshev shells of cells around the point's own cell until the shell's planes are
//          farther than the face it holds
// One lane owns one point / face / sample: no atomics.  The region walk keeps its barycentrics in named scalars.
// =====================================================================================================================
namespace {

#if defined(__HIP_DEVICE_COMPILE__)
#define F2N_DSQRT_RN(x) __dsqrt_rn(x)
#else
#define F2N_DSQRT_RN(x) sqrt(x)
#endif

struct ClosestHit {
  double d2, b0, b1, b2;
  int face;
};

__device__ __forceinline__ double dot3d(double ax, double ay, double az, double bx, double by, double bz) {
  return (ax * bx + ay * by) + az * bz;
}

// the contract for one (point, face) pair: A, B, C are the face's vertices; keeps the nearer face, the lower index among equals
__device__ __forceinline__ void closest_face(double px, double py, double pz, int face, float a0, float a1, float a2, float b0, float b1,
                                             float b2, float c0, float c1, float c2, ClosestHit* h) {
  const double ax = a0, ay = a1, az = a2, bx = b0, by = b1, bz = b2, cx = c0, cy = c1, cz = c2;
  const double abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
  const double d1 = dot3d(abx, aby, abz, px - ax, py - ay, pz - az), d2 = dot3d(acx, acy, acz, px - ax, py - ay, pz - az);
  const double d3 = dot3d(abx, aby, abz, px - bx, py - by, pz - bz), d4 = dot3d(acx, acy, acz, px - bx, py - by, pz - bz);
  const double d5 = dot3d(abx, aby, abz, px - cx, py - cy, pz - cz), d6 = dot3d(acx, acy, acz, px - cx, py - cy, pz - cz);
  double u, v, w;  // the weights of A, B, C
  if (d1 <= 0.0 && d2 <= 0.0) {
    u = 1.0; v = 0.0; w = 0.0;  // vertex A
  } else if (d3 >= 0.0 && d4 <= d3) {
    u = 0.0; v = 1.0; w = 0.0;  // vertex B
  } else if (d6 >= 0.0 && d5 <= d6) {
    u = 0.0; v = 0.0; w = 1.0;  // vertex C
  } else {
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double g = d4 - d3, k = d5 - d6;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {  // edge AB
      v = d1 / (d1 - d3); u = 1.0 - v; w = 0.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {  // edge AC
      w = d2 / (d2 - d6); u = 1.0 - w; v = 0.0;
    } else if (va <= 0.0 && g >= 0.0 && k >= 0.0) {  // edge BC
      w = g / (g + k); v = 1.0 - w; u = 0.0;
    } else {  // the interior (and every NaN: no comparison above holds)
      const double s = (va + vb) + vc;
      v = vb / s; w = vc / s; u = (1.0 - v) - w;
    }
  }
  const double ex = px - ((u * ax + v * bx) + w * cx), ey = py - ((u * ay + v * by) + w * cy), ez = pz - ((u * az + v * bz) + w * cz);
  const double dd = (ex * ex + ey * ey) + ez * ez;
  if (dd < h->d2 || (dd == h->d2 && face < h->face)) {  // (false for a NaN; +inf never wins: no face is held at index -1)
    h->d2 = dd; h->b0 = u; h->b1 = v; h->b2 = w; h->face = face;
  }
}

__device__ __forceinline__ void closest_store(const ClosestHit& h, float max_dist, int64_t i, float* __restrict__ out_dist,
                                              int32_t* __restrict__ out_face, float* __restrict__ out_bary) {
  const float dist = (float) F2N_DSQRT_RN(h.d2);
  const bool hit = h.face >= 0 && !(dist > max_dist);
  out_dist[i] = hit ? dist : __builtin_huge_valf();
  out_face[i] = hit ? h.face : -1;
  out_bary[i * 3] = hit ? (float) h.b0 : 0.f;
  out_bary[i * 3 + 1] = hit ? (float) h.b1 : 0.f;
  out_bary[i * 3 + 2] = hit ? (float) h.b2 : 0.f;
}

// flag_index: a face names a vertex that is not there; flag_box: a finite vertex lies outside the grid box dilated by the guard
__global__ void __launch_bounds__(256) closest_check_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                            const int32_t* __restrict__ faces, int with_grid, ClusterGrid g,
                                                            int32_t* flag_index, int32_t* flag_box) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  int a, b, c;
  if (i < n_faces && !face_in_range(faces, i, n_verts, &a, &b, &c)) *flag_index = 1;  // (benign race: every writer stores 1)
  if (with_grid && i < n_verts && finite3(verts + i * 3)) {
    const float guard = ray_guard(g.cell);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float x = verts[i * 3 + k], hi = F2N_ADD_RN(g.lo[k], F2N_MUL_RN((float) g.dims[k], g.cell));
      if (!(x >= F2N_SUB_RN(g.lo[k], guard) && x <= F2N_ADD_RN(hi, guard))) *flag_box = 1;
    }
  }
}

__global__ void __launch_bounds__(F2N_RAYCAST_TILE) closest_brute_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                                        const int32_t* __restrict__ faces, int n_points,
                                                                        const float* __restrict__ points, float max_dist,
                                                                        float* __restrict__ out_dist, int32_t* __restrict__ out_face,
                                                                        float* __restrict__ out_bary) {
  __shared__ float tile[9][F2N_RAYCAST_TILE];
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n_points;
  const float p0 = points[(live ? i : 0) * 3], p1 = points[(live ? i : 0) * 3 + 1], p2 = points[(live ? i : 0) * 3 + 2];
  const float inf = __builtin_huge_valf();
  const bool ok = live && fabsf(p0) < inf && fabsf(p1) < inf && fabsf(p2) < inf;
  ClosestHit h = {__builtin_huge_val(), 0.0, 0.0, 0.0, -1};
  for (int base = 0; base < n_faces; base += F2N_RAYCAST_TILE) {
    const int mine = base + (int) threadIdx.x;
    int a, b, c;
    const bool there = mine < n_faces && face_in_range(faces, mine, n_verts, &a, &b, &c);
    const float nan = __builtin_nanf("");  // (a face that is not there never wins)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      tile[k][threadIdx.x] = there ? verts[(int64_t) a * 3 + k] : nan;
      tile[3 + k][threadIdx.x] = there ? verts[(int64_t) b * 3 + k] : nan;
      tile[6 + k][threadIdx.x] = there ? verts[(int64_t) c * 3 + k] : nan;
    }
    __syncthreads();
    const int n = min(F2N_RAYCAST_TILE, n_faces - base);
    if (ok)
      for (int j = 0; j < n; j++)
        closest_face((double) p0, (double) p1, (double) p2, base + j, tile[0][j], tile[1][j], tile[2][j], tile[3][j], tile[4][j], tile[5][j],
                     tile[6][j], tile[7][j], tile[8][j], &h);
    __syncthreads();
  }
  if (live) closest_store(h, max_dist, i, out_dist, out_face, out_bary);
}

// every face of cell c's list against the point
__device__ __forceinline__ void closest_cell(double px, double py, double pz, int c, int n_verts, int n_faces, const float* __restrict__ verts,
                                             const int32_t* __restrict__ faces, const int32_t* __restrict__ cell_start,
                                             const int32_t* __restrict__ cell_faces, ClosestHit* h) {
  const int e1 = cell_start[c + 1];
  for (int e = cell_start[c]; e < e1; e++) {
    const int f = cell_faces[e];
    int a, b, cc;
    if (f < 0 || f >= n_faces || !face_in_range(faces, f, n_verts, &a, &b, &cc)) continue;
    const float* pa = verts + (int64_t) a * 3;
    const float* pb = verts + (int64_t) b * 3;
    const float* pc = verts + (int64_t) cc * 3;
    closest_face(px, py, pz, f, pa[0], pa[1], pa[2], pb[0], pb[1], pb[2], pc[0], pc[1], pc[2], h);
  }
}

__global__ void __launch_bounds__(256) closest_grid_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                           const int32_t* __restrict__ faces, ClusterGrid g,
                                                           const int32_t* __restrict__ cell_start, const int32_t* __restrict__ cell_faces,
                                                           int n_points, const float* __restrict__ points, float max_dist,
                                                           float* __restrict__ out_dist, int32_t* __restrict__ out_face,
                                                           float* __restrict__ out_bary) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_points) return;
  const float p0 = points[i * 3], p1 = points[i * 3 + 1], p2 = points[i * 3 + 2];
  const float inf = __builtin_huge_valf();
  ClosestHit h = {__builtin_huge_val(), 0.0, 0.0, 0.0, -1};
  if (fabsf(p0) < inf && fabsf(p1) < inf && fabsf(p2) < inf) {
    const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
    const int cx = ray_cell(g.lo[0], g.cell, nx, p0), cy = ray_cell(g.lo[1], g.cell, ny, p1), cz = ray_cell(g.lo[2], g.cell, nz, p2);
    const double px = p0, py = p1, pz = p2;
    for (int r = 0;; r++) {
      const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
      const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1);
      for (int z = z0; z <= z1; z++)
        for (int y = y0; y <= y1; y++) {
          const int row = (z * ny + y) * nx;
          if (z == cz - r || z == cz + r || y == cy - r || y == cy + r) {  // a face of the shell: the whole row
            for (int x = x0; x <= x1; x++) closest_cell(px, py, pz, row + x, n_verts, n_faces, verts, faces, cell_start, cell_faces, &h);
          } else {  // (r >= 1 here) the row's two ends, where they are inside the grid
            if (cx - r >= 0) closest_cell(px, py, pz, row + cx - r, n_verts, n_faces, verts, faces, cell_start, cell_faces, &h);
            if (cx + r <= nx - 1) closest_cell(px, py, pz, row + cx + r, n_verts, n_faces, verts, faces, cell_start, cell_faces, &h);
          }
        }
      // the nearest open side of the box: no face beyond it is listed inside
      float lb = inf;
      bool open = false;
#define F2N_CLOSEST_SIDE(C, N, LO, P)                                                                          \
  if (C - r > 0) {                                                                                             \
    open = true;                                                                                               \
    lb = fminf(lb, F2N_SUB_RN(P, F2N_ADD_RN(LO, F2N_MUL_RN((float) (C - r), g.cell))));                          \
  }                                                                                                            \
  if (C + r < N - 1) {                                                                                         \
    open = true;                                                                                               \
    lb = fminf(lb, F2N_SUB_RN(F2N_ADD_RN(LO, F2N_MUL_RN((float) (C + r + 1), g.cell)), P));                      \
  }
      F2N_CLOSEST_SIDE(cx, nx, g.lo[0], p0)
      F2N_CLOSEST_SIDE(cy, ny, g.lo[1], p1)
      F2N_CLOSEST_SIDE(cz, nz, g.lo[2], p2)
#undef F2N_CLOSEST_SIDE
      if (!open) break;  // every cell has been tested
      if ((h.face >= 0 && (float) F2N_DSQRT_RN(h.d2) < lb) || lb > max_dist) break;
    }
  }
  closest_store(h, max_dist, i, out_dist, out_face, out_bary);
}

// |(B - A) x (C - A)| in fp64; 0 for a face that names a vertex that is not there or is not finite
__global__ void __launch_bounds__(256) face_weights_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                           const int32_t* __restrict__ faces, double quantum, double* __restrict__ area2,
                                                           long long* __restrict__ weights) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int a, b, c;
  double area = 0.0;
  if (face_in_range(faces, f, n_verts, &a, &b, &c)) {
    const float* pa = verts + (int64_t) a * 3;
    const float* pb = verts + (int64_t) b * 3;
    const float* pc = verts + (int64_t) c * 3;
    if (finite3(pa) && finite3(pb) && finite3(pc)) {
      const double px = (double) pb[0] - (double) pa[0], py = (double) pb[1] - (double) pa[1], pz = (double) pb[2] - (double) pa[2];
      const double qx = (double) pc[0] - (double) pa[0], qy = (double) pc[1] - (double) pa[1], qz = (double) pc[2] - (double) pa[2];
      const double nx = py * qz - pz * qy, ny = pz * qx - px * qz, nz = px * qy - py * qx;
      area = F2N_DSQRT_RN((nx * nx + ny * ny) + nz * nz);
    }
  }
  if (area2 != nullptr) area2[f] = area;
  if (weights != nullptr) weights[f] = (long long) floor(area / quantum);
}

__global__ void __launch_bounds__(256) sample_surface_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                             const int32_t* __restrict__ faces, const long long* __restrict__ cum,
                                                             int n_samples, uint32_t key_lo, uint32_t key_hi, float* __restrict__ out_points,
                                                             int32_t* __restrict__ out_face, float* __restrict__ out_bary) {
  const int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_samples) return;
  uint32_t x[4];
  f2n_philox4x32((uint32_t) j, 0u, 0u, 0u, key_lo, key_hi, x);
  const double two32 = 1.0 / 4294967296.0;
  const long long T = cum[n_faces - 1];
  const double at = ((double) j + ((double) x[0] + 0.5) * two32) / (double) n_samples * (double) T;
  long long target = (long long) floor(at);
  if (target > T - 1) target = T - 1;
  int lo = 0, hi = n_faces - 1;  // the first face with cum > target (cum[F - 1] = T > target: there is one)
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (cum[mid] > target) hi = mid; else lo = mid + 1;
  }
  const double s = F2N_DSQRT_RN(((double) x[1] + 0.5) * two32), r = ((double) x[2] + 0.5) * two32;
  const float b0 = (float) (1.0 - s), b1 = (float) (s * (1.0 - r)), b2 = (float) (s * r);
  int a, b, c;
  const bool ok = face_in_range(faces, lo, n_verts, &a, &b, &c);  // (a face with a weight is in range: its area is not 0)
  out_face[j] = lo;
  out_bary[j * 3] = b0; out_bary[j * 3 + 1] = b1; out_bary[j * 3 + 2] = b2;
#pragma unroll
  for (int k = 0; k < 3; k++)
    out_points[j * 3 + k] = ok ? F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(b0, verts[(int64_t) a * 3 + k]), F2N_MUL_RN(b1, verts[(int64_t) b * 3 + k])),
                                            F2N_MUL_RN(b2, verts[(int64_t) c * 3 + k]))
                               : 0.f;
}

}  // namespace

int f2n_mesh_closest_point(void* stream, int n_verts, int n_faces, const float* verts, const int32_t* faces, const float* lo, float cell,
                           const int32_t* dims, const int32_t* cell_start, const int32_t* cell_faces, int n_points, const float* points,
                           float max_dist, float* out_dist, int32_t* out_face, float* out_bary) {
  ClusterGrid g = {};
  if (n_verts < 0 || n_faces < 0 || n_points < 0 || !(max_dist >= 0.f) || (cell_start != nullptr && !raycast_grid_ok(lo, cell, dims, &g)) ||
      (n_faces > 0 && (n_verts == 0 || verts == nullptr || faces == nullptr)) ||
      (n_points > 0 && (points == nullptr || out_dist == nullptr || out_face == nullptr || out_bary == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (cell_start != nullptr)  // the part of the walk's domain that is host data: the box within 2^15 cells of the origin of the frame
    for (int k = 0; k < 3; k++)
      if (!(fmaxf(fabsf(lo[k]), fabsf(lo[k] + (float) dims[k] * cell)) <= F2N_RAYCAST_DOMAIN_CELLS * cell)) return F2N_ERR_UNSUPPORTED;
  if (n_points == 0) return F2N_OK;
  hipStream_t st = (hipStream_t) stream;
  const bool with_grid = cell_start != nullptr && n_faces > 0;
  if (n_faces > 0) {  // the index check and the vertices' part of the domain, with out_face[0] and out_dist[0] as their flag words
    int32_t* flag_box = (int32_t*) out_dist;
    if (hipMemsetAsync(out_face, 0, sizeof(int32_t), st) != hipSuccess || hipMemsetAsync(flag_box, 0, sizeof(int32_t), st) != hipSuccess)
      return f2n_launch_status();
    hipLaunchKernelGGL(closest_check_kernel, dim3(f2n_div_up(n_faces > n_verts ? n_faces : n_verts, 256)), dim3(256), 0, st, n_verts, n_faces,
                       verts, faces, with_grid ? 1 : 0, g, out_face, flag_box);
    int32_t bad = 0, outside = 0;
    if (hipMemcpyAsync(&bad, out_face, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&outside, flag_box, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return f2n_launch_status();
    if (bad != 0) return F2N_ERR_INVALID_ARG;
    if (outside != 0) return F2N_ERR_UNSUPPORTED;
  }
  const dim3 grid(f2n_div_up(n_points, 256)), block(256);
  if (!with_grid)
    hipLaunchKernelGGL(closest_brute_kernel, grid, block, 0, st, n_verts, n_faces, verts, faces, n_points, points, max_dist, out_dist, out_face,
                       out_bary);
  else  // (cell_faces may be NULL when every list is empty: it is then never read)
    hipLaunchKernelGGL(closest_grid_kernel, grid, block, 0, st, n_verts, n_faces, verts, faces, g, cell_start, cell_faces, n_points, points,
                       max_dist, out_dist, out_face, out_bary);
  return f2n_launch_status();
}

int f2n_mesh_face_weights(void* stream, int n_verts, int n_faces, const float* verts, const int32_t* faces, double quantum, double* area2,
                          int64_t* weights) {
  if (n_verts < 0 || n_faces < 0 || (weights != nullptr && (!(quantum > 0.0) || !(quantum < __builtin_huge_val()))) ||
      (n_faces > 0 && (faces == nullptr || (n_verts > 0 && verts == nullptr) || (area2 == nullptr && weights == nullptr))))
    return F2N_ERR_INVALID_ARG;
  if (n_faces == 0) return F2N_OK;
  hipLaunchKernelGGL(face_weights_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, (hipStream_t) stream, n_verts, n_faces, verts, faces,
                     quantum, area2, (long long*) weights);
  return f2n_launch_status();
}

int f2n_mesh_sample_surface(void* stream, int n_verts, int n_faces, const float* verts, const int32_t* faces, const int64_t* cum,
                            int n_samples, uint64_t key, float* out_points, int32_t* out_face, float* out_bary) {
  if (n_verts < 0 || n_faces < 0 || n_samples < 0 ||
      (n_samples > 0 && (n_faces == 0 || n_verts == 0 || verts == nullptr || faces == nullptr || cum == nullptr || out_points == nullptr ||
                         out_face == nullptr || out_bary == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n_samples == 0) return F2N_OK;
  hipLaunchKernelGGL(sample_surface_kernel, dim3(f2n_div_up(n_samples, 256)), dim3(256), 0, (hipStream_t) stream, n_verts, n_faces, verts,
                     faces, (const long long*) cum, n_samples, (uint32_t) key, (uint32_t) (key >> 32), out_points, out_face, out_bary);
  return f2n_launch_status();
}

// =====================================================================================================================
// Texture atlas (include/f2n_abi.h, "Texture atlas of a triangle mesh"): one right-triangle chart per face in power-of-two
// blocks placed by the Morton decode of a prefix sum, the texel-to-surface map and a bilinear lookup.  One lane owns one
// face / texel / output value: no atomics, so every output is a function of the inputs alone.  The corner rotation is
// done with selects (sel3): a private array under a runtime index would live in scratch memory.
// =====================================================================================================================
namespace {

#define F2N_ATLAS_MAX_LOG 13      // blocks and the atlas itself are at most 8192 texels wide
#define F2N_ATLAS_DEGENERATE 4    // bit 2 of rot

__device__ __forceinline__ int morton_even_bits(long long m) {  // bits 0, 2, 4, ... of m, compacted (13 of them)
  int x = 0;
#pragma unroll
  for (int k = 0; k < F2N_ATLAS_MAX_LOG; k++) x |= (int) ((m >> (2 * k)) & 1) << k;
  return x;
}

__device__ __forceinline__ long long morton_encode(int x, int y) {
  long long m = 0;
#pragma unroll
  for (int k = 0; k < F2N_ATLAS_MAX_LOG; k++) m |= ((long long) ((x >> k) & 1) << (2 * k)) | ((long long) ((y >> k) & 1) << (2 * k + 1));
  return m;
}

__global__ void __launch_bounds__(256) atlas_classify_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                            const int32_t* __restrict__ faces, float density, int max_log,
                                                            int32_t* __restrict__ log_s, int32_t* __restrict__ rot) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int a, b, c, ls = 2, r = F2N_ATLAS_DEGENERATE;
  if (face_in_range(faces, f, n_verts, &a, &b, &c)) {
    const float* pa = verts + (int64_t) a * 3;
    const float* pb = verts + (int64_t) b * 3;
    const float* pc = verts + (int64_t) c * 3;
    if (finite3(pa) && finite3(pb) && finite3(pc)) {
      const double px = (double) pb[0] - (double) pa[0], py = (double) pb[1] - (double) pa[1], pz = (double) pb[2] - (double) pa[2];
      const double qx = (double) pc[0] - (double) pa[0], qy = (double) pc[1] - (double) pa[1], qz = (double) pc[2] - (double) pa[2];
      const double ex = (double) pc[0] - (double) pb[0], ey = (double) pc[1] - (double) pb[1], ez = (double) pc[2] - (double) pb[2];
      const double l_ab = (px * px + py * py) + pz * pz, l_bc = (ex * ex + ey * ey) + ez * ez, l_ca = (qx * qx + qy * qy) + qz * qz;
      const double nx = py * qz - pz * qy, ny = pz * qx - px * qz, nz = px * qy - py * qx;
      const double n2 = (nx * nx + ny * ny) + nz * nz;
      if (n2 > 0.0) {
        const double need = fmax(4.0, ceil(sqrt(sqrt(n2)) * (double) density) + 3.0);
        while (ls < max_log && (double) (1 << ls) < need) ls++;
        // the corner opposite the longest edge: corner 0 faces BC, corner 1 faces CA, corner 2 faces AB; the first among equals
        r = 0;
        double longest = l_bc;
        if (l_ca > longest) { r = 1; longest = l_ca; }
        if (l_ab > longest) r = 2;
      }
    }
  }
  log_s[f] = ls;
  rot[f] = r;
}

__global__ void __launch_bounds__(256) atlas_place_kernel(int n_faces, int n_blocks, int size, const int32_t* __restrict__ log_s,
                                                         const int32_t* __restrict__ rot, const int32_t* __restrict__ slot,
                                                         const long long* __restrict__ offsets, float* __restrict__ uv) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  const int sl = slot[f], ls = log_s[f];
  float o[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // (only constant indices below: registers)
  if (sl >= 0 && (sl >> 1) < n_blocks && ls >= 2 && ls <= F2N_ATLAS_MAX_LOG) {
    const long long off = offsets[sl >> 1];
    const float x0 = (float) morton_even_bits(off), y0 = (float) morton_even_bits(off >> 1), s = (float) (1 << ls), S = (float) size;
    const bool up = (sl & 1) != 0;
    // chart corners 0 (the right angle), 1 (along x), 2 (along y) in texels from the block's origin: every sum below is exact
    const float c0x = up ? s - 0.5f : 0.5f, c0y = c0x;
    const float c1x = up ? 2.5f : s - 2.5f, c1y = c0y;
    const float c2x = c0x, c2y = up ? 2.5f : s - 2.5f;
    const int r = rot[f] & 3;  // chart corner k is the face's corner (r + k) % 3: the face's corner j is chart corner (j - r) mod 3
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int k = (j - r + 3) % 3;
      o[2 * j] = F2N_DIV_RN(x0 + sel3(k, c0x, c1x, c2x), S);
      o[2 * j + 1] = F2N_DIV_RN(y0 + sel3(k, c0y, c1y, c2y), S);
    }
  }
#pragma unroll
  for (int k = 0; k < 6; k++) uv[f * 6 + k] = o[k];
}

// One wave owns an 8 x 8 texel tile (a block of four waves a 16 x 16 one): a tile lies inside one block of the atlas unless that
// block is a 4 x 4 one, so the wave's binary search takes one path and its loads are broadcasts.
__global__ void __launch_bounds__(256) atlas_texels_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                          const int32_t* __restrict__ faces, int n_blocks, int size,
                                                          const long long* __restrict__ offsets, const int32_t* __restrict__ block_log,
                                                          const int32_t* __restrict__ block_faces, const int32_t* __restrict__ rot,
                                                          int clamp, int row_begin, int row_end, int32_t* __restrict__ tex_face,
                                                          float* __restrict__ tex_bary, float* __restrict__ tex_pos) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int x = (int) blockIdx.x * 16 + (w & 1) * 8 + (l & 7);
  const int y = row_begin + (int) blockIdx.y * 16 + (w >> 1) * 8 + (l >> 3);
  if (x >= size || y >= row_end) return;
  const long long m = morton_encode(x, y);
  int face = -1;
  float b0 = 0.f, b1 = 0.f, b2 = 0.f, p0 = 0.f, p1 = 0.f, p2 = 0.f;
  if (m < offsets[n_blocks]) {
    int lo = 0, hi = n_blocks;  // the last block whose offset is <= m: offsets[lo] <= m < offsets[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (offsets[mid] <= m) lo = mid; else hi = mid;
    }
    const long long off = offsets[lo];
    const int ls = block_log[lo], s = 1 << ls;
    const int i = x - morton_even_bits(off), j = y - morton_even_bits(off >> 1);
    const bool up = i + j > s - 1;
    const int f = block_faces[lo * 2 + (up ? 1 : 0)];
    int a, b, c;
    if (f >= 0 && f < n_faces && (rot[f] & F2N_ATLAS_DEGENERATE) == 0 && i >= 0 && j >= 0 && i < s && j < s &&
        face_in_range(faces, f, n_verts, &a, &b, &c)) {
      const float leg = (float) (s - 3);
      const float u = F2N_DIV_RN((float) (up ? s - 1 - i : i), leg), v = F2N_DIV_RN((float) (up ? s - 1 - j : j), leg);
      const float w0 = F2N_SUB_RN(F2N_SUB_RN(1.f, u), v);
      const int r = rot[f] & 3;  // the face's corner j carries the weight of chart corner (j - r) mod 3
      b0 = sel3((3 - r) % 3, w0, u, v);
      b1 = sel3((4 - r) % 3, w0, u, v);
      b2 = sel3((5 - r) % 3, w0, u, v);
      if (clamp != 0 && (b0 < 0.f || b1 < 0.f || b2 < 0.f)) {
        b0 = fmaxf(b0, 0.f); b1 = fmaxf(b1, 0.f); b2 = fmaxf(b2, 0.f);
        const float sum = F2N_ADD_RN(F2N_ADD_RN(b0, b1), b2);
        b0 = F2N_DIV_RN(b0, sum); b1 = F2N_DIV_RN(b1, sum); b2 = F2N_DIV_RN(b2, sum);
      }
      const float* pa = verts + (int64_t) a * 3;
      const float* pb = verts + (int64_t) b * 3;
      const float* pc = verts + (int64_t) c * 3;
      p0 = F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(b0, pa[0]), F2N_MUL_RN(b1, pb[0])), F2N_MUL_RN(b2, pc[0]));
      p1 = F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(b0, pa[1]), F2N_MUL_RN(b1, pb[1])), F2N_MUL_RN(b2, pc[1]));
      p2 = F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(b0, pa[2]), F2N_MUL_RN(b1, pb[2])), F2N_MUL_RN(b2, pc[2]));
      face = f;
    }
  }
  const int64_t at = (int64_t) y * size + x;
  tex_face[at] = face;
  tex_bary[at * 3] = b0; tex_bary[at * 3 + 1] = b1; tex_bary[at * 3 + 2] = b2;
  tex_pos[at * 3] = p0; tex_pos[at * 3 + 1] = p1; tex_pos[at * 3 + 2] = p2;
}

__global__ void __launch_bounds__(256) texture_sample_kernel(int size, int channels, const float* __restrict__ tex, int64_t n,
                                                            const float* __restrict__ uv, float* __restrict__ out) {
  const int64_t at = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= n * channels) return;
  const int64_t row = at / channels;
  const int ch = (int) (at - row * channels);
  const float u = uv[row * 2], v = uv[row * 2 + 1], inf = __builtin_huge_valf();
  float r = 0.f;
  if (fabsf(u) < inf && fabsf(v) < inf) {
    const float top = (float) (size - 1), S = (float) size;
    const float fx = fminf(fmaxf(F2N_SUB_RN(F2N_MUL_RN(u, S), 0.5f), 0.f), top);
    const float fy = fminf(fmaxf(F2N_SUB_RN(F2N_MUL_RN(v, S), 0.5f), 0.f), top);
    const float gx = floorf(fx), gy = floorf(fy);
    const float ax = F2N_SUB_RN(fx, gx), ay = F2N_SUB_RN(fy, gy), cx = F2N_SUB_RN(1.f, ax), cy = F2N_SUB_RN(1.f, ay);
    const int x0 = (int) gx, y0 = (int) gy, x1 = min(x0 + 1, size - 1), y1 = min(y0 + 1, size - 1);
    const float t00 = tex[((int64_t) y0 * size + x0) * channels + ch], t10 = tex[((int64_t) y0 * size + x1) * channels + ch];
    const float t01 = tex[((int64_t) y1 * size + x0) * channels + ch], t11 = tex[((int64_t) y1 * size + x1) * channels + ch];
    r = F2N_ADD_RN(F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(t00, F2N_MUL_RN(cx, cy)), F2N_MUL_RN(t10, F2N_MUL_RN(ax, cy))),
                              F2N_MUL_RN(t01, F2N_MUL_RN(cx, ay))),
                   F2N_MUL_RN(t11, F2N_MUL_RN(ax, ay)));
  }
  out[at] = r;
}

bool atlas_size_ok(int size) { return size >= 4 && size <= (1 << F2N_ATLAS_MAX_LOG) && (size & (size - 1)) == 0; }

}  // namespace

int f2n_atlas_classify(void* stream, int n_verts, int n_faces, const float* verts, const int32_t* faces, float density, int max_log,
                       int32_t* log_s, int32_t* rot) {
  if (n_verts < 0 || n_faces < 0 || !(density > 0.f) || !(density < __builtin_huge_valf()) || max_log < 2 || max_log > F2N_ATLAS_MAX_LOG ||
      (n_faces > 0 && (faces == nullptr || log_s == nullptr || rot == nullptr || (n_verts > 0 && verts == nullptr))))
    return F2N_ERR_INVALID_ARG;
  if (n_faces == 0) return F2N_OK;
  hipLaunchKernelGGL(atlas_classify_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, (hipStream_t) stream, n_verts, n_faces, verts, faces,
                     density, max_log, log_s, rot);
  return f2n_launch_status();
}

int f2n_atlas_place(void* stream, int n_faces, int n_blocks, int size, const int32_t* log_s, const int32_t* rot, const int32_t* slot,
                    const int64_t* offsets, float* uv) {
  if (n_faces < 0 || n_blocks < 0 || !atlas_size_ok(size) ||
      (n_faces > 0 && (log_s == nullptr || rot == nullptr || slot == nullptr || offsets == nullptr || uv == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n_faces == 0) return F2N_OK;
  hipLaunchKernelGGL(atlas_place_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, (hipStream_t) stream, n_faces, n_blocks, size, log_s, rot,
                     slot, (const long long*) offsets, uv);
  return f2n_launch_status();
}

int f2n_atlas_texels(void* stream, int n_verts, int n_faces, const float* verts, const int32_t* faces, int n_blocks, int size,
                     const int64_t* offsets, const int32_t* block_log, const int32_t* block_faces, const int32_t* rot, int clamp,
                     int row_begin, int row_end, int32_t* tex_face, float* tex_bary, float* tex_pos) {
  if (n_verts < 0 || n_faces < 0 || n_blocks < 0 || !atlas_size_ok(size) || row_begin < 0 || row_end < row_begin || row_end > size ||
      offsets == nullptr || tex_face == nullptr || tex_bary == nullptr || tex_pos == nullptr || (clamp != 0 && clamp != 1) ||
      (n_blocks > 0 && (block_log == nullptr || block_faces == nullptr)) ||
      (n_faces > 0 && (faces == nullptr || rot == nullptr || (n_verts > 0 && verts == nullptr))))
    return F2N_ERR_INVALID_ARG;
  if (row_end == row_begin) return F2N_OK;
  hipLaunchKernelGGL(atlas_texels_kernel, dim3(f2n_div_up(size, 16), f2n_div_up(row_end - row_begin, 16)), dim3(256), 0, (hipStream_t) stream,
                     n_verts, n_faces, verts, faces, n_blocks, size, (const long long*) offsets, block_log, block_faces, rot, clamp, row_begin,
                     row_end, tex_face, tex_bary, tex_pos);
  return f2n_launch_status();
}

int f2n_texture_sample(void* stream, int size, int channels, const float* tex, int64_t n, const float* uv, float* out) {
  if (size < 1 || size > 32768 || channels < 1 || channels > 64 || n < 0 || n > (int64_t) 1 << 40 ||
      (n > 0 && (tex == nullptr || uv == nullptr || out == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  const int64_t blocks = (n * channels + 255) / 256;
  if (blocks > 0x7fffffffLL) return F2N_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(texture_sample_kernel, dim3((unsigned) blocks), dim3(256), 0, (hipStream_t) stream, size, channels, tex, n, uv, out);
  return f2n_launch_status();
}

// =====================================================================================================================
// Mesh refinement (include/f2n_abi.h, "Mesh refinement"): the vertex one-ring as a CSR built from sorted directed-edge
// keys (the sort is the caller's), the Taubin smoothing pass, the trust-region clamp, the per-iteration update of the
// projection onto a level set of ln(sigma), and the face quality.  One lane owns one face / vertex / point; the only
// atomics are the two integer edge counts.  No transcendental function: + - * / sqrt, one rounding each.
// =====================================================================================================================
namespace {

__global__ void __launch_bounds__(256) ring_keys_kernel(int n_verts, int n_faces, const int32_t* __restrict__ faces,
                                                       long long* __restrict__ keys) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int a, b, c;
  const bool ok = face_in_range(faces, f, n_verts, &a, &b, &c) && a != b && b != c && a != c;
  const long long V = n_verts;
  long long* k = keys + f * 6;
  k[0] = ok ? a * V + b : -1;
  k[1] = ok ? b * V + a : -1;
  k[2] = ok ? b * V + c : -1;
  k[3] = ok ? c * V + b : -1;
  k[4] = ok ? c * V + a : -1;
  k[5] = ok ? a * V + c : -1;
}

// the first index in [0, n) whose key is >= want
__device__ __forceinline__ int ring_lower_bound(const long long* __restrict__ keys, int n, long long want) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) ring_fill_kernel(int n_verts, int n_edges, const long long* __restrict__ edge_keys,
                                                       const long long* __restrict__ edge_uses, int32_t* __restrict__ start_end,
                                                       int32_t* __restrict__ ring, uint8_t* __restrict__ pinned, int32_t* edge_counts) {
  const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_verts) return;
  const long long V = n_verts;
  const int s = ring_lower_bound(edge_keys, n_edges, v * V), e = ring_lower_bound(edge_keys, n_edges, (v + 1) * V);
  start_end[v * 2] = s;
  start_end[v * 2 + 1] = e;
  bool pin = s == e;
  int boundary = 0, nonmanifold = 0;
  for (int j = s; j < e; j++) {
    const int w = (int) (edge_keys[j] - v * V);
    const long long uses = edge_uses[j];
    ring[j] = w;
    pin = pin || uses != 2;
    if (w > v) {  // (an undirected edge is counted at its lower end)
      boundary += uses == 1 ? 1 : 0;
      nonmanifold += uses >= 3 ? 1 : 0;
    }
  }
  pinned[v] = pin ? 1 : 0;
  if (boundary != 0) atomicAdd(edge_counts, boundary);
  if (nonmanifold != 0) atomicAdd(edge_counts + 1, nonmanifold);
}

__global__ void __launch_bounds__(256) mesh_smooth_kernel(int n_verts, int n_ring, const float* __restrict__ verts,
                                                         const int32_t* __restrict__ start_end, const int32_t* __restrict__ ring,
                                                         const uint8_t* __restrict__ pinned, double factor, float* __restrict__ out) {
  const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_verts) return;
  const float* p = verts + v * 3;
  const int s = start_end[v * 2], e = start_end[v * 2 + 1];
  bool move = pinned[v] == 0 && s >= 0 && s < e && e <= n_ring && finite3(p);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int j = s; move && j < e; j++) {
    const int w = ring[j];
    if (w < 0 || w >= n_verts || !finite3(verts + (int64_t) w * 3)) {
      move = false;
      break;
    }
    const float* q = verts + (int64_t) w * 3;
    sx = sx + (double) q[0];
    sy = sy + (double) q[1];
    sz = sz + (double) q[2];
  }
  if (!move) {
    out[v * 3] = p[0]; out[v * 3 + 1] = p[1]; out[v * 3 + 2] = p[2];
    return;
  }
  const double cnt = (double) (e - s);
  const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
  const double px = p[0], py = p[1], pz = p[2];
  const double dx = mx - px, dy = my - py, dz = mz - pz;
  const double tx = factor * dx, ty = factor * dy, tz = factor * dz;
  out[v * 3] = (float) (px + tx);
  out[v * 3 + 1] = (float) (py + ty);
  out[v * 3 + 2] = (float) (pz + tz);
}

// x [3] pulled back into the ball of radius r around p0 [3] (fp32): true if it moved
__device__ __forceinline__ bool move_clamp3(const float* p0, float r, float* x) {
  const float ux = F2N_SUB_RN(x[0], p0[0]), uy = F2N_SUB_RN(x[1], p0[1]), uz = F2N_SUB_RN(x[2], p0[2]);
  const float l = sqrtf(F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(ux, ux), F2N_MUL_RN(uy, uy)), F2N_MUL_RN(uz, uz)));
  if (!(l > r)) return false;  // (a NaN length leaves the point alone)
  float k = F2N_DIV_RN(r, l);
  for (int round = 0; round < F2N_MOVE_CLAMP_ROUNDS; round++) {
    x[0] = F2N_ADD_RN(p0[0], F2N_MUL_RN(ux, k));
    x[1] = F2N_ADD_RN(p0[1], F2N_MUL_RN(uy, k));
    x[2] = F2N_ADD_RN(p0[2], F2N_MUL_RN(uz, k));
    // the three sums round to the coordinates' own grid, which can leave the point just outside: measured again, pulled in again
    const float wx = F2N_SUB_RN(x[0], p0[0]), wy = F2N_SUB_RN(x[1], p0[1]), wz = F2N_SUB_RN(x[2], p0[2]);
    const float lw = sqrtf(F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(wx, wx), F2N_MUL_RN(wy, wy)), F2N_MUL_RN(wz, wz)));
    if (!(lw > r)) break;
    k = F2N_MUL_RN(F2N_MUL_RN(k, F2N_DIV_RN(r, lw)), 0x1.fffffp-1f);
  }
  return true;
}

__global__ void __launch_bounds__(256) move_clamp_kernel(int n, const float* __restrict__ p0, float max_move, float* __restrict__ pts) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x[3] = {pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]};
  if (move_clamp3(p0 + i * 3, max_move, x)) {
    pts[i * 3] = x[0]; pts[i * 3 + 1] = x[1]; pts[i * 3 + 2] = x[2];
  }
}

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) < __builtin_huge_valf(); }

__global__ void __launch_bounds__(256) level_step_kernel(int n, int first, int propose, const float* __restrict__ p0,
                                                        const float* __restrict__ sigma, const float* __restrict__ grad,
                                                        const float* __restrict__ h, float tol, float max_step, float max_move,
                                                        float* __restrict__ cand, float* __restrict__ best, float* __restrict__ h_best,
                                                        float* __restrict__ g_best, float* __restrict__ scale, int32_t* __restrict__ status,
                                                        int32_t* __restrict__ evals) {
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int st = first ? 0 : status[i];
  if (st & (F2N_LEVEL_EMPTY | F2N_LEVEL_CONVERGED)) {  // a finished point proposes its own position
    cand[i * 3] = best[i * 3]; cand[i * 3 + 1] = best[i * 3 + 1]; cand[i * 3 + 2] = best[i * 3 + 2];
    return;
  }
  const float c[3] = {cand[i * 3], cand[i * 3 + 1], cand[i * 3 + 2]};
  const float s = sigma[i], hc = h[i];
  const float g[3] = {F2N_DIV_RN(grad[i * 3], s), F2N_DIV_RN(grad[i * 3 + 1], s), F2N_DIV_RN(grad[i * 3 + 2], s)};
  const float q = F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(g[0], g[0]), F2N_MUL_RN(g[1], g[1])), F2N_MUL_RN(g[2], g[2]));
  const bool evaluable = s > 0.f && finite1(s) && finite1(hc) && finite3(g) && q != 0.f;
  float b[3], gb[3], hb, a;
  if (first) {
    evals[i] = 1;
    b[0] = c[0]; b[1] = c[1]; b[2] = c[2];
    hb = hc;
    a = 1.f;
    gb[0] = evaluable ? g[0] : 0.f; gb[1] = evaluable ? g[1] : 0.f; gb[2] = evaluable ? g[2] : 0.f;
    if (!evaluable) st = F2N_LEVEL_EMPTY;
  } else {
    evals[i] = evals[i] + 1;
    hb = h_best[i];
    a = scale[i];
    const bool accept = evaluable && fabsf(hc) <= fabsf(hb);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      b[k] = accept ? c[k] : best[i * 3 + k];
      gb[k] = accept ? g[k] : g_best[i * 3 + k];
    }
    if (accept) hb = hc; else a = F2N_MUL_RN(a, 0.5f);
  }
  if (!(st & F2N_LEVEL_EMPTY) && fabsf(hb) <= tol) st |= F2N_LEVEL_CONVERGED;
  float next[3] = {b[0], b[1], b[2]};
  if (propose && !(st & (F2N_LEVEL_EMPTY | F2N_LEVEL_CONVERGED))) {
    const float qb = F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(gb[0], gb[0]), F2N_MUL_RN(gb[1], gb[1])), F2N_MUL_RN(gb[2], gb[2]));
    const float t = -F2N_DIV_RN(F2N_MUL_RN(a, hb), qb);
    float d[3] = {F2N_MUL_RN(t, gb[0]), F2N_MUL_RN(t, gb[1]), F2N_MUL_RN(t, gb[2])};
    const float l = sqrtf(F2N_ADD_RN(F2N_ADD_RN(F2N_MUL_RN(d[0], d[0]), F2N_MUL_RN(d[1], d[1])), F2N_MUL_RN(d[2], d[2])));
    if (l > max_step) {
      const float k = F2N_DIV_RN(max_step, l);
      d[0] = F2N_MUL_RN(d[0], k); d[1] = F2N_MUL_RN(d[1], k); d[2] = F2N_MUL_RN(d[2], k);
      st |= F2N_LEVEL_STEP_CLAMPED;
    }
    next[0] = F2N_ADD_RN(b[0], d[0]); next[1] = F2N_ADD_RN(b[1], d[1]); next[2] = F2N_ADD_RN(b[2], d[2]);
    if (move_clamp3(p0 + i * 3, max_move, next)) st |= F2N_LEVEL_MOVE_CLAMPED;
    if (!finite3(next)) { next[0] = b[0]; next[1] = b[1]; next[2] = b[2]; }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    cand[i * 3 + k] = next[k];
    best[i * 3 + k] = b[k];
    g_best[i * 3 + k] = gb[k];
  }
  h_best[i] = hb;
  scale[i] = a;
  status[i] = st;
}

__global__ void __launch_bounds__(256) face_quality_kernel(int n_verts, int n_faces, const float* __restrict__ verts,
                                                          const int32_t* __restrict__ faces, double* __restrict__ out) {
  const int64_t f = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int a, b, c;
  double q = 0.0;
  if (face_in_range(faces, f, n_verts, &a, &b, &c) && a != b && b != c && a != c) {
    const float* pa = verts + (int64_t) a * 3;
    const float* pb = verts + (int64_t) b * 3;
    const float* pc = verts + (int64_t) c * 3;
    if (finite3(pa) && finite3(pb) && finite3(pc)) {
      const double px = (double) pb[0] - (double) pa[0], py = (double) pb[1] - (double) pa[1], pz = (double) pb[2] - (double) pa[2];
      const double qx = (double) pc[0] - (double) pa[0], qy = (double) pc[1] - (double) pa[1], qz = (double) pc[2] - (double) pa[2];
      const double rx = (double) pc[0] - (double) pb[0], ry = (double) pc[1] - (double) pb[1], rz = (double) pc[2] - (double) pb[2];
      const double nx = py * qz - pz * qy, ny = pz * qx - px * qz, nz = px * qy - py * qx;
      const double area2 = F2N_DSQRT_RN((nx * nx + ny * ny) + nz * nz);
      const double l1 = (px * px + py * py) + pz * pz, l2 = (qx * qx + qy * qy) + qz * qz, l3 = (rx * rx + ry * ry) + rz * rz;
      const double L = (l1 + l2) + l3;
      q = L > 0.0 ? (F2N_FACE_QUALITY_K * area2) / L : 0.0;
    } else {
      q = __builtin_nan("");
    }
  }
  out[f] = q;
}

}  // namespace

int f2n_mesh_ring_keys(void* stream, int n_verts, int n_faces, const int32_t* faces, int64_t* keys) {
  if (n_verts < 0 || n_faces < 0 || n_faces > 0x7fffffff / 6 || (n_faces > 0 && (faces == nullptr || keys == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n_faces == 0) return F2N_OK;
  hipLaunchKernelGGL(ring_keys_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, (hipStream_t) stream, n_verts, n_faces, faces,
                     (long long*) keys);
  return f2n_launch_status();
}

int f2n_mesh_ring_fill(void* stream, int n_verts, int n_edges, const int64_t* edge_keys, const int64_t* edge_uses, int32_t* ring_start_end,
                       int32_t* ring, uint8_t* pinned, int32_t* edge_counts) {
  if (n_verts < 0 || n_edges < 0 || edge_counts == nullptr || (n_verts > 0 && (ring_start_end == nullptr || pinned == nullptr)) ||
      (n_edges > 0 && (n_verts == 0 || edge_keys == nullptr || edge_uses == nullptr || ring == nullptr)))
    return F2N_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t) stream;
  if (hipMemsetAsync(edge_counts, 0, 2 * sizeof(int32_t), st) != hipSuccess) return f2n_launch_status();
  if (n_verts == 0) return F2N_OK;
  hipLaunchKernelGGL(ring_fill_kernel, dim3(f2n_div_up(n_verts, 256)), dim3(256), 0, st, n_verts, n_edges, (const long long*) edge_keys,
                     (const long long*) edge_uses, ring_start_end, ring, pinned, edge_counts);
  return f2n_launch_status();
}

int f2n_mesh_smooth(void* stream, int n_verts, int n_ring, const float* verts, const int32_t* ring_start_end, const int32_t* ring,
                    const uint8_t* pinned, double factor, float* out_verts) {
  if (n_verts < 0 || n_ring < 0 || !(fabs(factor) < __builtin_huge_val()) ||
      (n_verts > 0 && (verts == nullptr || ring_start_end == nullptr || pinned == nullptr || out_verts == nullptr || out_verts == verts)) ||
      (n_ring > 0 && ring == nullptr))
    return F2N_ERR_INVALID_ARG;
  if (n_verts == 0) return F2N_OK;
  hipLaunchKernelGGL(mesh_smooth_kernel, dim3(f2n_div_up(n_verts, 256)), dim3(256), 0, (hipStream_t) stream, n_verts, n_ring, verts,
                     ring_start_end, ring, pinned, factor, out_verts);
  return f2n_launch_status();
}

int f2n_mesh_move_clamp(void* stream, int n, const float* p0, float max_move, float* pts) {
  if (n < 0 || !(max_move > 0.f) || (n > 0 && (p0 == nullptr || pts == nullptr))) return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  hipLaunchKernelGGL(move_clamp_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, p0, max_move, pts);
  return f2n_launch_status();
}

int f2n_level_step(void* stream, int n, int first, int propose, const float* p0, const float* sigma, const float* grad, const float* h,
                   float tol, float max_step, float max_move, float* cand, float* best, float* h_best, float* g_best, float* scale,
                   int32_t* status, int32_t* evals) {
  if (n < 0 || !(tol >= 0.f) || !(max_step > 0.f) || !(max_move > 0.f) ||
      (n > 0 && (p0 == nullptr || sigma == nullptr || grad == nullptr || h == nullptr || cand == nullptr || best == nullptr ||
                 h_best == nullptr || g_best == nullptr || scale == nullptr || status == nullptr || evals == nullptr)))
    return F2N_ERR_INVALID_ARG;
  if (n == 0) return F2N_OK;
  hipLaunchKernelGGL(level_step_kernel, dim3(f2n_div_up(n, 256)), dim3(256), 0, (hipStream_t) stream, n, first ? 1 : 0, propose ? 1 : 0, p0,
                     sigma, grad, h, tol, max_step, max_move, cand, best, h_best, g_best, scale, status, evals);
  return f2n_launch_status();
}

int f2n_mesh_face_quality(void* stream, int n_verts, int n_faces, const float* verts, const int32_t* faces, double* quality) {
  if (n_verts < 0 || n_faces < 0 || (n_faces > 0 && (faces == nullptr || quality == nullptr || (n_verts > 0 && verts == nullptr))))
    return F2N_ERR_INVALID_ARG;
  if (n_faces == 0) return F2N_OK;
  hipLaunchKernelGGL(face_quality_kernel, dim3(f2n_div_up(n_faces, 256)), dim3(256), 0, (hipStream_t) stream, n_verts, n_faces, verts, faces,
                     quality);
  return f2n_launch_status();
}
