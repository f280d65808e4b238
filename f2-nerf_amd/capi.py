"""ctypes binding of libf2n_hip.so (include/f2n_abi.h) for torch tensors on a HIP device.

Thin by design: every function checks dtype/contiguity/device, passes raw device pointers and the current
torch HIP stream, and raises on a non-zero status.  No computation happens here and nothing falls back to
torch ops or to the CPU oracle."""
import ctypes
import os

import torch

from . import build

_lib = None
ABI_VERSION = 13  # include/f2n_abi.h


class F2nError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(build.LIB):
            raise F2nError("native library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % build.LIB)
        _lib = ctypes.CDLL(build.LIB)
        _lib.f2n_build_info.restype = ctypes.c_char_p
        if _lib.f2n_abi_version() != ABI_VERSION:  # a stale library next to a newer binding: argument lists would not match
            raise F2nError("%s reports ABI version %d, this binding is written for %d: rebuild (__graft_entry__.build())"
                           % (build.LIB, _lib.f2n_abi_version(), ABI_VERSION))
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_DT = {"f32": torch.float32, "i32": torch.int32, "i64": torch.int64, "u8": torch.uint8, "h16": torch.float16}


def _p(t, kind=None, allow_none=False):
    if t is None:
        if allow_none:
            return ctypes.c_void_p(0)
        raise F2nError("required tensor is None")
    if not t.is_cuda:
        raise F2nError("tensor must live on the HIP device (no CPU path)")
    if not t.is_contiguous():
        raise F2nError("tensor must be contiguous")
    if kind is not None and t.dtype != _DT[kind]:
        raise F2nError("expected dtype %s, got %s" % (kind, t.dtype))
    return ctypes.c_void_p(t.data_ptr())


def _ck(rc, name):
    if rc != 0:
        raise F2nError("%s failed with status %d" % (name, rc))


_i = ctypes.c_int
_f = ctypes.c_float
_d = ctypes.c_double  # (the Adam betas: doubles as in torch::optim::AdamOptions, include/f2n_abi.h)


def build_info():
    return lib().f2n_build_info().decode()


def debug_counters(reset=False):
    """Diagnostic event counters of the library (f2n_debug_counters): [0] = scatter records applied by the atomic fallback,
    [1] = table slices whose owner summed in fp64 instead of its packed fixed-point image (same bits, slower), [2] = (debug variant) the
    largest per-slice sum of |addend| as float bits, [3] = records that travelled through an overflow list (exact, order-free)."""
    out = (ctypes.c_int32 * 8)()
    torch.cuda.synchronize()
    _ck(lib().f2n_debug_counters(out, _i(1 if reset else 0)), "f2n_debug_counters")
    return [int(v) for v in out]


def set_scatter_producer(variant):
    """Which instantiation of the producer kernel the owner-binned hash-gradient scatter launches from now on, process-wide
    (f2n_set_scatter_producer): 1 = staged, hash constants in LDS (the default), 0 = non-staged.  Same gradient table either way."""
    _ck(lib().f2n_set_scatter_producer(_i(variant)), "f2n_set_scatter_producer")


def _debug_only(name):
    if not hasattr(lib(), name):
        raise RuntimeError("%s exists in the debug variant of the library only (include/f2n_debug.h): set F2N_DEBUG_BUILD=1 before "
                           "importing the package" % name)


def debug_pollute(value):
    """Garbage derived from `value` in 64 KB of LDS and ~100 vector registers of every CU, on the current stream (f2n_debug_pollute)."""
    _debug_only("f2n_debug_pollute")
    _ck(lib().f2n_debug_pollute(_stream(), ctypes.c_uint(int(value) & 0xFFFFFFFF)), "f2n_debug_pollute")


def debug_spin(microseconds):
    """One wave spinning for that long on the current stream (f2n_debug_spin)."""
    _debug_only("f2n_debug_spin")
    _ck(lib().f2n_debug_spin(_stream(), _i(microseconds)), "f2n_debug_spin")


# ---------------------------------------------------------------- sampler
def normalize_dirs(n, dirs, out):
    _ck(lib().f2n_normalize_dirs(_stream(), _i(n), _p(dirs, "f32"), _p(out, "f32")), "f2n_normalize_dirs")


def sampler_prologue(n, dirs, out, zero=None, u=None, fineness=0.0, noise_out=None):
    _ck(lib().f2n_sampler_prologue(_stream(), _i(n), _p(dirs, "f32"), _p(out, "f32"), _p(zero, "i32", True),
                                   _i(0 if zero is None else zero.numel()), _i(0 if u is None else u.numel()), _p(u, "f32", True),
                                   _f(fineness), _p(noise_out, "f32", True)), "f2n_sampler_prologue")


def sampler_prologue_keyed(n, dirs, out, zero, n_noise, key, seq, fineness, noise_out):
    """f2n_sampler_prologue with the march noise drawn by the launch (Philox4x32-10 keyed by (key, seq): include/f2n_abi.h)."""
    _ck(lib().f2n_sampler_prologue_keyed(_stream(), _i(n), _p(dirs, "f32"), _p(out, "f32"), _p(zero, "i32", True),
                                         _i(0 if zero is None else zero.numel()), _i(n_noise), ctypes.c_uint64(int(key) & (2 ** 64 - 1)),
                                         ctypes.c_uint64(int(seq) & (2 ** 64 - 1)), _f(fineness), _p(noise_out, "f32")), "f2n_sampler_prologue_keyed")


def edge_samples_ex(n, edge_pool, n_edges, transes, edge_idx, edge_coords, u01, out_pts, out_idx, idx_stride, out_pts2=None,
                    out_idx2=None, idx_stride2=1):
    _ck(lib().f2n_edge_samples_ex(_stream(), _i(n), _p(edge_pool, "u8"), _i(n_edges), _p(transes, "u8"), _p(edge_idx, "i32", True),
                                  _p(edge_coords, "f32", True), _p(u01, "f32", True), _p(out_pts, "f32"), _p(out_idx, "i32"),
                                  _i(idx_stride), _p(out_pts2, "f32", True), _p(out_idx2, "i32", True), _i(idx_stride2)),
        "f2n_edge_samples_ex")


def oct_intersect_count(n_rays, max_hits, search_order, rays_o, rays_d, near, far, tree_nodes, hit_counts, child_blocks=None):
    _ck(lib().f2n_oct_intersect_count(_stream(), _i(n_rays), _i(max_hits), _p(search_order, "u8"), _p(rays_o, "f32"),
                                      _p(rays_d, "f32"), _f(near), _f(far), _p(tree_nodes, "u8"), _p(hit_counts, "i32"),
                                      _p(child_blocks, "u8", True)), "f2n_oct_intersect_count")


def oct_intersect_strided(n_rays, max_hits, search_order, rays_o, rays_d, near, far, tree_nodes, oct_se, oct_idx, oct_nf, total,
                          oct_trans=None, child_blocks=None):
    _ck(lib().f2n_oct_intersect_strided(_stream(), _i(n_rays), _i(max_hits), _p(search_order, "u8"), _p(rays_o, "f32"),
                                        _p(rays_d, "f32"), _f(near), _f(far), _p(tree_nodes, "u8"), _p(oct_se, "i32"),
                                        _p(oct_idx, "i32"), _p(oct_nf, "f32"), _p(total, "i32"), _p(oct_trans, "i32", True),
                                        _p(child_blocks, "u8", True)), "f2n_oct_intersect_strided")


def oct_lds_max_interior():
    return int(lib().f2n_oct_lds_max_interior())


def oct_intersect_strided_lds(n_rays, max_hits, search_order, rays_o, rays_d, near, far, tree_nodes, oct_se, oct_idx, oct_nf, total,
                              oct_trans, child_blocks, interior_nodes, rank_of):
    """The walk of oct_intersect_strided out of LDS-resident child records (trees with few interior nodes)."""
    _ck(lib().f2n_oct_intersect_strided_lds(_stream(), _i(n_rays), _i(max_hits), _p(search_order, "u8"), _p(rays_o, "f32"),
                                            _p(rays_d, "f32"), _f(near), _f(far), _p(tree_nodes, "u8"), _p(oct_se, "i32"),
                                            _p(oct_idx, "i32"), _p(oct_nf, "f32"), _p(total, "i32"), _p(oct_trans, "i32", True),
                                            _p(child_blocks, "u8"), _p(interior_nodes, "i32"), _p(rank_of, "i32"),
                                            _i(int(interior_nodes.numel()))), "f2n_oct_intersect_strided_lds")


def segment_scan(n, counts, start_end, total):
    _ck(lib().f2n_segment_scan(_stream(), _i(n), _p(counts, "i32"), _p(start_end, "i32"), _p(total, "i32")),
        "f2n_segment_scan")


def _mapped(host_tensor):
    """Device address of a PINNED host int32 tensor (hipHostMalloc memory is mapped into the device's address space at the
    same address), or NULL."""
    if host_tensor is None:
        return ctypes.c_void_p(0)
    if host_tensor.is_cuda or not host_tensor.is_pinned() or host_tensor.dtype != _DT["i32"] or not host_tensor.is_contiguous():
        raise F2nError("mirror must be a contiguous pinned host int32 tensor")
    return ctypes.c_void_p(host_tensor.data_ptr())


def segment_scan_ex(n, counts, start_end, total, mirror=None, also=None):
    """mirror: pinned host int32 tensor of len(also) + 1 words that the scan kernel itself fills (read it after a sync)."""
    n_also = 0 if also is None else int(also.numel())
    _ck(lib().f2n_segment_scan_ex(_stream(), _i(n), _p(counts, "i32"), _p(start_end, "i32"), _p(total, "i32"), _mapped(mirror),
                                  _p(also, "i32", True), _i(n_also)), "f2n_segment_scan_ex")


def oct_intersect_fill(n_rays, search_order, rays_o, rays_d, near, far, tree_nodes, oct_se, oct_idx, oct_nf, child_blocks=None):
    _ck(lib().f2n_oct_intersect_fill(_stream(), _i(n_rays), _p(search_order, "u8"), _p(rays_o, "f32"), _p(rays_d, "f32"),
                                     _f(near), _f(far), _p(tree_nodes, "u8"), _p(oct_se, "i32"), _p(oct_idx, "i32"),
                                     _p(oct_nf, "f32"), _p(child_blocks, "u8", True)), "f2n_oct_intersect_fill")


def ray_march_count(n_rays, sample_l, scale_by_dis, rays_o, rays_d, noise, oct_se, oct_idx, oct_nf, tree_nodes, transes,
                    counts):
    _ck(lib().f2n_ray_march_count(_stream(), _i(n_rays), _f(sample_l), _i(int(scale_by_dis)), _p(rays_o, "f32"),
                                  _p(rays_d, "f32"), _p(noise, "f32"), _p(oct_se, "i32"), _p(oct_idx, "i32"),
                                  _p(oct_nf, "f32"), _p(tree_nodes, "u8"), _p(transes, "u8"), _p(counts, "i32")),
        "f2n_ray_march_count")


def ray_march_fill(n_rays, sample_l, scale_by_dis, rays_o, rays_d, noise, oct_se, oct_idx, oct_nf, tree_nodes, transes,
                   pts_se, pts, dirs, dt, t, anchors, first_oct_dis):
    _ck(lib().f2n_ray_march_fill(_stream(), _i(n_rays), _f(sample_l), _i(int(scale_by_dis)), _p(rays_o, "f32"),
                                 _p(rays_d, "f32"), _p(noise, "f32"), _p(oct_se, "i32"), _p(oct_idx, "i32"),
                                 _p(oct_nf, "f32"), _p(tree_nodes, "u8"), _p(transes, "u8"), _p(pts_se, "i32"),
                                 _p(pts, "f32"), _p(dirs, "f32"), _p(dt, "f32"), _p(t, "f32"), _p(anchors, "i32"),
                                 _p(first_oct_dis, "f32")), "f2n_ray_march_fill")


def ray_march_strided(n_rays, sample_l, scale_by_dis, rays_o, rays_d, noise, oct_se, oct_idx, oct_nf, tree_nodes, transes, counts,
                      s_pts, s_dt, s_t, s_anchors, first_oct_dis, oct_trans=None):
    _ck(lib().f2n_ray_march_strided(_stream(), _i(n_rays), _f(sample_l), _i(int(scale_by_dis)), _p(rays_o, "f32"), _p(rays_d, "f32"),
                                    _p(noise, "f32"), _p(oct_se, "i32"), _p(oct_idx, "i32"), _p(oct_nf, "f32"), _p(tree_nodes, "u8"),
                                    _p(transes, "u8"), _p(counts, "i32"), _p(s_pts, "f32", True), _p(s_dt, "f32"), _p(s_t, "f32"),
                                    _p(s_anchors, "i32"), _p(first_oct_dis, "f32"), _p(oct_trans, "i32", True)), "f2n_ray_march_strided")


def pack_samples(n_rays, pts_se, rays_o, rays_d, transes, s_pts, s_dt, s_t, s_anchors, pts, dirs, dt, t, anchors):
    _ck(lib().f2n_pack_samples(_stream(), _i(n_rays), _p(pts_se, "i32"), _p(rays_o, "f32", True), _p(rays_d, "f32"),
                               _p(transes, "u8", True), _p(s_pts, "f32", True), _p(s_dt, "f32"),
                               _p(s_t, "f32"), _p(s_anchors, "i32"), _p(pts, "f32"), _p(dirs, "f32"), _p(dt, "f32"), _p(t, "f32"),
                               _p(anchors, "i32")), "f2n_pack_samples")


def pack_samples_repair(n_rays, pts_se, rays_o, rays_d, transes, s_pts, s_dt, s_t, s_anchors, pts, dirs, dt, t, anchors, death_epoch,
                        spec_epoch):
    """pack_samples again, on the device only if a leaf died in an epoch >= spec_epoch (see f2n_abi.h, speculative sampling)."""
    _ck(lib().f2n_pack_samples_repair(_stream(), _i(n_rays), _p(pts_se, "i32"), _p(rays_o, "f32", True), _p(rays_d, "f32"),
                                      _p(transes, "u8", True), _p(s_pts, "f32", True), _p(s_dt, "f32"), _p(s_t, "f32"),
                                      _p(s_anchors, "i32"), _p(pts, "f32"), _p(dirs, "f32"), _p(dt, "f32"), _p(t, "f32"),
                                      _p(anchors, "i32"), _p(death_epoch, "i32"), _i(spec_epoch)), "f2n_pack_samples_repair")


def edge_samples(n, edge_pool, transes, edge_idx, edge_coords, out_pts, out_idx):
    _ck(lib().f2n_edge_samples(_stream(), _i(n), _p(edge_pool, "u8"), _p(transes, "u8"), _p(edge_idx, "i32"),
                               _p(edge_coords, "f32"), _p(out_pts, "f32"), _p(out_idx, "i32")), "f2n_edge_samples")


def early_stop_votes(n_rays, pts_se, f0, f0_stride, dt, weights, alphas, mask, kept, anchors, anchor_stride, w_adder, a_adder, mark,
                     visit_cnt):
    _ck(lib().f2n_early_stop_votes(_stream(), _i(n_rays), _p(pts_se, "i32"), _p(f0, "f32"), _i(f0_stride), _p(dt, "f32"),
                                   _p(weights, "f32"), _p(alphas, "f32"), _p(mask, "i32"), _p(kept, "i32"), _i(w_adder.numel()),
                                   _p(anchors, "i32"), _i(anchor_stride), _p(w_adder, "i32"), _p(a_adder, "i32"), _p(mark, "i32"),
                                   _p(visit_cnt, "i32")), "f2n_early_stop_votes")


def oct_mark_visit(n_rays, pts_se, anchors, anchor_stride, weights, alphas, w_adder, a_adder, mark, visit_cnt):
    _ck(lib().f2n_oct_mark_visit(_stream(), _i(n_rays), _i(w_adder.numel()), _p(pts_se, "i32"), _p(anchors, "i32"), _i(anchor_stride),
                                 _p(weights, "f32"), _p(alphas, "f32"), _p(w_adder, "i32"), _p(a_adder, "i32"),
                                 _p(mark, "i32"), _p(visit_cnt, "i32")), "f2n_oct_mark_visit")


def oct_update_stats(n_nodes, w_adder, a_adder, mark, w_stats, a_stats, tree_nodes, child_blocks=None, reset_votes=False):
    _ck(lib().f2n_oct_update_stats(_stream(), _i(n_nodes), _p(w_adder, "i32"), _p(a_adder, "i32"), _p(mark, "i32"),
                                   _p(w_stats, "i32"), _p(a_stats, "i32"), _p(tree_nodes, "u8"),
                                   _p(child_blocks, "u8", True), _i(1 if reset_votes else 0)), "f2n_oct_update_stats")


def oct_update_stats_ex(n_nodes, w_adder, a_adder, mark, w_stats, a_stats, tree_nodes, child_blocks, reset_votes, died_at, epoch,
                        death_epoch):
    _ck(lib().f2n_oct_update_stats_ex(_stream(), _i(n_nodes), _p(w_adder, "i32"), _p(a_adder, "i32"), _p(mark, "i32"),
                                      _p(w_stats, "i32"), _p(a_stats, "i32"), _p(tree_nodes, "u8"), _p(child_blocks, "u8", True),
                                      _i(int(reset_votes)), _p(died_at, "i32", True), _i(epoch), _p(death_epoch, "i32", True),
                                      ctypes.c_void_p(0)), "f2n_oct_update_stats_ex")


def oct_intersect_repair(n_rays, max_hits, search_order, rays_o, rays_d, near, far, tree_nodes, oct_se, oct_idx, oct_nf, total,
                         oct_trans, child_blocks, died_at, spec_epoch, death_epoch, repair_flags, n_repaired=None):
    _ck(lib().f2n_oct_intersect_repair(_stream(), _i(n_rays), _i(max_hits), _p(search_order, "u8"), _p(rays_o, "f32"),
                                       _p(rays_d, "f32"), _f(near), _f(far), _p(tree_nodes, "u8"), _p(oct_se, "i32"),
                                       _p(oct_idx, "i32"), _p(oct_nf, "f32"), _p(total, "i32"), _p(oct_trans, "i32", True),
                                       _p(child_blocks, "u8", True), _p(died_at, "i32"), _i(spec_epoch), _p(death_epoch, "i32"),
                                       _p(repair_flags, "i32"), _p(n_repaired, "i32", True)), "f2n_oct_intersect_repair")


def ray_march_repair(n_rays, sample_l, scale_by_dis, rays_o, rays_d, noise, oct_se, oct_idx, oct_nf, tree_nodes, transes, counts,
                     s_pts, s_dt, s_t, s_anchors, first_oct_dis, oct_trans, repair_flags, death_epoch, spec_epoch):
    _ck(lib().f2n_ray_march_repair(_stream(), _i(n_rays), _f(sample_l), _i(int(scale_by_dis)), _p(rays_o, "f32"), _p(rays_d, "f32"),
                                   _p(noise, "f32"), _p(oct_se, "i32"), _p(oct_idx, "i32"), _p(oct_nf, "f32"), _p(tree_nodes, "u8"),
                                   _p(transes, "u8"), _p(counts, "i32"), _p(s_pts, "f32", True), _p(s_dt, "f32"), _p(s_t, "f32"),
                                   _p(s_anchors, "i32"), _p(first_oct_dis, "f32"), _p(oct_trans, "i32", True),
                                   _p(repair_flags, "i32"), _p(death_epoch, "i32"), _i(spec_epoch)), "f2n_ray_march_repair")


def ray_march_strided_rec(n_rays, max_hits, sample_l, scale_by_dis, rays_o, rays_d, noise, oct_se, oct_idx, oct_nf, tree_nodes, transes,
                          counts, s_pts, s_dt, s_t, s_anchors, first_oct_dis, oct_trans, leaf_state, reached):
    """ray_march_strided that records resumable states per leaf-list entry (tail repair of speculative batches)."""
    _ck(lib().f2n_ray_march_strided_rec(_stream(), _i(n_rays), _i(max_hits), _f(sample_l), _i(int(scale_by_dis)), _p(rays_o, "f32"),
                                        _p(rays_d, "f32"), _p(noise, "f32"), _p(oct_se, "i32"), _p(oct_idx, "i32"), _p(oct_nf, "f32"),
                                        _p(tree_nodes, "u8"), _p(transes, "u8"), _p(counts, "i32"), _p(s_pts, "f32", True),
                                        _p(s_dt, "f32"), _p(s_t, "f32"), _p(s_anchors, "i32"), _p(first_oct_dis, "f32"),
                                        _p(oct_trans, "i32", True), _p(leaf_state, "i32"), _p(reached, "i32")),
        "f2n_ray_march_strided_rec")


def ray_march_persistent(n_rays, max_hits, n_blocks, sample_l, scale_by_dis, rays_o, rays_d, noise, oct_se, oct_idx, oct_nf, tree_nodes,
                         transes, counts, s_pts, s_dt, s_t, s_anchors, first_oct_dis, oct_trans, leaf_state, reached, order, counter, block_waves=1):
    """The strided march on n_blocks persistent waves (workgroups of block_waves), rays sorted by leaf count (see f2n_abi.h)."""
    _ck(lib().f2n_ray_march_persistent(_stream(), _i(n_rays), _i(max_hits), _i(n_blocks), _i(block_waves), _f(sample_l), _i(int(scale_by_dis)),
                                       _p(rays_o, "f32"), _p(rays_d, "f32"), _p(noise, "f32"), _p(oct_se, "i32"), _p(oct_idx, "i32"),
                                       _p(oct_nf, "f32"), _p(tree_nodes, "u8"), _p(transes, "u8"), _p(counts, "i32"),
                                       _p(s_pts, "f32", True), _p(s_dt, "f32"), _p(s_t, "f32"), _p(s_anchors, "i32"),
                                       _p(first_oct_dis, "f32"), _p(oct_trans, "i32", True), _p(leaf_state, "i32", True),
                                       _p(reached, "i32", True), _p(order, "i32"), _p(counter, "i32")), "f2n_ray_march_persistent")


def oct_list_repair(n_rays, max_hits, oct_se, oct_idx, oct_nf, oct_trans, total, died_at, spec_epoch, death_epoch, reached, repair_from,
                    n_repaired, n_full):
    _ck(lib().f2n_oct_list_repair(_stream(), _i(n_rays), _i(max_hits), _p(oct_se, "i32"), _p(oct_idx, "i32"), _p(oct_nf, "f32"),
                                  _p(oct_trans, "i32", True), _p(total, "i32"), _p(died_at, "i32"), _i(spec_epoch),
                                  _p(death_epoch, "i32"), _p(reached, "i32"), _p(repair_from, "i32"), _p(n_repaired, "i32", True),
                                  _p(n_full, "i32")), "f2n_oct_list_repair")


def oct_intersect_repair_flagged(n_rays, max_hits, search_order, rays_o, rays_d, near, far, tree_nodes, oct_se, oct_idx, oct_nf, total,
                                 oct_trans, child_blocks, death_epoch, spec_epoch, repair_from, n_full):
    _ck(lib().f2n_oct_intersect_repair_flagged(_stream(), _i(n_rays), _i(max_hits), _p(search_order, "u8"), _p(rays_o, "f32"),
                                               _p(rays_d, "f32"), _f(near), _f(far), _p(tree_nodes, "u8"), _p(oct_se, "i32"),
                                               _p(oct_idx, "i32"), _p(oct_nf, "f32"), _p(total, "i32"), _p(oct_trans, "i32", True),
                                               _p(child_blocks, "u8", True), _p(death_epoch, "i32"), _i(spec_epoch),
                                               _p(repair_from, "i32"), _p(n_full, "i32")), "f2n_oct_intersect_repair_flagged")


def ray_march_repair_tail(n_rays, max_hits, sample_l, scale_by_dis, rays_o, rays_d, noise, oct_se, oct_idx, oct_nf, tree_nodes, transes,
                          counts, s_pts, s_dt, s_t, s_anchors, first_oct_dis, oct_trans, leaf_state, reached, repair_from, death_epoch,
                          spec_epoch):
    _ck(lib().f2n_ray_march_repair_tail(_stream(), _i(n_rays), _i(max_hits), _f(sample_l), _i(int(scale_by_dis)), _p(rays_o, "f32"),
                                        _p(rays_d, "f32"), _p(noise, "f32"), _p(oct_se, "i32"), _p(oct_idx, "i32"), _p(oct_nf, "f32"),
                                        _p(tree_nodes, "u8"), _p(transes, "u8"), _p(counts, "i32"), _p(s_pts, "f32", True),
                                        _p(s_dt, "f32"), _p(s_t, "f32"), _p(s_anchors, "i32"), _p(first_oct_dis, "f32"),
                                        _p(oct_trans, "i32", True), _p(leaf_state, "i32"), _p(reached, "i32"), _p(repair_from, "i32"),
                                        _p(death_epoch, "i32"), _i(spec_epoch)), "f2n_ray_march_repair_tail")


def oct_build_child_blocks(n_nodes, tree_nodes, child_blocks):
    _ck(lib().f2n_oct_build_child_blocks(_stream(), _i(n_nodes), _p(tree_nodes, "u8"), _p(child_blocks, "u8")),
        "f2n_oct_build_child_blocks")


def oct_mark_invisible(n_nodes, n_cams, tree_nodes, intris, w2cs, bounds):
    _ck(lib().f2n_oct_mark_invisible(_stream(), _i(n_nodes), _i(n_cams), _p(tree_nodes, "u8"), _p(intris, "f32"),
                                     _p(w2cs, "f32"), _p(bounds, "f32")), "f2n_oct_mark_invisible")


# ---------------------------------------------------------------- hash grid / MLP / field
def hash_fwd(n, n_volumes, table_h, prim_pool, local_idx, local_size, bias_pool, level_scale, pts, pts_are_warped,
             volume_idx, vol_stride, out_h):
    _ck(lib().f2n_hash_fwd(_stream(), _i(n), _i(n_volumes), _p(table_h, "h16"), _p(prim_pool, "i32"), _p(local_idx, "i32"),
                           _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"), _p(pts, "f32"),
                           _i(int(pts_are_warped)), _p(volume_idx, "i32"), _i(vol_stride), _p(out_h, "h16")), "f2n_hash_fwd")


def hash_bwd(n, n_volumes, prim_pool, local_idx, local_size, bias_pool, level_scale, pts, pts_are_warped, volume_idx,
             vol_stride, grad_in_h, grad_table_h, level_entries=0):
    _ck(lib().f2n_hash_bwd(_stream(), _i(n), _i(n_volumes), _p(prim_pool, "i32"), _p(local_idx, "i32"),
                           _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"), _p(pts, "f32"),
                           _i(int(pts_are_warped)), _p(volume_idx, "i32"), _i(vol_stride), _p(grad_in_h, "h16"),
                           _p(grad_table_h, "h16"), _i(level_entries)), "f2n_hash_bwd")


def mlp_n_params(d_in, d_hidden, n_hidden):
    return lib().f2n_mlp_n_params(_i(d_in), _i(d_hidden), _i(n_hidden))


def mlp_init_params(seed, d_in, d_hidden, n_hidden, params_f32):
    _ck(lib().f2n_mlp_init_params(_stream(), ctypes.c_uint64(seed), _i(d_in), _i(d_hidden), _i(n_hidden),
                                  _p(params_f32, "f32")), "f2n_mlp_init_params")


def params_to_h16(n, params_f32, params_h):
    _ck(lib().f2n_params_to_h16(_stream(), _i(n), _p(params_f32, "f32"), _p(params_h, "h16")), "f2n_params_to_h16")


def mlp_fwd(n, d_in, d_hidden, n_hidden, params_h, x, out_h):
    _ck(lib().f2n_mlp_fwd(_stream(), _i(n), _i(d_in), _i(d_hidden), _i(n_hidden), _p(params_h, "h16"), _p(x, "f32"),
                          _p(out_h, "h16")), "f2n_mlp_fwd")


def mlp_bwd(n, d_in, d_hidden, n_hidden, loss_scale, params_h, x, dy, dparams_scaled, dx):
    _ck(lib().f2n_mlp_bwd(_stream(), _i(n), _i(d_in), _i(d_hidden), _i(n_hidden), _f(loss_scale), _p(params_h, "h16"),
                          _p(x, "f32"), _p(dy, "f32"), _p(dparams_scaled, "f32"), _p(dx, "f32", True)), "f2n_mlp_bwd")


def field_fwd(n, n_volumes, table_h, prim_pool, local_idx, local_size, bias_pool, level_scale, pts_warped, volume_idx,
              vol_stride, mlp_params_h, out_feat, out_f0, save_x_h):
    _ck(lib().f2n_field_fwd(_stream(), _i(n), _i(n_volumes), _p(table_h, "h16"), _p(prim_pool, "i32"), _p(local_idx, "i32"),
                            _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"), _p(pts_warped, "f32"),
                            _p(volume_idx, "i32"), _i(vol_stride), _p(mlp_params_h, "h16"), _p(out_feat, "f32", True),
                            _p(out_f0, "f32", True), _p(save_x_h, "h16", True)), "f2n_field_fwd")


def field_fwd_ex(n, n_volumes, table_h, prim_pool, local_idx, local_size, bias_pool, level_scale, pts_warped, volume_idx,
                 vol_stride, mlp_params_h, out_feat, out_f0, save_x_h, out_feat_h, fused=False):
    """f2n_field_fwd_ex / f2n_field_fwd_fused_ex (include/f2n_abi.h, "Reuse of the density pre-pass's field outputs"): field_fwd
    with out_feat_h [n,16] h16, the network's outputs at their f16 output precision."""
    fn, name = (lib().f2n_field_fwd_fused_ex, "f2n_field_fwd_fused_ex") if fused else (lib().f2n_field_fwd_ex, "f2n_field_fwd_ex")
    _ck(fn(_stream(), _i(n), _i(n_volumes), _p(table_h, "h16"), _p(prim_pool, "i32"), _p(local_idx, "i32"),
           _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"), _p(pts_warped, "f32"),
           _p(volume_idx, "i32"), _i(vol_stride), _p(mlp_params_h, "h16"), _p(out_feat, "f32", True),
           _p(out_f0, "f32", True), _p(save_x_h, "h16", True), _p(out_feat_h, "h16", True)), name)


def hash_gather_planes(n, n_volumes, table_h, prim_pool, local_idx, local_size, bias_pool, level_scale, pts, pts_are_warped,
                       volume_idx, vol_stride, planes_h):
    _ck(lib().f2n_hash_gather_planes(_stream(), _i(n), _i(n_volumes), _p(table_h, "h16"), _p(prim_pool, "i32"),
                                     _p(local_idx, "i32"), _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"),
                                     _p(pts, "f32"), _i(int(pts_are_warped)), _p(volume_idx, "i32"), _i(vol_stride),
                                     _p(planes_h, "h16")), "f2n_hash_gather_planes")


def hash_gather_planes_binned(n, n_volumes, table_h, prim_pool, local_idx, local_size, bias_pool, level_scale, pts, pts_are_warped,
                              volume_idx, vol_stride, planes_h, level_entries, first_binned_pair):
    """hash_gather_planes for tables beyond the L2s: level pairs >= first_binned_pair through the slice-binned pipeline."""
    _ck(lib().f2n_hash_gather_planes_binned(_stream(), _i(n), _i(n_volumes), _p(table_h, "h16"), _p(prim_pool, "i32"),
                                            _p(local_idx, "i32"), _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"),
                                            _p(pts, "f32"), _i(int(pts_are_warped)), _p(volume_idx, "i32"), _i(vol_stride),
                                            _p(planes_h, "h16"), _i(level_entries), _i(first_binned_pair)),
        "f2n_hash_gather_planes_binned")


def hash_gather_planes_balanced(n, n_volumes, table_h, prim_pool, local_idx, local_size, bias_pool, level_scale, pts,
                                pts_are_warped, volume_idx, vol_stride, planes_h, step01, level_scale_host):
    """level_scale_host: 16 floats on the HOST (numpy array / list); step01 <= 0 -> the plain one-pair-per-XCD gather."""
    import ctypes
    arr = (ctypes.c_float * 16)(*[float(v) for v in level_scale_host])
    _ck(lib().f2n_hash_gather_planes_balanced(_stream(), _i(n), _i(n_volumes), _p(table_h, "h16"), _p(prim_pool, "i32"),
                                              _p(local_idx, "i32"), _p(local_size, "i32"), _p(bias_pool, "f32"),
                                              _p(level_scale, "f32"), _p(pts, "f32"), _i(int(pts_are_warped)),
                                              _p(volume_idx, "i32"), _i(vol_stride), _p(planes_h, "h16"),
                                              ctypes.c_float(step01), arr), "f2n_hash_gather_planes_balanced")


def hash_gather_variant(n, n_volumes, step01, level_scale_host):
    """bit 0: staged hash constants, bit 1: run combining + balanced split (what f2n_hash_gather_planes_balanced would launch)."""
    import ctypes
    arr = (ctypes.c_float * 16)(*[float(v) for v in level_scale_host])
    rc = lib().f2n_hash_gather_variant(_i(n), _i(n_volumes), ctypes.c_float(step01), arr)
    if rc < 0:
        _ck(rc, "f2n_hash_gather_variant")
    return rc


def field_mlp_planes(n, planes_h, mlp_params_h, out_feat, out_f0, save_x_h):
    _ck(lib().f2n_field_mlp_planes(_stream(), _i(n), _p(planes_h, "h16"), _p(mlp_params_h, "h16"), _p(out_feat, "f32", True),
                                   _p(out_f0, "f32", True), _p(save_x_h, "h16", True)), "f2n_field_mlp_planes")


def field_mlp_planes_ex(n, planes_h, mlp_params_h, out_feat, out_f0, save_x_h, out_feat_h):
    """f2n_field_mlp_planes_ex: field_mlp_planes with out_feat_h [n,16] h16 (the pre-pass's field outputs, kept for shade_fwd_feat)."""
    _ck(lib().f2n_field_mlp_planes_ex(_stream(), _i(n), _p(planes_h, "h16"), _p(mlp_params_h, "h16"), _p(out_feat, "f32", True),
                                      _p(out_f0, "f32", True), _p(save_x_h, "h16", True), _p(out_feat_h, "h16", True)),
        "f2n_field_mlp_planes_ex")


def field_fwd_cached(n, n_cache, src_rows, x_cache_h, mlp_params_h, out_feat, out_f0, save_x_h):
    _ck(lib().f2n_field_fwd_cached(_stream(), _i(n), _i(n_cache), _p(src_rows, "i32", True), _p(x_cache_h, "h16"),
                                   _p(mlp_params_h, "h16"), _p(out_feat, "f32", True), _p(out_f0, "f32", True),
                                   _p(save_x_h, "h16", True)), "f2n_field_fwd_cached")


def field_bwd(n, n_volumes, prim_pool, local_idx, local_size, bias_pool, level_scale, pts_warped, volume_idx, vol_stride,
              mlp_params_h, saved_x_h, dfeat, loss_scale, dparams_scaled, grad_table_h, level_entries=0):
    _ck(lib().f2n_field_bwd(_stream(), _i(n), _i(n_volumes), _p(prim_pool, "i32"), _p(local_idx, "i32"),
                            _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"), _p(pts_warped, "f32"),
                            _p(volume_idx, "i32"), _i(vol_stride), _p(mlp_params_h, "h16"), _p(saved_x_h, "h16"),
                            _p(dfeat, "f32"), _f(loss_scale), _p(dparams_scaled, "f32"), _p(grad_table_h, "h16"),
                            _i(level_entries)), "f2n_field_bwd")


# ---------------------------------------------------------------- shader
def sh_encode(n, degree, dirs, out):
    _ck(lib().f2n_sh_encode(_stream(), _i(n), _i(degree), _p(dirs, "f32"), _p(out, "f32")), "f2n_sh_encode")


def scatter_idx(n_rays, start_end, ray_val, out):
    _ck(lib().f2n_scatter_idx(_stream(), _i(n_rays), _p(start_end, "i32"), _p(ray_val, "i32"), _p(out, "i32")),
        "f2n_scatter_idx")


def shade_fwd(n, feat, dirs, app_emb, sample_emb_idx, mlp_params_h, rgb, save_x_h):
    _ck(lib().f2n_shade_fwd(_stream(), _i(n), _p(feat, "f32"), _p(dirs, "f32"), _p(app_emb, "f32", True),
                            _p(sample_emb_idx, "i32", True), _p(mlp_params_h, "h16"), _p(rgb, "f32"),
                            _p(save_x_h, "h16", True)), "f2n_shade_fwd")


def field_shade_fwd(n, src_rows, x_cache_h, field_params_h, dirs, app_emb, sample_emb_idx, color_params_h, out_f0, save_field_x_h,
                    save_shade_x_h, rgb, n_dev=None, x_extra_h=None, feat_extra=None, save_x_extra_h=None):
    n_extra = 0 if x_extra_h is None else x_extra_h.shape[0]
    _ck(lib().f2n_field_shade_fwd_extra(_stream(), _i(n), _p(n_dev, "i32", True), _p(src_rows, "i32", True), _p(x_cache_h, "h16"),
                                        _p(field_params_h, "h16"), _p(dirs, "f32"), _p(app_emb, "f32", True),
                                        _p(sample_emb_idx, "i32", True), _p(color_params_h, "h16"), _p(out_f0, "f32", True),
                                        _p(save_field_x_h, "h16", True), _p(save_shade_x_h, "h16", True), _p(rgb, "f32"), _i(n_extra),
                                        _p(x_extra_h, "h16", True), _p(feat_extra, "f32", True), _p(save_x_extra_h, "h16", True)),
        "f2n_field_shade_fwd_extra")


def shade_fwd_feat(n, src_rows, feat_cache_h, dirs, app_emb, sample_emb_idx, color_params_h, out_f0, save_shade_x_h, rgb, n_dev=None,
                   feat_extra_h=None, feat_extra=None):
    """f2n_shade_fwd_feat: field_shade_fwd's colour path from the pre-pass's cached field outputs feat_cache_h [*,16] h16 (no field
    network); the extra (edge) rows feat_extra_h [n_extra,16] h16 are widened into feat_extra fp32."""
    n_extra = 0 if feat_extra_h is None else feat_extra_h.shape[0]
    _ck(lib().f2n_shade_fwd_feat(_stream(), _i(n), _p(n_dev, "i32", True), _p(src_rows, "i32", True), _p(feat_cache_h, "h16"),
                                 _p(dirs, "f32"), _p(app_emb, "f32", True), _p(sample_emb_idx, "i32", True), _p(color_params_h, "h16"),
                                 _p(out_f0, "f32", True), _p(save_shade_x_h, "h16", True), _p(rgb, "f32"), _i(n_extra),
                                 _p(feat_extra_h, "h16", True), _p(feat_extra, "f32", True)), "f2n_shade_fwd_feat")


def shade_bwd(n, drgb, sample_emb_idx, mlp_params_h, saved_x_h, loss_scale, dfeat, dparams_scaled, dapp_emb, df0=None):
    _ck(lib().f2n_shade_bwd(_stream(), _i(n), _p(drgb, "f32"), _p(sample_emb_idx, "i32", True), _p(mlp_params_h, "h16"),
                            _p(saved_x_h, "h16"), _f(loss_scale), _p(dfeat, "f32"), _p(dparams_scaled, "f32"),
                            _p(dapp_emb, "f32", True), _i(0 if dapp_emb is None else dapp_emb.shape[0]), _p(df0, "f32", True)),
        "f2n_shade_bwd")


# ---------------------------------------------------------------- ray generation
def img2world_rays(n, poses, intri, dist_params, cam_idx, ij, rays_o, rays_d):
    _ck(lib().f2n_img2world_rays(_stream(), _i(n), _p(poses, "f32"), _p(intri, "f32"), _p(dist_params, "f32"), _p(cam_idx, "i32"),
                                 _p(ij, "i32"), _p(rays_o, "f32"), _p(rays_d, "f32")), "f2n_img2world_rays")


def draw_ray_batch(n_rays, u01, image_set, height, width, poses, intri, dist_params, images, cam_bounds, cam_indices, ij, rays_o,
                   rays_d, gt_colors, bounds):
    _ck(lib().f2n_draw_ray_batch(_stream(), _i(n_rays), _p(u01, "f32"), _p(image_set, "i32"), _i(int(image_set.numel())), _i(height),
                                 _i(width), _p(poses, "f32"), _p(intri, "f32"), _p(dist_params, "f32"), _p(images, "f32", True),
                                 _p(cam_bounds, "f32"), _p(cam_indices, "i32"), _p(ij, "i32"), _p(rays_o, "f32"), _p(rays_d, "f32"),
                                 _p(gt_colors, "f32", True), _p(bounds, "f32")), "f2n_draw_ray_batch")


def gather_pixels(n, height, width, images, cam_bounds, cam_idx, ij, gt_colors, bounds):
    _ck(lib().f2n_gather_pixels(_stream(), _i(n), _i(height), _i(width), _p(images, "f32", True), _p(cam_bounds, "f32", True),
                                _p(cam_idx, "i32"), _p(ij, "i32"), _p(gt_colors, "f32", True), _p(bounds, "f32", True)),
        "f2n_gather_pixels")


# ---------------------------------------------------------------- renderer
def early_stop(n_rays, pts_se, f0, f0_stride, dt, weights, alphas, mask, kept):
    _ck(lib().f2n_early_stop(_stream(), _i(n_rays), _p(pts_se, "i32"), _p(f0, "f32"), _i(f0_stride), _p(dt, "f32"),
                             _p(weights, "f32"), _p(alphas, "f32"), _p(mask, "i32"), _p(kept, "i32")), "f2n_early_stop")


def compact_samples(n_rays, old_se, new_se, mask, pts, dirs, dt, t, anchors, o_pts, o_dirs, o_dt, o_t, o_anchors):
    _ck(lib().f2n_compact_samples(_stream(), _i(n_rays), _p(old_se, "i32"), _p(new_se, "i32"), _p(mask, "i32"),
                                  _p(pts, "f32"), _p(dirs, "f32"), _p(dt, "f32"), _p(t, "f32"), _p(anchors, "i32"),
                                  _p(o_pts, "f32"), _p(o_dirs, "f32"), _p(o_dt, "f32"), _p(o_t, "f32"),
                                  _p(o_anchors, "i32")), "f2n_compact_samples")


def compact_samples_src(n_rays, old_se, new_se, mask, pts, dirs, dt, t, anchors, o_pts, o_dirs, o_dt, o_t, o_anchors, o_src,
                        o_vol=None, ray_val=None, o_ray_val=None):
    _ck(lib().f2n_compact_samples_src(_stream(), _i(n_rays), _p(old_se, "i32"), _p(new_se, "i32"), _p(mask, "i32"),
                                      _p(pts, "f32"), _p(dirs, "f32"), _p(dt, "f32"), _p(t, "f32"), _p(anchors, "i32"),
                                      _p(o_pts, "f32"), _p(o_dirs, "f32"), _p(o_dt, "f32"), _p(o_t, "f32"),
                                      _p(o_anchors, "i32", True), _p(o_src, "i32"), _p(o_vol, "i32", True), _p(ray_val, "i32", True),
                                      _p(o_ray_val, "i32", True)), "f2n_compact_samples_src")


def oct_visible_cams(n_boxes, n_cams, boxes, c2w, bounds, fx, fy, cx, cy, res_h, res_w, pix_i, pix_j, visible):
    _ck(lib().f2n_oct_visible_cams(_stream(), _i(n_boxes), _i(n_cams), _p(boxes, "f32"), _p(c2w, "f32"), _p(bounds, "f32"), _f(fx),
                                   _f(fy), _f(cx), _f(cy), _i(res_h), _i(res_w), _p(pix_i, "f32"), _p(pix_j, "f32"),
                                   _p(visible, "u8")), "f2n_oct_visible_cams")


def march_noise(n, u, fineness, out):
    _ck(lib().f2n_march_noise(_stream(), _i(n), _p(u, "f32"), _f(fineness), _p(out, "f32")), "f2n_march_noise")


def composite_fwd(n_rays, pts_se, feat, dt, t, rgb, bg, colors, disparity, depth, weights, f0_stride=16, out_vars=None):
    """feat: the field output [M,16] (f0_stride 16, column 0 is read) or a compact density array [M] (f0_stride 1)."""
    _ck(lib().f2n_composite_fwd(_stream(), _i(n_rays), _p(pts_se, "i32"), _p(feat, "f32"), _i(f0_stride), _p(dt, "f32"),
                                _p(t, "f32"), _p(rgb, "f32"), _p(bg, "f32"), _p(colors, "f32"), _p(disparity, "f32"),
                                _p(depth, "f32"), _p(weights, "f32"), _p(out_vars, "f32", True)), "f2n_composite_fwd")


def composite_bwd(n_rays, pts_se, feat, dt, t, rgb, bg, dcolors, ddisp, ddepth, dweights, gs_progress, drgb, dfeat, f0_stride=16,
                  df0_stride=16, var_weights=None, dvars=None):
    _ck(lib().f2n_composite_bwd(_stream(), _i(n_rays), _p(pts_se, "i32"), _p(feat, "f32"), _i(f0_stride), _p(dt, "f32"),
                                _p(t, "f32"), _p(rgb, "f32"), _p(bg, "f32"), _p(dcolors, "f32", True), _p(ddisp, "f32", True),
                                _p(ddepth, "f32", True), _p(dweights, "f32", True), _f(gs_progress), _p(drgb, "f32"),
                                _p(dfeat, "f32"), _i(df0_stride), _p(var_weights, "f32", True), _p(dvars, "f32", True)),
        "f2n_composite_bwd")


def weight_var_fwd(n_rays, weights, pts_se, out):
    _ck(lib().f2n_weight_var_fwd(_stream(), _i(n_rays), _p(weights, "f32"), _p(pts_se, "i32"), _p(out, "f32")),
        "f2n_weight_var_fwd")


def weight_var_bwd(n_rays, weights, pts_se, dvars, dweights):
    _ck(lib().f2n_weight_var_bwd(_stream(), _i(n_rays), _p(weights, "f32"), _p(pts_se, "i32"), _p(dvars, "f32"),
                                 _p(dweights, "f32")), "f2n_weight_var_bwd")


def distortion_fwd(n_rays, pts_se, weights, dt, dist):
    """dist [R]: the distortion loss of every ray on its warped intervals (f2n_distortion_fwd; no reference counterpart)."""
    _ck(lib().f2n_distortion_fwd(_stream(), _i(n_rays), _p(pts_se, "i32"), _p(weights, "f32"), _p(dt, "f32"), _p(dist, "f32")),
        "f2n_distortion_fwd")


def distortion_bwd(n_rays, pts_se, weights, dt, ddist, dweights, dist=None):
    """dweights [M] = ddist[ray] * d dist / d w for the samples of non-empty rays (the rest is untouched); dist [R] if given."""
    _ck(lib().f2n_distortion_bwd(_stream(), _i(n_rays), _p(pts_se, "i32"), _p(weights, "f32"), _p(dt, "f32"), _p(ddist, "f32"),
                                 _p(dweights, "f32"), _p(dist, "f32", True)), "f2n_distortion_bwd")


def loss_add_mean(n, x, weight, losses, slot):
    """losses[slot] = mean(x[:n]), losses[0] += weight * mean (f2n_loss_add_mean: one workgroup, fp64, a fixed order)."""
    _ck(lib().f2n_loss_add_mean(_stream(), _i(n), _p(x, "f32"), _f(weight), _p(losses, "f32"), _i(slot)), "f2n_loss_add_mean")


def flex_sum_fwd(n_rays, vec, val, se, out):
    _ck(lib().f2n_flex_sum_fwd(_stream(), _i(n_rays), _i(vec), _p(val, "f32"), _p(se, "i32"), _p(out, "f32")), "f2n_flex_sum_fwd")


def flex_sum_bwd(n_rays, vec, dsum, se, out):
    _ck(lib().f2n_flex_sum_bwd(_stream(), _i(n_rays), _i(vec), _p(dsum, "f32"), _p(se, "i32"), _p(out, "f32")), "f2n_flex_sum_bwd")


def flex_acc_fwd(n_rays, include_this, val, se, out):
    _ck(lib().f2n_flex_acc_fwd(_stream(), _i(n_rays), _i(int(include_this)), _p(val, "f32"), _p(se, "i32"), _p(out, "f32")),
        "f2n_flex_acc_fwd")


def flex_acc_bwd(n_rays, include_this, dsum, se, out):
    _ck(lib().f2n_flex_acc_bwd(_stream(), _i(n_rays), _i(int(include_this)), _p(dsum, "f32"), _p(se, "i32"), _p(out, "f32")),
        "f2n_flex_acc_bwd")


# ---------------------------------------------------------------- optimiser
def adam_coefficients(step, lr, beta1=0.9, beta2=0.99, eps=1e-15, weight_decay=0.0, grad_scale=1.0):
    """The nine float scalars the Adam kernels are launched with (host function, no device): [lr / (1 - beta1^step),
    sqrt(1 - beta2^step), beta1, beta2, 1 - beta1, 1 - beta2, eps, weight_decay, grad_scale]."""
    out = (ctypes.c_float * 9)()
    _ck(lib().f2n_adam_coefficients(_i(step), _f(lr), _d(beta1), _d(beta2), _f(eps), _f(weight_decay), _f(grad_scale), out),
        "f2n_adam_coefficients")
    return [float(v) for v in out]


def adam_step(n, param, grad, grad_scale, grad_round_h16, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, wd, param_h,
              skip_flag=None, zero_grad=False):
    _ck(lib().f2n_adam_step(_stream(), _i(n), _p(param, "f32"), _p(grad, "f32"), _f(grad_scale), _i(int(grad_round_h16)),
                            _p(exp_avg, "f32"), _p(exp_avg_sq, "f32"), _i(step), _f(lr), _d(beta1), _d(beta2), _f(eps),
                            _f(wd), _p(param_h, "h16", True), _i(int(zero_grad)), _p(skip_flag, "i32", True)), "f2n_adam_step")


class _AdamGroup(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("param_h", ctypes.c_void_p), ("n", ctypes.c_int), ("grad_scale", ctypes.c_float), ("weight_decay", ctypes.c_float),
                ("grad_round_h16", ctypes.c_int), ("check_finite", ctypes.c_int)]


def adam_small_groups(groups, step, lr, beta1, beta2, eps, zero_grad, flags=None, skip_flag=None):
    """groups: list of dicts {param, grad, exp_avg, exp_avg_sq, param_h (or None), grad_scale, weight_decay, grad_round_h16,
    check_finite}; one launch (f2n_adam_small_groups)."""
    arr = (_AdamGroup * len(groups))()
    for a, g in zip(arr, groups):
        a.param = _p(g["param"], "f32").value
        a.grad = _p(g["grad"], "f32").value
        a.exp_avg = _p(g["exp_avg"], "f32").value
        a.exp_avg_sq = _p(g["exp_avg_sq"], "f32").value
        a.param_h = _p(g.get("param_h"), "h16", True).value
        a.n = int(g["param"].numel())
        a.grad_scale = float(g["grad_scale"])
        a.weight_decay = float(g["weight_decay"])
        a.grad_round_h16 = int(bool(g.get("grad_round_h16", False)))
        a.check_finite = int(bool(g.get("check_finite", False)))
    _ck(lib().f2n_adam_small_groups(_stream(), _i(len(groups)), arr, _i(step), _f(lr), _d(beta1), _d(beta2), _f(eps),
                                    _i(int(zero_grad)), _p(flags, "i32", True), _p(skip_flag, "i32", True)), "f2n_adam_small_groups")


def adam_fused(groups, table, step, lr, beta1, beta2, eps, zero_grad, skip_flag=None):
    """groups as in adam_small_groups (check_finite ignored); table: dict {param, grad_h, exp_avg, exp_avg_sq, param_h, grad_scale, n}
    or None; ONE launch (f2n_adam_fused)."""
    arr = (_AdamGroup * max(len(groups), 1))()
    for a, g in zip(arr, groups):
        a.param = _p(g["param"], "f32").value
        a.grad = _p(g["grad"], "f32").value
        a.exp_avg = _p(g["exp_avg"], "f32").value
        a.exp_avg_sq = _p(g["exp_avg_sq"], "f32").value
        a.param_h = _p(g.get("param_h"), "h16", True).value
        a.n = int(g["param"].numel())
        a.grad_scale = float(g["grad_scale"])
        a.weight_decay = float(g["weight_decay"])
        a.grad_round_h16 = int(bool(g.get("grad_round_h16", False)))
        a.check_finite = 0
    t = table or {}
    _ck(lib().f2n_adam_fused(_stream(), _i(len(groups)), arr, _i(int(t.get("n", 0))), _p(t.get("param"), "f32", True),
                             _p(t.get("grad_h"), "h16", True), _f(float(t.get("grad_scale", 1.0))), _p(t.get("exp_avg"), "f32", True),
                             _p(t.get("exp_avg_sq"), "f32", True), _p(t.get("param_h"), "h16", True), _i(step), _f(lr), _d(beta1),
                             _d(beta2), _f(eps), _i(int(zero_grad)), _p(skip_flag, "i32", True)), "f2n_adam_fused")


def field_bwd_dyn(n_max, n_dev, n_off, n_volumes, prim_pool, local_idx, local_size, bias_pool, level_scale, pts_warped, volume_idx,
                  vol_stride, mlp_params_h, saved_x_h, dfeat, loss_scale, dparams_scaled, grad_table_h, level_entries, defer_reduce):
    _ck(lib().f2n_field_bwd_dyn(_stream(), _i(n_max), _p(n_dev, "i32", True), _i(n_off), _i(n_volumes), _p(prim_pool, "i32"),
                                _p(local_idx, "i32"), _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"),
                                _p(pts_warped, "f32"), _p(volume_idx, "i32"), _i(vol_stride), _p(mlp_params_h, "h16"),
                                _p(saved_x_h, "h16"), _p(dfeat, "f32"), _f(loss_scale), _p(dparams_scaled, "f32"),
                                _p(grad_table_h, "h16"), _i(level_entries), _i(int(defer_reduce))), "f2n_field_bwd_dyn")


def field_bwd_dyn_rows(n_max, n_dev, n_off, n_volumes, prim_pool, local_idx, local_size, bias_pool, level_scale, pts_warped, volume_idx,
                       vol_stride, mlp_params_h, x_edge_h, x_cache_h, src_rows, dfeat, loss_scale, dparams_scaled, grad_table_h,
                       level_entries, defer_reduce):
    """f2n_field_bwd_dyn_rows: field_bwd_dyn whose input rows are read in place -- rows < n_off from x_edge_h [n_off,32] (None when
    n_off == 0), row s >= n_off = row src_rows[s - n_off] of x_cache_h (the pre-pass feature cache)."""
    _ck(lib().f2n_field_bwd_dyn_rows(_stream(), _i(n_max), _p(n_dev, "i32", True), _i(n_off), _i(n_volumes), _p(prim_pool, "i32"),
                                     _p(local_idx, "i32"), _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"),
                                     _p(pts_warped, "f32"), _p(volume_idx, "i32"), _i(vol_stride), _p(mlp_params_h, "h16"),
                                     _p(x_edge_h, "h16", True), _p(x_cache_h, "h16"), _p(src_rows, "i32"), _p(dfeat, "f32"),
                                     _f(loss_scale), _p(dparams_scaled, "f32"), _p(grad_table_h, "h16"), _i(level_entries),
                                     _i(int(defer_reduce))), "f2n_field_bwd_dyn_rows")


def field_bwd_dyn_planes(n_max, n_dev, n_off, n_volumes, prim_pool, local_idx, local_size, bias_pool, level_scale, pts_warped, volume_idx,
                         vol_stride, mlp_params_h, x_edge_h, x_edge_planes_h, x_planes_h, plane_rows, src_rows, dfeat, loss_scale,
                         dparams_scaled, grad_table_h, level_entries, defer_reduce):
    """f2n_field_bwd_dyn_planes: field_bwd_dyn_rows on the gather's f16 planes [8][plane_rows][4] -- x_planes_h is a contiguous view
    that starts at the survivors' first row of plane 0; the edge rows from x_edge_h [n_off,32] or, when x_edge_planes_h (a view that
    starts at the edge samples' first row of plane 0) is given, from the planes."""
    _ck(lib().f2n_field_bwd_dyn_planes(_stream(), _i(n_max), _p(n_dev, "i32", True), _i(n_off), _i(n_volumes), _p(prim_pool, "i32"),
                                       _p(local_idx, "i32"), _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"),
                                       _p(pts_warped, "f32"), _p(volume_idx, "i32"), _i(vol_stride), _p(mlp_params_h, "h16"),
                                       _p(x_edge_h, "h16", True), _p(x_edge_planes_h, "h16", True), _p(x_planes_h, "h16"), _i(plane_rows),
                                       _p(src_rows, "i32"), _p(dfeat, "f32"), _f(loss_scale), _p(dparams_scaled, "f32"),
                                       _p(grad_table_h, "h16"), _i(level_entries), _i(int(defer_reduce))), "f2n_field_bwd_dyn_planes")


class _StepTail(ctypes.Structure):
    _fields_ = [("n_flags_a", ctypes.c_int), ("flags_grad_a", ctypes.c_void_p), ("n_flags_b", ctypes.c_int), ("flags_grad_b", ctypes.c_void_p),
                ("flags", ctypes.c_void_p), ("flags_mirror", ctypes.c_void_p), ("n_groups", ctypes.c_int), ("groups", ctypes.c_void_p),
                ("n_table", ctypes.c_int), ("table_param", ctypes.c_void_p), ("table_exp_avg", ctypes.c_void_p),
                ("table_exp_avg_sq", ctypes.c_void_p), ("table_param_h", ctypes.c_void_p), ("table_grad_scale", ctypes.c_float),
                ("step", ctypes.c_int), ("lr", ctypes.c_float), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_float),
                ("after_reduce", ctypes.c_void_p), ("after_reduce_user", ctypes.c_void_p), ("leave_table_to_caller", ctypes.c_int)]


def field_bwd_step_tail(n_max, n_dev, n_off, n_volumes, prim_pool, local_idx, local_size, bias_pool, level_scale, pts_warped, volume_idx,
                        vol_stride, mlp_params_h, saved_x_h, dfeat, loss_scale, dparams_scaled, grad_table_h, level_entries, flags_a,
                        flags_b, flags, groups, table, step, lr, beta1, beta2, eps, tail_stream=None, flags_mirror=None, leave_table_to_caller=False,
                        after_reduce=None, x_cache_h=None, src_rows=None, plane_rows=0, x_edge_planes_h=None):
    """f2n_field_bwd_step_tail: the field backward + the rest of the training step (deferred reductions, finiteness flags, Adam of
    `groups` (as adam_fused) and of `table` = {param, exp_avg, exp_avg_sq, param_h, grad_scale, n}) re-ordered around the scatter.
    Returns 1 when the scatter's owners stepped the table.  x_cache_h / src_rows given: f2n_field_bwd_step_tail_rows, with
    saved_x_h as its x_edge_h (rows < n_off; None when n_off == 0) -- see field_bwd_dyn_rows.  plane_rows > 0:
    f2n_field_bwd_step_tail_planes, x_cache_h as its x_planes_h -- see field_bwd_dyn_planes."""
    arr = (_AdamGroup * max(len(groups), 1))()
    for a, g in zip(arr, groups):
        a.param = _p(g["param"], "f32").value
        a.grad = _p(g["grad"], "f32").value
        a.exp_avg = _p(g["exp_avg"], "f32").value
        a.exp_avg_sq = _p(g["exp_avg_sq"], "f32").value
        a.param_h = _p(g.get("param_h"), "h16", True).value
        a.n = int(g["param"].numel())
        a.grad_scale = float(g["grad_scale"])
        a.weight_decay = float(g["weight_decay"])
        a.grad_round_h16 = int(bool(g.get("grad_round_h16", False)))
        a.check_finite = 0
    t = _StepTail()
    t.n_flags_a, t.flags_grad_a = int(flags_a.numel()), _p(flags_a, "f32").value
    t.n_flags_b, t.flags_grad_b = int(flags_b.numel()), _p(flags_b, "f32").value
    t.flags, t.flags_mirror = _p(flags, "i32").value, _mapped(flags_mirror).value
    t.n_groups, t.groups = len(groups), ctypes.cast(arr, ctypes.c_void_p).value
    t.n_table = int(table["n"])
    t.table_param, t.table_exp_avg, t.table_exp_avg_sq = _p(table["param"], "f32").value, _p(table["exp_avg"], "f32").value, _p(table["exp_avg_sq"], "f32").value
    t.table_param_h, t.table_grad_scale = _p(table["param_h"], "h16").value, float(table["grad_scale"])
    t.step, t.lr, t.beta1, t.beta2, t.eps = int(step), float(lr), float(beta1), float(beta2), float(eps)
    t.leave_table_to_caller = int(bool(leave_table_to_caller))
    cb = None
    if after_reduce is not None:  # (python callable(chain_stream_handle): what a data-parallel host does between the reductions and the flags)
        cb = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p)(lambda user, chain: after_reduce(chain))
        t.after_reduce = ctypes.cast(cb, ctypes.c_void_p).value
    by_owners = ctypes.c_int(0)
    ts = ctypes.c_void_p(tail_stream.cuda_stream) if tail_stream is not None else ctypes.c_void_p(0)
    if plane_rows > 0:
        _ck(lib().f2n_field_bwd_step_tail_planes(_stream(), ts, _i(n_max), _p(n_dev, "i32", True), _i(n_off), _i(n_volumes), _p(prim_pool, "i32"),
                                                 _p(local_idx, "i32"), _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"),
                                                 _p(pts_warped, "f32"), _p(volume_idx, "i32"), _i(vol_stride), _p(mlp_params_h, "h16"),
                                                 _p(saved_x_h, "h16", True), _p(x_edge_planes_h, "h16", True), _p(x_cache_h, "h16"),
                                                 _i(plane_rows), _p(src_rows, "i32"), _p(dfeat, "f32"), _f(loss_scale),
                                                 _p(dparams_scaled, "f32"), _p(grad_table_h, "h16"), _i(level_entries), ctypes.byref(t),
                                                 ctypes.byref(by_owners)), "f2n_field_bwd_step_tail_planes")
        return by_owners.value
    if x_cache_h is not None:
        _ck(lib().f2n_field_bwd_step_tail_rows(_stream(), ts, _i(n_max), _p(n_dev, "i32", True), _i(n_off), _i(n_volumes), _p(prim_pool, "i32"),
                                               _p(local_idx, "i32"), _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"),
                                               _p(pts_warped, "f32"), _p(volume_idx, "i32"), _i(vol_stride), _p(mlp_params_h, "h16"),
                                               _p(saved_x_h, "h16", True), _p(x_cache_h, "h16"), _p(src_rows, "i32"), _p(dfeat, "f32"),
                                               _f(loss_scale), _p(dparams_scaled, "f32"), _p(grad_table_h, "h16"), _i(level_entries),
                                               ctypes.byref(t), ctypes.byref(by_owners)), "f2n_field_bwd_step_tail_rows")
        return by_owners.value
    _ck(lib().f2n_field_bwd_step_tail(_stream(), ts, _i(n_max), _p(n_dev, "i32", True), _i(n_off), _i(n_volumes), _p(prim_pool, "i32"),
                                      _p(local_idx, "i32"), _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"),
                                      _p(pts_warped, "f32"), _p(volume_idx, "i32"), _i(vol_stride), _p(mlp_params_h, "h16"),
                                      _p(saved_x_h, "h16"), _p(dfeat, "f32"), _f(loss_scale), _p(dparams_scaled, "f32"),
                                      _p(grad_table_h, "h16"), _i(level_entries), ctypes.byref(t), ctypes.byref(by_owners)),
        "f2n_field_bwd_step_tail")
    return by_owners.value


def reduce_deferred():
    _ck(lib().f2n_reduce_deferred(_stream()), "f2n_reduce_deferred")


def deferred_reset():
    _ck(lib().f2n_deferred_reset(), "f2n_deferred_reset")


def adam_step_h16grad(n, param, grad_h, grad_scale, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, wd, param_h,
                      zero_grad, skip_flag=None):
    _ck(lib().f2n_adam_step_h16grad(_stream(), _i(n), _p(param, "f32"), _p(grad_h, "h16"), _f(grad_scale),
                                    _p(exp_avg, "f32"), _p(exp_avg_sq, "f32"), _i(step), _f(lr), _d(beta1), _d(beta2),
                                    _f(eps), _f(wd), _p(param_h, "h16"), _i(int(zero_grad)),
                                    _p(skip_flag, "i32", True)), "f2n_adam_step_h16grad")


def train_loss(n_rays, pred, gt, disparity, sampled_var, n_edge, feat_dim, edge_feats, var_w, disp_w, tv_w, out_losses,
               dcolors, ddisparity, dvar, dedge_feats):
    _ck(lib().f2n_train_loss(_stream(), _i(n_rays), _p(pred, "f32"), _p(gt, "f32"), _p(disparity, "f32", True),
                             _p(sampled_var, "f32", True), _i(n_edge), _i(feat_dim), _p(edge_feats, "f32", True), _f(var_w),
                             _f(disp_w), _f(tv_w), _p(out_losses, "f32"), _p(dcolors, "f32", True), _p(ddisparity, "f32", True),
                             _p(dvar, "f32", True), _p(dedge_feats, "f32", True)), "f2n_train_loss")


def composite_train(n_rays, se, f0, f0_stride, dt, t, rgb, bg, gt, var_w, disp_w, tv_w, gs_progress, n_edge, feat_dim, edge_feats,
                    dedge_feats, colors, weights, drgb, df0, df0_stride, out_losses, defer_reduce=False):
    """composite_fwd + train_loss + composite_bwd in one launch (include/f2n_abi.h)."""
    _ck(lib().f2n_composite_train(_stream(), _i(n_rays), _p(se, "i32"), _p(f0, "f32"), _i(f0_stride), _p(dt, "f32"), _p(t, "f32"),
                                  _p(rgb, "f32"), _p(bg, "f32"), _p(gt, "f32"), _f(var_w), _f(disp_w), _f(tv_w), _f(gs_progress),
                                  _i(n_edge), _i(feat_dim), _p(edge_feats, "f32", True), _p(dedge_feats, "f32", True),
                                  _p(colors, "f32"), _p(weights, "f32"), _p(drgb, "f32"), _p(df0, "f32"), _i(df0_stride),
                                  _p(out_losses, "f32"), _i(1 if defer_reduce else 0)), "f2n_composite_train")


def nonfinite_flags(n_a, a, n_b, b, flags, mirror=None):
    _ck(lib().f2n_nonfinite_flags_ex(_stream(), _i(n_a), _p(a, "f32", True), _i(n_b), _p(b, "f32", True), _p(flags, "i32"),
                                     _mapped(mirror)), "f2n_nonfinite_flags_ex")


# ---------------------------------------------------------------- world-space queries and meshes
def _lo3(lo):
    return (_f * 3)(*(float(v) for v in lo))


def oct_locate_warp(n, pts_world, tree_nodes, transes, out_pts, out_anchors):
    """World points -> (warped points, anchors (trans_idx, leaf, 0) or (-1, -1, 0)) by octree descent (f2n_oct_locate_warp)."""
    _ck(lib().f2n_oct_locate_warp(_stream(), _i(n), _p(pts_world, "f32"), _p(tree_nodes, "u8"), _p(transes, "u8"), _p(out_pts, "f32"),
                                  _p(out_anchors, "i32")), "f2n_oct_locate_warp")


def oct_locate_warp_grid(lo, step, nx, ny, nz, first_z, n_z, tree_nodes, transes, out_pts, out_anchors):
    """The same for the grid points lo + step * (ix, iy, iz), iz in [first_z, first_z + n_z), x fastest."""
    _ck(lib().f2n_oct_locate_warp_grid(_stream(), _lo3(lo), _f(step), _i(nx), _i(ny), _i(nz), _i(first_z), _i(n_z), _p(tree_nodes, "u8"),
                                       _p(transes, "u8"), _p(out_pts, "f32"), _p(out_anchors, "i32")), "f2n_oct_locate_warp_grid")


def located_compact(n, anchors, pts_warped, counts, start_end, total, out_pts, out_vol, out_src=None):
    _ck(lib().f2n_located_compact(_stream(), _i(n), _p(anchors, "i32"), _p(pts_warped, "f32"), _p(counts, "i32"), _p(start_end, "i32"),
                                  _p(total, "i32"), _p(out_pts, "f32"), _p(out_vol, "i32"), _p(out_src, "i32", True)),
        "f2n_located_compact")


def density_scatter(n, anchors, start_end, f0, density):
    _ck(lib().f2n_density_scatter(_stream(), _i(n), _p(anchors, "i32"), _p(start_end, "i32"), _p(f0, "f32"), _p(density, "f32")),
        "f2n_density_scatter")


def field_density_grad(n, n_volumes, table_h, prim_pool, local_idx, local_size, bias_pool, level_scale, pts_warped, volume_idx, vol_stride,
                       mlp_params_h, x_h, out_dx, out_df0_dw):
    """df0/dx [n,32] (out_dx, optional) and df0/dw [n,3] of the shipped field shape from the pre-pass's h16 features x_h
    (f2n_field_density_grad: all fp32, the same bits on every call)."""
    _ck(lib().f2n_field_density_grad(_stream(), _i(n), _i(n_volumes), _p(table_h, "h16"), _p(prim_pool, "i32"), _p(local_idx, "i32"),
                                     _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"), _p(pts_warped, "f32", n == 0),
                                     _p(volume_idx, "i32", n == 0), _i(vol_stride), _p(mlp_params_h, "h16"), _p(x_h, "h16", n == 0),
                                     _p(out_dx, "f32", True), _p(out_df0_dw, "f32", n == 0)), "f2n_field_density_grad")


def hash_pos_grad(n, n_volumes, table_h, prim_pool, local_idx, local_size, bias_pool, level_scale, pts_warped, volume_idx, vol_stride, dx,
                  out_df0_dw):
    """df0/dw [n,3] from any df0/dx [n,32] f32 (f2n_hash_pos_grad)."""
    _ck(lib().f2n_hash_pos_grad(_stream(), _i(n), _i(n_volumes), _p(table_h, "h16"), _p(prim_pool, "i32"), _p(local_idx, "i32"),
                                _p(local_size, "i32"), _p(bias_pool, "f32"), _p(level_scale, "f32"), _p(pts_warped, "f32", n == 0),
                                _p(volume_idx, "i32", n == 0), _i(vol_stride), _p(dx, "f32", n == 0), _p(out_df0_dw, "f32", n == 0)),
        "f2n_hash_pos_grad")


def density_grad_scatter(n, pts_world, anchors, start_end, transes, f0, df0_dw, out_density, out_grad, out_normal=None):
    """density_scatter with the gradient sigma J^T df0/dw (and optionally the unit normal -grad / |grad|); zeros for the empty points."""
    _ck(lib().f2n_density_grad_scatter(_stream(), _i(n), _p(pts_world, "f32", n == 0), _p(anchors, "i32", n == 0),
                                       _p(start_end, "i32", n == 0), _p(transes, "u8"), _p(f0, "f32", True), _p(df0_dw, "f32", True),
                                       _p(out_density, "f32", n == 0), _p(out_grad, "f32", n == 0), _p(out_normal, "f32", True)),
        "f2n_density_grad_scatter")


def composite_geometry(n_rays, pts_start_end, weights, t, rays_o, rays_d, anchors, transes, df0_dw, tau, out_opacity, out_normal, out_surf_idx,
                       out_surf_t, out_surf_point, out_surf_normal, out_sample_grad=None, out_sample_normal=None):
    """Geometry buffers of rendered rays from f2n_composite_fwd's weights (f2n_composite_geometry): opacity, composited unit normal and
    the first sample whose accumulated weight reaches tau; rays_d are the unit directions the samples' t count along."""
    _ck(lib().f2n_composite_geometry(_stream(), _i(n_rays), _p(pts_start_end, "i32", n_rays == 0), _p(weights, "f32", n_rays == 0),
                                     _p(t, "f32", n_rays == 0), _p(rays_o, "f32", n_rays == 0), _p(rays_d, "f32", n_rays == 0),
                                     _p(anchors, "i32", n_rays == 0), _p(transes, "u8", n_rays == 0), _p(df0_dw, "f32", n_rays == 0), _f(tau),
                                     _p(out_opacity, "f32", n_rays == 0), _p(out_normal, "f32", n_rays == 0), _p(out_surf_idx, "i32", n_rays == 0),
                                     _p(out_surf_t, "f32", n_rays == 0), _p(out_surf_point, "f32", n_rays == 0),
                                     _p(out_surf_normal, "f32", n_rays == 0), _p(out_sample_grad, "f32", True), _p(out_sample_normal, "f32", True)),
        "f2n_composite_geometry")


def mesh_from_grid(grid, level, lo=(0.0, 0.0, 0.0), step=1.0):
    """Marching-tetrahedra iso-surface of a float32 grid [nz, ny, nx] (f2n_mesh_count -> f2n_mesh_emit): (verts [V,3], faces [F,3]).
    Reads back the two totals only (they size the outputs)."""
    nz, ny, nx = (int(v) for v in grid.shape)
    dev = grid.device
    n, c = nx * ny * nz, (nx - 1) * (ny - 1) * (nz - 1)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    vc, vse = torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev)
    fc, fse = torch.empty(c, dtype=torch.int32, device=dev), torch.empty((c, 2), dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    _ck(lib().f2n_mesh_count(_stream(), _i(nx), _i(ny), _i(nz), _p(grid, "f32"), _f(level), _p(mask, "u8"), _p(vc, "i32"), _p(vse, "i32"),
                             _p(fc, "i32"), _p(fse, "i32"), _p(totals, "i32")), "f2n_mesh_count")
    nv, nf = (int(v) for v in totals.cpu())
    verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    if nv or nf:
        _ck(lib().f2n_mesh_emit(_stream(), _i(nx), _i(ny), _i(nz), _p(grid, "f32"), _f(level), _lo3(lo), _f(step), _p(mask, "u8"),
                                _p(vse, "i32"), _p(fse, "i32"), _p(verts, "f32"), _p(faces, "i32")), "f2n_mesh_emit")
    return verts, faces


def radiance_scatter(n, anchors, start_end, f0, rgb_rows, density, rgb):
    """density_scatter with a colour: rows of the compacted (f0, rgb) back to every point, zeros for the empty ones."""
    _ck(lib().f2n_radiance_scatter(_stream(), _i(n), _p(anchors, "i32"), _p(start_end, "i32"), _p(f0, "f32", True),
                                   _p(rgb_rows, "f32", True), _p(density, "f32"), _p(rgb, "f32")), "f2n_radiance_scatter")


def grid_normals(grid, pts, lo=(0.0, 0.0, 0.0), step=1.0):
    """Unit normals [n,3] at pts [n,3] from the gradient of a float32 grid [nz, ny, nx] (f2n_grid_normals)."""
    nz, ny, nx = (int(v) for v in grid.shape)
    n = int(pts.shape[0])
    out = torch.empty((n, 3), dtype=torch.float32, device=grid.device)
    _ck(lib().f2n_grid_normals(_stream(), _i(n), _p(pts, "f32", n == 0), _p(grid, "f32"), _i(nx), _i(ny), _i(nz), _lo3(lo), _f(step),
                               _p(out, "f32", n == 0)), "f2n_grid_normals")
    return out


def mesh_components(faces, n_verts, with_rounds=False):
    """labels [V] int32: the smallest vertex index of every vertex's connected component (f2n_mesh_components; synchronises)."""
    nf = int(faces.shape[0])
    labels = torch.empty(int(n_verts), dtype=torch.int32, device=faces.device)
    changed = torch.zeros(1, dtype=torch.int32, device=faces.device)
    rounds = ctypes.c_int(0)
    _ck(lib().f2n_mesh_components(_stream(), _i(n_verts), _i(nf), _p(faces, "i32", nf == 0), _p(labels, "i32", n_verts == 0),
                                  _p(changed, "i32"), ctypes.byref(rounds)), "f2n_mesh_components")
    return (labels, rounds.value) if with_rounds else labels


def mesh_filter_components(verts, faces, min_faces):
    """The mesh without its components of fewer than min_faces faces, order kept: (verts, faces, vert_src).  min_faces <= 1: the input.
    Reads back the two totals only (they size the outputs)."""
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    dev = verts.device
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    if min_faces <= 1:
        return verts, faces, torch.arange(nv, dtype=torch.int32, device=dev)
    labels = mesh_components(faces, nv)
    comp, vkeep, vse, fkeep, fse, totals = i32(nv), i32(nv), i32(nv, 2), i32(nf), i32(nf, 2), i32(2)
    _ck(lib().f2n_mesh_filter_count(_stream(), _i(nv), _i(nf), _p(faces, "i32", nf == 0), _p(labels, "i32", nv == 0), _i(min_faces),
                                    _p(comp, "i32", nv == 0), _p(vkeep, "i32", nv == 0), _p(vse, "i32", nv == 0), _p(fkeep, "i32", nf == 0),
                                    _p(fse, "i32", nf == 0), _p(totals, "i32")), "f2n_mesh_filter_count")
    kv, kf = (int(v) for v in totals.cpu())
    ov = torch.empty((kv, 3), dtype=torch.float32, device=dev)
    src, of = i32(kv), i32(kf, 3)
    if kv or kf:
        _ck(lib().f2n_mesh_filter_emit(_stream(), _i(nv), _i(nf), _p(verts, "f32"), _p(faces, "i32", nf == 0), _p(vkeep, "i32"),
                                       _p(vse, "i32"), _p(fkeep, "i32", nf == 0), _p(fse, "i32", nf == 0), _p(ov, "f32", kv == 0),
                                       _p(src, "i32", kv == 0), _p(of, "i32", kf == 0)), "f2n_mesh_filter_emit")
    return ov, of, src


def mesh_simplify(verts, faces, cell, lo=None, lam=1e-3):
    """Vertex clustering with quadric-error placement (f2n_mesh_cluster_keys -> sorted unique -> f2n_mesh_cluster_accumulate ->
    f2n_mesh_cluster_place -> f2n_mesh_cluster_faces -> unique rows -> f2n_mesh_filter_count / _emit): (verts, faces, vert_map [V] int32,
    the output vertex of every input vertex or -1).  lo None: the minimum of the finite coordinates.  The sorted uniques are
    torch ops (plumbing); reads back three scalars and the two totals."""
    import numpy as np
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    dev = verts.device
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    f32 = np.float32
    cell = float(f32(cell))
    lo3 = [f32(0.0)] * 3 if lo is None else [f32(x) for x in lo]
    dims = [1, 1, 1]
    if nv > 0 and cell > 0.0 and cell < float("inf"):
        fin = torch.isfinite(verts)  # (per coordinate, over its finite values)
        lows, highs = torch.where(fin, verts, verts.new_full((1,), float("inf"))), torch.where(fin, verts, verts.new_full((1,), float("-inf")))
        box = torch.stack([lows[:, k].min() for k in range(3)] + [highs[:, k].max() for k in range(3)]).cpu().numpy()
        mn, mx = box[:3], box[3:]
        for k in range(3):
            if mn[k] <= mx[k]:  # (the coordinate has a finite value)
                if lo is None:
                    lo3[k] = mn[k]
                with np.errstate(all="ignore"):
                    u = f32(f32(mx[k] - lo3[k]) / f32(cell))  # (two fp32 roundings, as the keys' u)
                if u >= 1048575.0:
                    raise F2nError("cell %g is too small for the extent of the mesh (at most 2^20 cells per axis)" % cell)
                dims[k] = int(np.floor(u)) + 1 if u >= 0 else 1
    lo_c, dims_c = _lo3(lo3), (ctypes.c_int32 * 3)(*dims)
    keys = torch.empty(nv, dtype=torch.int64, device=dev)
    _ck(lib().f2n_mesh_cluster_keys(_stream(), _i(nv), _p(verts, "f32", nv == 0), lo_c, _f(cell), dims_c, _p(keys, "i64", nv == 0)),
        "f2n_mesh_cluster_keys")
    uk, inv = torch.unique(keys, sorted=True, return_inverse=True)
    bad = 1 if len(uk) > 0 and int(uk[0]) < 0 else 0  # key -1 sorts first
    ckeys = uk[bad:].contiguous()
    cluster_of = (inv - bad).to(torch.int32).contiguous()
    nc = int(ckeys.shape[0])
    none_v, none_f = torch.empty((0, 3), dtype=torch.float32, device=dev), i32(0, 3)
    vert_map = torch.full((nv,), -1, dtype=torch.int32, device=dev)
    if nc == 0:
        return none_v, none_f, vert_map
    acc = torch.zeros((nc, 16), dtype=torch.int64, device=dev)
    _ck(lib().f2n_mesh_cluster_accumulate(_stream(), _i(nv), _i(nf), _p(verts, "f32"), _p(faces, "i32", nf == 0), _p(cluster_of, "i32"),
                                          _i(nc), lo_c, _f(cell), dims_c, _p(acc, "i64"), _p(i32(1), "i32")), "f2n_mesh_cluster_accumulate")
    cverts = torch.empty((nc, 3), dtype=torch.float32, device=dev)
    _ck(lib().f2n_mesh_cluster_place(_stream(), _i(nc), _p(acc, "i64"), _p(ckeys, "i64"), lo_c, _f(cell), dims_c, _d(lam),
                                     _p(cverts, "f32")), "f2n_mesh_cluster_place")
    if nf == 0:
        return none_v, none_f, vert_map
    rows = i32(nf, 3)
    _ck(lib().f2n_mesh_cluster_faces(_stream(), _i(nv), _i(nf), _p(faces, "i32"), _p(cluster_of, "i32"), _p(rows, "i32")),
        "f2n_mesh_cluster_faces")
    uf = torch.unique(rows, sorted=True, dim=0)
    if len(uf) > 0 and int(uf[0, 0]) < 0:  # the dropped faces' row sorts first
        uf = uf[1:]
    uf = uf.contiguous()
    kf0 = int(uf.shape[0])
    if kf0 == 0:
        return none_v, none_f, vert_map
    # the clusters no face uses leave, order kept: the component filter with one label and a threshold every face passes
    labels = torch.zeros(nc, dtype=torch.int32, device=dev)
    comp, vkeep, vse, fkeep, fse, totals = i32(nc), i32(nc), i32(nc, 2), i32(kf0), i32(kf0, 2), i32(2)
    _ck(lib().f2n_mesh_filter_count(_stream(), _i(nc), _i(kf0), _p(uf, "i32"), _p(labels, "i32"), _i(1), _p(comp, "i32"), _p(vkeep, "i32"),
                                    _p(vse, "i32"), _p(fkeep, "i32"), _p(fse, "i32"), _p(totals, "i32")), "f2n_mesh_filter_count")
    kv, kf = (int(v) for v in totals.cpu())
    ov, src, of = torch.empty((kv, 3), dtype=torch.float32, device=dev), i32(kv), i32(kf, 3)
    _ck(lib().f2n_mesh_filter_emit(_stream(), _i(nc), _i(kf0), _p(cverts, "f32"), _p(uf, "i32"), _p(vkeep, "i32"), _p(vse, "i32"),
                                   _p(fkeep, "i32"), _p(fse, "i32"), _p(ov, "f32"), _p(src, "i32"), _p(of, "i32")), "f2n_mesh_filter_emit")
    new_of_cluster = torch.where(vkeep != 0, vse[:, 0], torch.full_like(vkeep, -1))
    vert_map = torch.where(cluster_of >= 0, new_of_cluster[cluster_of.clamp_min(0).long()], vert_map).contiguous()
    return ov, of, vert_map


# ---------------------------------------------------------------- mesh refinement
LEVEL_EMPTY, LEVEL_CONVERGED, LEVEL_STEP_CLAMPED, LEVEL_MOVE_CLAMPED = 1, 2, 4, 8  # the status bits of f2n_level_step


def _mesh_ring(faces, n_verts):
    """(ring_start_end, ring, pinned, edge_counts [2] int32 on the device): f2n_mesh_ring_keys -> sort, run lengths (torch ops:
    plumbing) -> f2n_mesh_ring_fill"""
    nv, nf = int(n_verts), int(faces.shape[0])
    if nv < 0:
        raise ValueError("mesh_ring: n_verts must be >= 0")
    dev = faces.device
    ek = uses = torch.empty(0, dtype=torch.int64, device=dev)
    if nf > 0:
        keys = torch.empty((nf, 6), dtype=torch.int64, device=dev)
        _ck(lib().f2n_mesh_ring_keys(_stream(), _i(nv), _i(nf), _p(faces, "i32"), _p(keys, "i64")), "f2n_mesh_ring_keys")
        keys = torch.sort(keys.view(-1)).values
        ek, uses = torch.unique_consecutive(keys[keys >= 0], return_counts=True)
        ek, uses = ek.contiguous(), uses.to(torch.int64).contiguous()
    ne = int(ek.shape[0])
    se = torch.empty((nv, 2), dtype=torch.int32, device=dev)
    ring = torch.empty(ne, dtype=torch.int32, device=dev)
    pinned = torch.empty(nv, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    _ck(lib().f2n_mesh_ring_fill(_stream(), _i(nv), _i(ne), _p(ek, "i64", ne == 0), _p(uses, "i64", ne == 0), _p(se, "i32", nv == 0),
                                 _p(ring, "i32", ne == 0), _p(pinned, "u8", nv == 0), _p(counts, "i32")), "f2n_mesh_ring_fill")
    return se, ring, pinned, counts


def mesh_ring(faces, n_verts):
    """The vertex one-ring of a mesh: (ring_start_end [V,2], ring [E] (neighbours ascending, each once), pinned [V] uint8 (on a boundary or
    non-manifold edge, or used by no face), [boundary_edges, nonmanifold_edges])."""
    se, ring, pinned, counts = _mesh_ring(faces, n_verts)
    return se, ring, pinned, [int(v) for v in counts.cpu()]


def mesh_smooth(verts, faces, passes, lam=0.5, mu=-0.53, max_move=float("inf")):
    """`passes` Taubin lambda|mu pairs of f2n_mesh_smooth over the one-ring, pinned vertices copied through; then f2n_mesh_move_clamp
    against the input for a finite max_move."""
    import math
    if passes < 0:
        raise ValueError("mesh_smooth: passes must be >= 0")
    if not (math.isfinite(lam) and math.isfinite(mu)):
        raise ValueError("mesh_smooth: lam and mu must be finite")
    if not max_move > 0:
        raise ValueError("mesh_smooth: max_move must be > 0 (inf: no clamp)")
    nv = int(verts.shape[0])
    a = verts.clone()
    if nv == 0 or passes == 0:
        return a
    se, ring, pinned, _ = _mesh_ring(faces, nv)
    ne = int(ring.shape[0])
    b = torch.empty_like(a)
    for _ in range(passes):
        for src, dst, factor in ((a, b, lam), (b, a, mu)):
            _ck(lib().f2n_mesh_smooth(_stream(), _i(nv), _i(ne), _p(src, "f32"), _p(se, "i32"), _p(ring, "i32", ne == 0), _p(pinned, "u8"),
                                      _d(factor), _p(dst, "f32")), "f2n_mesh_smooth")
    if math.isfinite(max_move):
        _ck(lib().f2n_mesh_move_clamp(_stream(), _i(nv), _p(verts, "f32"), _f(max_move), _p(a, "f32")), "f2n_mesh_move_clamp")
    return a


def mesh_face_quality(verts, faces):
    """[F] float64: 4 sqrt(3) area / (sum of the squared edge lengths) per face (f2n_mesh_face_quality)."""
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    q = torch.empty(nf, dtype=torch.float64, device=faces.device)
    _ck(lib().f2n_mesh_face_quality(_stream(), _i(nv), _i(nf), _p(verts, "f32", nv == 0), _p(faces, "i32", nf == 0),
                                    ctypes.c_void_p(q.data_ptr()) if nf else ctypes.c_void_p(0)), "f2n_mesh_face_quality")
    return q


def level_step(first, propose, p0, sigma, grad, h, tol, max_step, max_move, cand, best, h_best, g_best, scale, status, evals):
    """f2n_level_step on the caller's arrays; cand, best, h_best, g_best, scale, status and evals are updated in place."""
    n = int(p0.shape[0])
    for t in (grad, cand, best, g_best):
        if tuple(t.shape) != (n, 3):
            raise F2nError("level_step: grad, cand, best and g_best must be [n,3]")
    for t in (sigma, h, h_best, scale, status, evals):
        if tuple(t.shape) != (n,):
            raise F2nError("level_step: sigma, h, h_best, scale, status and evals must be [n]")
    e = n == 0
    _ck(lib().f2n_level_step(_stream(), _i(n), _i(1 if first else 0), _i(1 if propose else 0), _p(p0, "f32", e), _p(sigma, "f32", e),
                             _p(grad, "f32", e), _p(h, "f32", e), _f(tol), _f(max_step), _f(max_move), _p(cand, "f32", e), _p(best, "f32", e),
                             _p(h_best, "f32", e), _p(g_best, "f32", e), _p(scale, "f32", e), _p(status, "i32", e), _p(evals, "i32", e)),
        "f2n_level_step")


# ---------------------------------------------------------------- ray casting against a triangle mesh
RAYCAST_MAX_CELLS = 1 << 27
RAYCAST_DOMAIN_CELLS = 32768.0  # the grid traversal is exact for coordinates up to 2^15 cells (include/f2n_abi.h)


def _finite_box(verts):
    """(min [3], max [3]) per coordinate over its finite values (min > max for a coordinate without one)"""
    fin = torch.isfinite(verts)
    lows, highs = torch.where(fin, verts, verts.new_full((1,), float("inf"))), torch.where(fin, verts, verts.new_full((1,), float("-inf")))
    box = torch.stack([lows[:, k].min() for k in range(3)] + [highs[:, k].max() for k in range(3)]).cpu().numpy()
    return box[:3], box[3:]


def mesh_raycast_default_cell(mn, mx, n_faces):
    """sqrt(10 A / F), A = the area of the vertices' bounding box (about ten faces per occupied cell if the surface had the box's area),
    at least 1/500 of the box's longest side; 1 for an empty or flat box.  A heuristic, not measured on a trained scene."""
    import numpy as np
    e = [float(mx[k]) - float(mn[k]) if mn[k] <= mx[k] else 0.0 for k in range(3)]
    area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0])
    cell = max(np.sqrt(10.0 * area / max(int(n_faces), 1)), max(e) / 500.0)
    c32 = float(np.float32(cell))
    return c32 if c32 > 0.0 and c32 < float("inf") else 1.0


def mesh_raycast_build(verts, faces, cell=None, lo=None):
    """The acceleration grid of mesh_raycast (f2n_mesh_raycast_count -> prefix sum -> f2n_mesh_raycast_fill -> sort -> searchsorted):
    (lo [3], cell, dims [3], cell_start [ncells + 1] int32, cell_faces [E] int32).  cell None: mesh_raycast_default_cell; lo None: the
    minimum of the vertices' finite coordinates (a given lo must not lie above it).  ValueError for a grid that is too fine."""
    import numpy as np
    f32 = np.float32
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    dev = verts.device
    mn, mx = (np.ones(3, f32), np.zeros(3, f32)) if nv == 0 else _finite_box(verts)
    cell = mesh_raycast_default_cell(mn, mx, nf) if cell is None else float(f32(cell))
    if not (cell > 0.0 and cell < float("inf")):
        raise ValueError("mesh_raycast_build: cell must be positive and finite, got %r" % (cell,))
    lo3, dims = [f32(0.0) if lo is None else f32(x) for x in (lo if lo is not None else (0, 0, 0))], [1, 1, 1]
    for k in range(3):
        if not np.isfinite(lo3[k]):
            raise ValueError("mesh_raycast_build: lo must be finite")
        if mn[k] <= mx[k]:
            if lo is None:
                lo3[k] = mn[k]
            if lo3[k] > mn[k]:
                raise ValueError("mesh_raycast_build: the grid must cover the mesh (lo above a vertex)")
            with np.errstate(all="ignore"):
                u = f32(f32(mx[k] - lo3[k]) / f32(cell))
            if not u < 1048575.0:
                raise ValueError("mesh_raycast_build: cell is too small for the extent of the mesh")
            dims[k] = int(np.floor(u)) + 1
    nc = dims[0] * dims[1] * dims[2]
    if nc > RAYCAST_MAX_CELLS:
        raise ValueError("mesh_raycast_build: more than 2^27 cells (cell is too small for the mesh)")
    lo_c, dims_c = _lo3(lo3), (ctypes.c_int32 * 3)(*dims)
    counts = torch.zeros(nf, dtype=torch.int32, device=dev)
    _ck(lib().f2n_mesh_raycast_count(_stream(), _i(nv), _i(nf), _p(verts, "f32", nf == 0), _p(faces, "i32", nf == 0), lo_c, _f(cell), dims_c,
                                     _p(counts, "i32", nf == 0), _p(torch.empty(1, dtype=torch.int32, device=dev), "i32")),
        "f2n_mesh_raycast_count")
    ends = counts.cumsum(0, dtype=torch.int64)
    total = int(ends[-1]) if nf else 0
    if total > 2 ** 31 - 1:
        raise ValueError("mesh_raycast_build: more than 2^31 list entries (cell is too small for the mesh)")
    offsets = (ends - counts).contiguous()
    keys = torch.empty(total, dtype=torch.int64, device=dev)
    if total:
        _ck(lib().f2n_mesh_raycast_fill(_stream(), _i(nv), _i(nf), _p(verts, "f32"), _p(faces, "i32"), lo_c, _f(cell), dims_c,
                                        _p(offsets, "i64"), _p(keys, "i64")), "f2n_mesh_raycast_fill")
    keys = torch.sort(keys)[0]
    m = max(nf, 1)
    cell_start = torch.searchsorted(keys, torch.arange(nc + 1, dtype=torch.int64, device=dev) * m).to(torch.int32).contiguous()
    cell_faces = torch.remainder(keys, m).to(torch.int32).contiguous()
    return [float(x) for x in lo3], cell, dims, cell_start, cell_faces


def mesh_raycast(verts, faces, accel, rays_o, rays_d, bounds=None):
    """(t [R], face [R] int32, bary [R,3]): the rays' first hit on the mesh inside their window (f2n_mesh_raycast); accel =
    mesh_raycast_build's tuple, or None for the brute-force mode.  ValueError for rays outside the grid traversal's domain."""
    nv, nf, R = int(verts.shape[0]), int(faces.shape[0]), int(rays_o.shape[0])
    dev = rays_o.device
    if int(rays_d.shape[0]) != R or (bounds is not None and int(bounds.shape[0]) != R):
        raise F2nError("rays_o [R,3], rays_d [R,3] and bounds [R,2] must agree")
    t = torch.zeros(R, dtype=torch.float32, device=dev)
    face = torch.full((R,), -1, dtype=torch.int32, device=dev)
    bary = torch.zeros((R, 3), dtype=torch.float32, device=dev)
    lo_c = dims_c = None
    cell, cs, cf = 0.0, None, None
    if accel is not None:
        lo, cell, dims, cs, cf = accel
        if cs.numel() != int(dims[0]) * int(dims[1]) * int(dims[2]) + 1:
            raise ValueError("mesh_raycast: cell_start does not match dims")
        far = max(max(abs(float(lo[k])), abs(float(lo[k]) + dims[k] * float(cell))) for k in range(3))
        if R:
            fo = float(rays_o.abs().max())
            far = fo if fo != fo else max(far, fo)  # (an origin that is not finite is outside the domain)
        if not far <= RAYCAST_DOMAIN_CELLS * cell:
            raise ValueError("mesh_raycast: a ray origin (or the grid) lies more than 2^15 cells from the frame's origin: outside the domain "
                             "in which the grid traversal is exact; use a larger cell or accel=None")
        lo_c, dims_c = _lo3(lo), (ctypes.c_int32 * 3)(*(int(x) for x in dims))
    _ck(lib().f2n_mesh_raycast(_stream(), _i(nv), _i(nf), _p(verts, "f32", nf == 0), _p(faces, "i32", nf == 0), lo_c, _f(cell), dims_c,
                               _p(cs, "i32", True), _p(cf if cf is not None and cf.numel() else None, "i32", True), _i(R),
                               _p(rays_o, "f32", R == 0), _p(rays_d, "f32", R == 0), _p(bounds, "f32", True), _p(t, "f32", R == 0),
                               _p(face, "i32", R == 0), _p(bary, "f32", R == 0)), "f2n_mesh_raycast")
    return t, face, bary


# ---------------------------------------------------------------- mesh-to-mesh distance: closest points and surface samples
MESH_SAMPLE_PURPOSE = 0x8CB92BA72F3D8DD7  # host/Renderer.h: kMeshSamplePurpose


def mesh_closest_point(verts, faces, accel, points, max_dist=float("inf")):
    """(dist [N] (+inf: none within max_dist), face [N] int32 (-1: none), bary [N,3]): the points' closest point on the mesh
    (f2n_mesh_closest_point); accel = mesh_raycast_build's tuple, or None for the brute-force mode.  ValueError for a finite point outside
    the grid walk's domain."""
    nv, nf, N = int(verts.shape[0]), int(faces.shape[0]), int(points.shape[0])
    dev = points.device
    if not float(max_dist) >= 0.0:
        raise ValueError("mesh_closest_point: max_dist must be >= 0 (inf: no cut-off)")
    dist = torch.full((N,), float("inf"), dtype=torch.float32, device=dev)
    face = torch.full((N,), -1, dtype=torch.int32, device=dev)
    bary = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    lo_c = dims_c = None
    cell, cs, cf = 0.0, None, None
    if accel is not None:
        lo, cell, dims, cs, cf = accel
        if cs.numel() != int(dims[0]) * int(dims[1]) * int(dims[2]) + 1:
            raise ValueError("mesh_closest_point: cell_start does not match dims")
        far = max(max(abs(float(lo[k])), abs(float(lo[k]) + dims[k] * float(cell))) for k in range(3))
        if N:
            far = max(far, float(torch.where(torch.isfinite(points), points.abs(), points.new_zeros(1)).max()))
        if not far <= RAYCAST_DOMAIN_CELLS * cell:
            raise ValueError("mesh_closest_point: a point (or the grid) lies more than 2^15 cells from the frame's origin: outside the domain "
                             "in which the grid walk is exact; use a larger cell or accel=None")
        lo_c, dims_c = _lo3(lo), (ctypes.c_int32 * 3)(*(int(x) for x in dims))
    _ck(lib().f2n_mesh_closest_point(_stream(), _i(nv), _i(nf), _p(verts, "f32", nf == 0), _p(faces, "i32", nf == 0), lo_c, _f(cell), dims_c,
                                     _p(cs, "i32", True), _p(cf if cf is not None and cf.numel() else None, "i32", True), _i(N),
                                     _p(points, "f32", N == 0), _f(max_dist), _p(dist, "f32", N == 0), _p(face, "i32", N == 0),
                                     _p(bary, "f32", N == 0)), "f2n_mesh_closest_point")
    return dist, face, bary


def mesh_sample_surface(verts, faces, n, seed=0):
    """(points [n,3], face [n] int32, bary [n,3]): n area-uniform, stratified samples of the surface (f2n_mesh_face_weights -> max, prefix
    sum -> f2n_mesh_sample_surface), a pure function of (mesh, n, seed).  ValueError for a mesh without area."""
    nv, nf, n = int(verts.shape[0]), int(faces.shape[0]), int(n)
    dev = verts.device
    if n < 0 or n >= 2 ** 31:
        raise ValueError("mesh_sample_surface: n must lie in [0, 2^31)")
    area2 = torch.zeros(nf, dtype=torch.float64, device=dev)
    weights = torch.zeros(nf, dtype=torch.int64, device=dev)
    if nf:
        _ck(lib().f2n_mesh_face_weights(_stream(), _i(nv), _i(nf), _p(verts, "f32", nv == 0), _p(faces, "i32"), _d(0.0),
                                        ctypes.c_void_p(area2.data_ptr()), ctypes.c_void_p(0)), "f2n_mesh_face_weights")
    largest = float(area2.max()) if nf else 0.0
    if not largest > 0.0:
        raise ValueError("mesh_sample_surface: the mesh has no face with an area")
    _ck(lib().f2n_mesh_face_weights(_stream(), _i(nv), _i(nf), _p(verts, "f32"), _p(faces, "i32"), _d(largest * 2.0 ** -31), ctypes.c_void_p(0),
                                    _p(weights, "i64")), "f2n_mesh_face_weights")
    cum = weights.cumsum(0).contiguous()
    pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    bary = torch.empty((n, 3), dtype=torch.float32, device=dev)
    key = (int(seed) ^ MESH_SAMPLE_PURPOSE) & 0xFFFFFFFFFFFFFFFF
    _ck(lib().f2n_mesh_sample_surface(_stream(), _i(nv), _i(nf), _p(verts, "f32"), _p(faces, "i32"), _p(cum, "i64"), _i(n), ctypes.c_uint64(key),
                                      _p(pts, "f32", n == 0), _p(face, "i32", n == 0), _p(bary, "f32", n == 0)), "f2n_mesh_sample_surface")
    return pts, face, bary


# ---------------------------------------------------------------- texture atlas of a triangle mesh
def mesh_atlas(verts, faces, density, max_size=8192, max_log=7):
    """(uv [F,3,2], size, blocks, density_used): host.mesh_atlas through ctypes (f2n_atlas_classify -> sort and prefix sums ->
    f2n_atlas_place; include/f2n_abi.h states the layout).  blocks: dict of offsets [B+1] int64, block_log [B], block_faces [B,2],
    log_s [F], rot [F], slot [F].  While the atlas is wider than max_size the density is halved, at most 32 times; ValueError for a
    max_size that is no power of two and for a mesh that cannot fit."""
    import numpy as np
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    dev = verts.device
    max_size, max_log = int(max_size), int(max_log)
    density = float(np.float32(density))
    if max_size < 4 or max_size & (max_size - 1):
        raise ValueError("mesh_atlas: max_size must be a power of two, at least 4")
    if not 2 <= max_log <= 13:
        raise ValueError("mesh_atlas: max_log must lie in [2, 13]")
    if not (density > 0.0 and density < float("inf")):
        raise ValueError("mesh_atlas: density must be positive and finite")
    least = 4
    while least * least < 16 * ((nf + 1) // 2):
        least *= 2
    if least > max_size:
        raise ValueError("mesh_atlas: the mesh does not fit max_size even at the smallest block size")
    i64 = dict(dtype=torch.int64, device=dev)
    m, ncls = max(nf, 1), max_log - 1
    log_s, rot = torch.empty(nf, dtype=torch.int32, device=dev), torch.empty(nf, dtype=torch.int32, device=dev)
    for _ in range(33):
        if not density > 0.0:
            break
        _ck(lib().f2n_atlas_classify(_stream(), _i(nv), _i(nf), _p(verts, "f32", True), _p(faces, "i32", nf == 0), _f(density), _i(max_log),
                                     _p(log_s, "i32", nf == 0), _p(rot, "i32", nf == 0)), "f2n_atlas_classify")
        keys = torch.sort((max_log - log_s.to(torch.int64)) * m + torch.arange(nf, **i64))[0]
        order, cls = torch.remainder(keys, m), torch.div(keys, m, rounding_mode="floor")
        n_c = torch.bincount(cls, minlength=ncls)
        nb_c = torch.div(n_c + 1, 2, rounding_mode="floor")
        c0, b0 = n_c.cumsum(0) - n_c, nb_c.cumsum(0) - nb_c
        q = torch.arange(nf, **i64) - c0[cls]
        sl = (b0[cls] + torch.div(q, 2, rounding_mode="floor")) * 2 + torch.remainder(q, 2)
        B = int(nb_c.sum())
        block_log = (max_log - torch.repeat_interleave(torch.arange(ncls, **i64), nb_c)).to(torch.int32).contiguous()
        offsets = torch.cat([torch.zeros(1, **i64), torch.bitwise_left_shift(torch.ones(B, **i64), block_log.to(torch.int64) * 2).cumsum(0)])
        offsets = offsets.contiguous()
        total, size = int(offsets[B]), 4
        while size * size < total:
            size *= 2
        if size > max_size:
            density = float(np.float32(density * 0.5))
            continue
        slot = torch.zeros(nf, dtype=torch.int32, device=dev)
        slot[order] = sl.to(torch.int32)
        block_faces = torch.full((B * 2,), -1, dtype=torch.int32, device=dev)
        block_faces[sl] = order.to(torch.int32)
        uv = torch.zeros((nf, 3, 2), dtype=torch.float32, device=dev)
        _ck(lib().f2n_atlas_place(_stream(), _i(nf), _i(B), _i(size), _p(log_s, "i32", nf == 0), _p(rot, "i32", nf == 0),
                                  _p(slot, "i32", nf == 0), _p(offsets, "i64"), _p(uv, "f32", nf == 0)), "f2n_atlas_place")
        blocks = {"offsets": offsets, "block_log": block_log, "block_faces": block_faces.view(B, 2), "log_s": log_s, "rot": rot, "slot": slot}
        return uv, size, blocks, density
    raise ValueError("mesh_atlas: the mesh does not fit max_size after 32 halvings of the density")


def mesh_atlas_texels(verts, faces, blocks, size, clamp=True):
    """(tex_face [S,S] int32 (-1: unowned), tex_bary [S,S,3], tex_pos [S,S,3]) of mesh_atlas's blocks (f2n_atlas_texels), in row
    bands above 4096^2 texels."""
    nv, nf, S = int(verts.shape[0]), int(faces.shape[0]), int(size)
    dev = verts.device
    B = int(blocks["block_log"].numel())
    if S < 4 or S > 8192 or S & (S - 1):
        raise ValueError("mesh_atlas_texels: size must be a power of two in [4, 8192]")
    if blocks["offsets"].numel() != B + 1 or blocks["block_faces"].numel() != 2 * B or blocks["rot"].numel() != nf:
        raise ValueError("mesh_atlas_texels: blocks do not match (offsets [B+1], block_faces [B,2], rot [F])")
    tex_face = torch.empty((S, S), dtype=torch.int32, device=dev)
    tex_bary, tex_pos = torch.empty((S, S, 3), dtype=torch.float32, device=dev), torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    band = max(16, 4096 * 4096 // S)
    for y in range(0, S, band):
        _ck(lib().f2n_atlas_texels(_stream(), _i(nv), _i(nf), _p(verts, "f32", True), _p(faces, "i32", nf == 0), _i(B), _i(S),
                                   _p(blocks["offsets"], "i64"), _p(blocks["block_log"], "i32", B == 0), _p(blocks["block_faces"], "i32", B == 0),
                                   _p(blocks["rot"], "i32", nf == 0), _i(1 if clamp else 0), _i(y), _i(min(S, y + band)), _p(tex_face, "i32"),
                                   _p(tex_bary, "f32"), _p(tex_pos, "f32")), "f2n_atlas_texels")
    return tex_face, tex_bary, tex_pos


def texture_sample(tex, uv):
    """[N,C]: the bilinear lookup of tex [S,S,C] at uv [N,2] (f2n_texture_sample): texel centres at (i + 0.5) / S, clamped to the edge,
    zeros for a uv that is not finite."""
    if tex.dim() != 3 or tex.shape[0] != tex.shape[1] or not 1 <= int(tex.shape[0]) <= 32768 or not 1 <= int(tex.shape[2]) <= 64:
        raise ValueError("texture_sample: tex must be [S,S,C] with S in [1, 32768] and C in [1, 64]")
    n = int(uv.shape[0])
    out = torch.empty((n, int(tex.shape[2])), dtype=torch.float32, device=tex.device)
    _ck(lib().f2n_texture_sample(_stream(), _i(int(tex.shape[0])), _i(int(tex.shape[2])), _p(tex, "f32"), ctypes.c_int64(n),
                                 _p(uv, "f32", n == 0), _p(out, "f32", n == 0)), "f2n_texture_sample")
    return out


# ---------------------------------------------------------------- SSIM
def ssim_window(filter_size=11, filter_sigma=1.5):
    """The reference's normalised Gaussian window as a list of filter_size floats (f2n_ssim_window; host only)."""
    out = (ctypes.c_double * 33)()
    if lib().f2n_ssim_window(_i(int(filter_size)), _d(float(filter_sigma)), out) != 0:
        raise ValueError("ssim_window: filter_size in [1, 33], filter_sigma > 0 and finite")
    return [float(out[k]) for k in range(int(filter_size))]


def image_ssim(a, b, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """(mean, per_channel [C] float64 on the host, map [H-fs+1,W-fs+1,C] float64 on the device or None): the reference's rgb_ssim
    (scripts/eval.py:29-75) of two float32 [H,W,C] device images (f2n_image_ssim: fp64, fixed tap order, exact integer mean).  A mean is NaN
    if a value under it is not finite.  Reads the statistics back: it synchronises."""
    rules = ("image_ssim: a and b must be float32 [H,W,C] of one shape with C in [1, 4], filter_size in [1, 33] and at most min(H, W), "
             "(H - filter_size + 1) (W - filter_size + 1) <= 2^26, filter_sigma > 0 and finite")
    fs = int(filter_size)
    if a.dim() != 3 or a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(rules)
    H, W, C = (int(v) for v in a.shape)
    if not (1 <= C <= 4 and 1 <= fs <= min(H, W, 33) and 0.0 < float(filter_sigma) < float("inf") and (H - fs + 1) * (W - fs + 1) <= 2 ** 26):
        raise ValueError(rules)
    w = (ctypes.c_double * 33)(*ssim_window(fs, filter_sigma))
    c1, c2 = (float(k1) * float(max_val)) ** 2, (float(k2) * float(max_val)) ** 2
    oh, ow = H - fs + 1, W - fs + 1
    stats = torch.empty((C, 2), dtype=torch.int64, device=a.device)
    m = torch.empty((oh, ow, C), dtype=torch.float64, device=a.device) if return_map else None
    _ck(lib().f2n_image_ssim(_stream(), _i(H), _i(W), _i(C), _p(a, "f32"), _p(b, "f32"), w, _i(fs), _d(c1), _d(c2),
                             ctypes.c_void_p(m.data_ptr()) if return_map else ctypes.c_void_p(0), ctypes.c_void_p(stats.data_ptr())),
        "f2n_image_ssim")
    st = [[int(v) for v in row] for row in stats.cpu().tolist()]
    n = oh * ow
    nan = float("nan")
    per = torch.tensor([float(s) / (2.0 ** 36 * n) if k == n else nan for s, k in st], dtype=torch.float64)
    mean = float(sum(s for s, _ in st)) / (2.0 ** 36 * (n * C)) if all(k == n for _, k in st) else nan
    return mean, per, m


# ---------------------------------------------------------------- TSDF fusion of depth maps
def tsdf_integrate(S, W, lo, step, poses, intri, dist_params, depth, conf, trunc):
    """Adds the depth maps depth [V,h,w] (conf [V,h,w] or None: weight 1) seen from poses [V,3,4] / intri [V,3,3] / dist_params [V,4] into
    the running sums S, W [nz, ny, nx] of the grid lo + step * (ix, iy, iz), in place (f2n_tsdf_integrate)."""
    nz, ny, nx = (int(v) for v in S.shape)
    if tuple(W.shape) != tuple(S.shape):
        raise F2nError("S and W must have the same shape")
    V, h, w = (int(v) for v in depth.shape)
    if poses.numel() != 12 * V or intri.numel() != 9 * V or dist_params.numel() != 4 * V or (conf is not None and conf.shape != depth.shape):
        raise F2nError("poses [V,3,4], intri [V,3,3], dist_params [V,4] and conf must match depth [V,h,w]")
    none = V == 0 or nx * ny * nz == 0
    _ck(lib().f2n_tsdf_integrate(_stream(), _lo3(lo), _f(step), _i(nx), _i(ny), _i(nz), _i(V), _p(poses, "f32", none), _p(intri, "f32", none),
                                 _p(dist_params, "f32", none), _p(depth, "f32", none), _p(conf, "f32", True), _i(h), _i(w), _f(trunc),
                                 _p(S, "f32", none), _p(W, "f32", none)), "f2n_tsdf_integrate")


def tsdf_finalize(S, W, min_weight):
    """(g, valid uint8) of the running sums: valid = (W >= min_weight and W > 0), g = -S / W (positive inside), 0 where not valid."""
    if tuple(W.shape) != tuple(S.shape):
        raise F2nError("S and W must have the same shape")
    n = S.numel()
    g = torch.empty_like(S)
    valid = torch.empty(S.shape, dtype=torch.uint8, device=S.device)
    _ck(lib().f2n_tsdf_finalize(_stream(), ctypes.c_int64(n), _p(S, "f32", n == 0), _p(W, "f32", n == 0), _f(min_weight), _p(g, "f32", n == 0),
                                _p(valid, "u8", n == 0)), "f2n_tsdf_finalize")
    return g, valid


# ---------------------------------------------------------------- view-colour fusion
def view_colors_accumulate(acc, wsum, count, points, normals, poses, intri, dist_params, depth, conf, image, tol, cos_min):
    """Adds what the views (poses [V,3,4] / intri [V,3,3] / dist_params [V,4], depth [V,h,w], conf [V,h,w] or None: 1, image [V,h,w,C])
    observe of points [n,3] (outward normals [n,3] or None) to the running sums acc [n,C], wsum [n], count [n] int32, in place
    (f2n_view_colors_accumulate)."""
    n = int(points.shape[0])
    if acc.dim() != 2 or int(acc.shape[0]) != n or tuple(points.shape) != (n, 3) or wsum.numel() != n or count.numel() != n or (
            normals is not None and normals.shape != points.shape):
        raise F2nError("points [n,3], normals [n,3] or None, acc [n,C], wsum [n] and count [n] must match")
    C = int(acc.shape[1])
    V, h, w = (int(v) for v in depth.shape)
    if (poses.numel() != 12 * V or intri.numel() != 9 * V or dist_params.numel() != 4 * V or (conf is not None and conf.shape != depth.shape) or
            tuple(image.shape) != (V, h, w, C)):
        raise F2nError("poses [V,3,4], intri [V,3,3], dist_params [V,4], conf and image [V,h,w,C] must match depth [V,h,w]")
    none = V == 0 or n == 0
    _ck(lib().f2n_view_colors_accumulate(_stream(), ctypes.c_int64(n), _p(points, "f32", none), _p(normals, "f32", True), _i(V),
                                         _p(poses, "f32", none), _p(intri, "f32", none), _p(dist_params, "f32", none), _p(depth, "f32", none),
                                         _p(conf, "f32", True), _p(image, "f32", none), _i(C), _i(h), _i(w), _f(tol), _f(cos_min),
                                         _p(acc, "f32", none), _p(wsum, "f32", none), _p(count, "i32", none)), "f2n_view_colors_accumulate")


def view_colors_finalize(acc, wsum, count, min_views):
    """(rgb [n,C], known [n] uint8) of the running sums: known = (count >= min_views and wsum > 0), rgb = acc / wsum, 0 where not known."""
    n = int(acc.shape[0])
    if acc.dim() != 2 or wsum.numel() != n or count.numel() != n:
        raise F2nError("acc [n,C], wsum [n] and count [n] must match")
    rgb = torch.empty_like(acc)
    known = torch.empty((n,), dtype=torch.uint8, device=acc.device)
    _ck(lib().f2n_view_colors_finalize(_stream(), ctypes.c_int64(n), _i(int(acc.shape[1])), _p(acc, "f32", n == 0), _p(wsum, "f32", n == 0),
                                       _p(count, "i32", n == 0), _i(int(min_views)), _p(rgb, "f32", n == 0), _p(known, "u8", n == 0)),
        "f2n_view_colors_finalize")
    return rgb, known


def mesh_from_grid_masked(grid, valid, lo=(0.0, 0.0, 0.0), step=1.0, level=0.0):
    """mesh_from_grid over the grid points that carry a value (valid [nz, ny, nx] uint8; f2n_mesh_count_masked -> f2n_mesh_emit): faces
    only from cells whose eight corners are valid, vertices only where a face uses them."""
    nz, ny, nx = (int(v) for v in grid.shape)
    if tuple(valid.shape) != tuple(grid.shape):
        raise F2nError("valid must have the shape of the grid")
    dev = grid.device
    n, c = nx * ny * nz, (nx - 1) * (ny - 1) * (nz - 1)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    vc, vse = torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev)
    fc, fse = torch.empty(c, dtype=torch.int32, device=dev), torch.empty((c, 2), dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    _ck(lib().f2n_mesh_count_masked(_stream(), _i(nx), _i(ny), _i(nz), _p(grid, "f32"), _f(level), _p(valid, "u8"), _p(mask, "u8"),
                                    _p(vc, "i32"), _p(vse, "i32"), _p(fc, "i32"), _p(fse, "i32"), _p(totals, "i32")), "f2n_mesh_count_masked")
    nv, nf = (int(v) for v in totals.cpu())
    verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    if nv or nf:
        _ck(lib().f2n_mesh_emit(_stream(), _i(nx), _i(ny), _i(nz), _p(grid, "f32"), _f(level), _lo3(lo), _f(step), _p(mask, "u8"),
                                _p(vse, "i32"), _p(fse, "i32"), _p(verts, "f32"), _p(faces, "i32")), "f2n_mesh_emit")
    return verts, faces


# ---------------------------------------------------------------- sparse meshing on bricks (include/f2n_abi.h)
def _brick_counts(n, B):
    """(nbx, nby, nbz) of the virtual grid n = (nx, ny, nz); ValueError for what the library refuses (F2N_ERR_INVALID_ARG / _UNSUPPORTED)."""
    if B not in (4, 8, 16):
        raise ValueError("brick size must be 4, 8 or 16, got %r" % (B,))
    if len(n) != 3 or any(int(v) < 2 or int(v) > (1 << 19) for v in n):
        raise ValueError("the grid must have 2 .. 2^19 points per axis")
    nb = tuple((int(v) - 1 + B - 1) // B for v in n)
    if nb[0] * nb[1] * nb[2] > 0x7fffffff:
        raise ValueError("the grid has %d bricks; at most 2^31 - 1 are supported" % (nb[0] * nb[1] * nb[2]))
    return nb


def brick_mark(tree_nodes, lo, step, n, B):
    """flags [nbz, nby, nbx] uint8: 1 for the bricks of B^3 cells of the virtual grid (lo, step, n = (nx, ny, nz)) whose closed box can
    hold a non-empty point of the octree `tree_nodes` (uint8, 64 B per node) -- f2n_brick_mark, a pure function of its arguments."""
    nb = _brick_counts(n, B)
    flags = torch.empty((nb[2], nb[1], nb[0]), dtype=torch.uint8, device=tree_nodes.device)
    _ck(lib().f2n_brick_mark(_stream(), _p(tree_nodes, "u8"), _lo3(lo), _f(step), _i(n[0]), _i(n[1]), _i(n[2]), _i(B), _p(flags, "u8")),
        "f2n_brick_mark")
    return flags


def locate_warp_bricks(brick_ids, lo, step, n, B, tree_nodes, transes):
    """(warped [m,3], anchors [m,3] int32), m = len(brick_ids) (B+1)^3: f2n_oct_locate_warp_grid for the corners of the listed bricks, brick
    major, local x fastest; a corner outside the grid is an empty point (f2n_oct_locate_warp_bricks)."""
    _brick_counts(n, B)
    m = int(brick_ids.numel()) * (B + 1) ** 3
    warped = torch.empty((m, 3), dtype=torch.float32, device=brick_ids.device)
    anchors = torch.empty((m, 3), dtype=torch.int32, device=brick_ids.device)
    _ck(lib().f2n_oct_locate_warp_bricks(_stream(), _lo3(lo), _f(step), _i(n[0]), _i(n[1]), _i(n[2]), _i(B), _i(brick_ids.numel()),
                                         _p(brick_ids, "i32", m == 0), _p(tree_nodes, "u8"), _p(transes, "u8"), _p(warped, "f32", m == 0),
                                         _p(anchors, "i32", m == 0)), "f2n_oct_locate_warp_bricks")
    return warped, anchors


def mesh_from_bricks(values, brick_ids, n, lo, step, level, B, batch_bricks=0):
    """(verts [V,3], faces [F,3] int32) of values [n_bricks, (B+1)^3] float32 for brick_ids [n_bricks] (any order, each id once):
    f2n_brick_mesh_count -> cumsum (int64) -> f2n_brick_mesh_emit per batch of batch_bricks bricks (0: one batch), then the plumbing of the
    host's BrickMeshAssemble: vertices sorted by key, faces = searchsorted(sorted keys, face_vert_keys) sorted by face key -- the bits of
    mesh_from_grid on the dense grid when the list holds every brick with a value on either side of the level.  ValueError: a brick size
    outside {4, 8, 16}, a brick id outside the grid or listed twice, a list that lacks the owner of a face's vertex, more than
    2^31 - 1 vertices or faces."""
    return _mesh_from_bricks(values, None, brick_ids, n, lo, step, level, B, batch_bricks)


def _checked_brick_ids(brick_ids, n, B):
    """brick_ids as int32 [n_bricks], every id inside the grid and listed once (ValueError otherwise)"""
    nb = _brick_counts(n, B)
    total = nb[0] * nb[1] * nb[2]
    ids = brick_ids.to(torch.int64).reshape(-1)
    nbr = int(ids.numel())
    if nbr:
        s = torch.sort(ids)[0]
        if int(s[0]) < 0 or int(s[-1]) >= total:
            raise ValueError("a brick id lies outside the grid's %d bricks" % total)
        if nbr > 1 and bool((s[1:] == s[:-1]).any()):
            raise ValueError("a brick id is listed twice")
    return ids.to(torch.int32).contiguous()


def _mesh_from_bricks(values, valid, brick_ids, n, lo, step, level, B, batch_bricks):
    """valid None: mesh_from_bricks; else mesh_from_bricks_masked"""
    ids = _checked_brick_ids(brick_ids, n, B)
    nbr, P, dev = int(ids.numel()), (B + 1) ** 3, values.device
    if values.numel() != nbr * P or (valid is not None and valid.numel() != nbr * P):
        raise F2nError("values (and valid) must be [n_bricks, (B+1)^3]")
    values = values.reshape(nbr, P)
    masked = valid is not None
    if masked:
        valid = valid.reshape(nbr, P)
    L = lib()
    count = L.f2n_brick_mesh_count_masked if masked else L.f2n_brick_mesh_count
    emit = L.f2n_brick_mesh_emit_masked if masked else L.f2n_brick_mesh_emit
    per = int(batch_bricks) if batch_bricks > 0 else max(nbr, 1)
    i64 = dict(dtype=torch.int64, device=dev)
    vk, vv, fk, fv = [torch.empty(0, **i64)], [torch.empty((0, 3), dtype=torch.float32, device=dev)], [torch.empty(0, **i64)], [torch.empty((0, 3), **i64)]
    for j0 in range(0, nbr, per):
        b, val = ids[j0:j0 + per].contiguous(), values[j0:j0 + per].contiguous()
        c = int(b.numel())
        vc, fc = torch.empty(c, dtype=torch.int32, device=dev), torch.empty(c, dtype=torch.int32, device=dev)
        ok = (_p(valid[j0:j0 + per].contiguous(), "u8"),) if masked else ()  # (the slice of a contiguous [nbr, P] is the memory itself)
        _ck(count(_stream(), _i(n[0]), _i(n[1]), _i(n[2]), _i(B), _i(c), _p(b, "i32"), _p(val, "f32"), *ok, _f(level),
                  _p(vc, "i32"), _p(fc, "i32")), "f2n_brick_mesh_count")
        vend, fend = torch.cumsum(vc, 0, dtype=torch.int64), torch.cumsum(fc, 0, dtype=torch.int64)
        nv, nf = int(vend[-1]), int(fend[-1])
        if nv == 0 and nf == 0:
            continue
        # (a batch may own vertices but no face, or the other way round: the emit wants its four outputs, at least one row each)
        bvk, bvv = torch.empty(max(nv, 1), **i64), torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev)
        bfk, bfv = torch.empty(max(nf, 1), **i64), torch.empty((max(nf, 1), 3), **i64)
        vstart, fstart = (vend - vc).contiguous(), (fend - fc).contiguous()  # (named: they must outlive the call's argument list)
        _ck(emit(_stream(), _i(n[0]), _i(n[1]), _i(n[2]), _i(B), _i(c), _p(b, "i32"), _p(val, "f32"), *ok, _f(level), _lo3(lo),
                 _f(step), _p(vstart, "i64"), _p(fstart, "i64"), _p(bvk, "i64"), _p(bvv, "f32"), _p(bfk, "i64"),
                 _p(bfv, "i64")), "f2n_brick_mesh_emit")
        vk.append(bvk[:nv]), vv.append(bvv[:nv]), fk.append(bfk[:nf]), fv.append(bfv[:nf])
    keys, verts, fkeys, fverts = torch.cat(vk), torch.cat(vv), torch.cat(fk), torch.cat(fv)
    if keys.numel() > 0x7fffffff or fkeys.numel() > 0x7fffffff:
        raise ValueError("the mesh has %d vertices and %d faces; at most 2^31 - 1 of each are supported" % (keys.numel(), fkeys.numel()))
    skeys, perm = torch.sort(keys)
    verts = verts[perm].contiguous()
    if fkeys.numel() == 0:
        return (verts[:0] if masked else verts), torch.empty((0, 3), dtype=torch.int32, device=dev)
    want = fverts.reshape(-1)
    at = torch.searchsorted(skeys, want).clamp_(max=max(int(skeys.numel()) - 1, 0))
    if skeys.numel() == 0 or not bool((skeys[at] == want).all()):
        raise ValueError("the brick list lacks the owner of a face's vertex")
    if masked:  # the vertices some face names, in key order; a face's index = the number of kept vertices in front of it
        used = torch.zeros(skeys.numel(), dtype=torch.int64, device=dev)
        used[at] = 1
        verts = verts[used.bool()].contiguous()
        at = (torch.cumsum(used, 0) - used)[at]
    return verts, at.to(torch.int32).reshape(-1, 3)[torch.argsort(fkeys)].contiguous()


def mesh_from_bricks_masked(values, valid, brick_ids, n, lo, step, level, B, batch_bricks=0):
    """mesh_from_bricks over the corners that carry a value (valid [n_bricks, (B+1)^3] uint8; f2n_brick_mesh_count_masked /
    f2n_brick_mesh_emit_masked), then without the vertices no face names: the bits of mesh_from_grid_masked on the dense grid when the
    list holds the owner of every face."""
    if valid is None:
        raise F2nError("valid is required")
    return _mesh_from_bricks(values, valid, brick_ids, n, lo, step, level, B, batch_bricks)


# ---------------------------------------------------------------- sparse TSDF fusion on bricks (include/f2n_abi.h)
def _tsdf_views(poses, intri, dist_params, depth, conf):
    V, h, w = (int(v) for v in depth.shape)
    if poses.numel() != 12 * V or intri.numel() != 9 * V or dist_params.numel() != 4 * V or (conf is not None and conf.shape != depth.shape):
        raise F2nError("poses [V,3,4], intri [V,3,3], dist_params [V,4] and conf must match depth [V,h,w]")
    none = V == 0
    return (_i(V), _p(poses, "f32", none), _p(intri, "f32", none), _p(dist_params, "f32", none), _p(depth, "f32", none), _p(conf, "f32", True),
            _i(h), _i(w))


def _check_trunc(trunc):
    if not 0.0 < float(trunc) < float("inf"):
        raise ValueError("trunc must be positive and finite, got %r" % (trunc,))


def tsdf_brick_mark(lo, step, n, B, poses, intri, dist_params, depth, conf, trunc):
    """flags [nbz, nby, nbx] uint8: 1 for the bricks of B^3 cells of the virtual grid (lo, step, n = (nx, ny, nz)) whose (B+1)^3 row holds
    an existing corner that some view sees at most trunc behind its surface (f2n_tsdf_brick_mark; all zero without views)."""
    nb = _brick_counts(n, B)
    _check_trunc(trunc)
    flags = torch.zeros((nb[2], nb[1], nb[0]), dtype=torch.uint8, device=depth.device)
    _ck(lib().f2n_tsdf_brick_mark(_stream(), _lo3(lo), _f(step), _i(n[0]), _i(n[1]), _i(n[2]), _i(B),
                                  *_tsdf_views(poses, intri, dist_params, depth, conf), _f(trunc), _p(flags, "u8")), "f2n_tsdf_brick_mark")
    return flags


def tsdf_integrate_bricks(S, W, brick_ids, lo, step, n, B, poses, intri, dist_params, depth, conf, trunc):
    """tsdf_integrate for the rows S, W [n_bricks, (B+1)^3] of brick_ids (each id once, inside the grid), in place
    (f2n_tsdf_integrate_bricks): an existing corner gets the bits of the dense grid point; the others are left untouched."""
    ids = _checked_brick_ids(brick_ids, n, B)
    _check_trunc(trunc)
    m = int(ids.numel()) * (B + 1) ** 3
    if S.numel() != m or W.numel() != m:
        raise F2nError("S and W must be [n_bricks, (B+1)^3]")
    _ck(lib().f2n_tsdf_integrate_bricks(_stream(), _lo3(lo), _f(step), _i(n[0]), _i(n[1]), _i(n[2]), _i(B), _i(ids.numel()),
                                        _p(ids, "i32", m == 0), *_tsdf_views(poses, intri, dist_params, depth, conf), _f(trunc),
                                        _p(S, "f32", m == 0), _p(W, "f32", m == 0)), "f2n_tsdf_integrate_bricks")
