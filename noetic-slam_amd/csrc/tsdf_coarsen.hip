// tsdf_coarsen.hip — a map coarsened 2:1 into a map of twice the voxel size
// (include/tsdf_hip_coarsen.h).  The host (tsdf_capi.cpp) runs, on the destination's
// stream and with both contexts drained:
//   k_coarsen_parents   one lane per source pool slot: the selection (rule 1), the parent's key
//                       into a scratch hash set (64-bit CAS on the key, as k_merge_candidates<true>
//                       does); the lane that wins a key appends it to the parent list
//   k_coarsen_flag      one workgroup per parent brick, one lane per coarse voxel: the eight child
//                       weights, n and validity, whether dst holds the brick, the integer counts
//   (the host reads the counts, and grows dst or refuses)
//   k_merge_insert      the flagged parents into dst's table and pool (tsdf_merge.hip's kernel,
//                       through launch_merge_insert: one definition)
//   k_coarsen_apply     one workgroup per flagged brick: the children's S and W, (s, w) by rule 5,
//                       fused in place in dst's pool by rule 6, each voxel by its own lane
// Flat launches, no workgroup waits for another.  The order of the parent list depends on the CAS
// order, and so does the pool slot a new brick takes; no result does: a coarse voxel is a pure
// function of its eight children, all of one source brick (coarsen_plan.h), and exports are
// ordered by brick coordinate.  The counts are integer atomics.
//
// A lane's children are four aligned 8-byte pairs (a = 0, 1 adjacent in x) per plane, read as
// float2: the four lanes x & 3 = 0..3 of a row read one 32-byte run, and a wave's 64 lanes read
// 16 such runs per pair index.
// The other form that was built -- the child bricks' whole planes copied into LDS as
// 16-byte-per-lane rows (32 KiB in k_coarsen_apply, 16 KiB in k_coarsen_flag) and gathered from
// there -- measured 10 % faster in the flag pass and 14 % slower in the apply pass, the same in sum
// (DESIGN.md §24), and was dropped.
#define COARSEN_FN __host__ __device__ inline
#include "coarsen_plan.h"
#include "tsdf_sample_dev.h"

namespace tsdf {

namespace {

constexpr int CS_PAR_THREADS = 256;
constexpr uint32_t COARSEN_GRID_CAP = 4096;  // workgroups of the per-brick kernels (they stride)

__device__ __forceinline__ int ckey_coord(uint64_t key, int axis) {
    return (int)((key >> (21 * axis)) & 0x1FFFFFull) - BRICK_COORD_BIAS;
}

// ctr[0]: selected source bricks; ctr[1]: distinct parents = list entries (at most n_src)
__global__ __launch_bounds__(CS_PAR_THREADS) void k_coarsen_parents(
    const uint64_t* __restrict__ src_keys, uint32_t n_src, CoarsenSel sel,
    uint64_t* __restrict__ set, uint64_t set_mask, uint64_t* __restrict__ list,
    unsigned long long* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * CS_PAR_THREADS;
    for (uint64_t base = (uint64_t)blockIdx.x * CS_PAR_THREADS; base < n_src; base += stride) {
        const uint64_t i = base + threadIdx.x;  // (uniform trip count: the barrier below)
        bool chosen = false;
        if (i < n_src) {
            const uint64_t sk = src_keys[i];
            const int bx = ckey_coord(sk, 0), by = ckey_coord(sk, 1), bz = ckey_coord(sk, 2);
            chosen = coarsen_selected(sel, bx, by, bz);
            if (chosen) {
                const uint64_t key =
                    pack_brick(coarsen_parent(bx), coarsen_parent(by), coarsen_parent(bz));
                uint64_t h = mix64(key) & set_mask;
                // (the set holds at most half its slots: an EMPTY slot is always met)
                for (uint64_t probe = 0; probe <= set_mask; probe++) {
                    const uint64_t k = set[h];
                    if (k == key) break;
                    if (k == EMPTY_KEY) {
                        const unsigned long long old =
                            atomicCAS((unsigned long long*)&set[h], (unsigned long long)EMPTY_KEY,
                                      (unsigned long long)key);
                        if (old == EMPTY_KEY) {
                            const unsigned long long at = atomicAdd(&ctr[1], 1ull);
                            if (at < n_src) list[at] = key;
                            break;
                        }
                        if (old == key) break;
                    }
                    h = (h + 1) & set_mask;
                }
            }
        }
        const int ns = __syncthreads_count(chosen ? 1 : 0);
        if (threadIdx.x == 0 && ns) atomicAdd(&ctr[0], (unsigned long long)ns);
    }
}

struct CoarsenArgs {
    CoarsenSel sel;
    uint32_t min_children;
    float min_w, max_w;
};

// rule 3
__device__ __forceinline__ bool child_ok(float w, float min_w) { return w > 0.0f && w >= min_w; }

// The pool slot in the source of child brick j of destination brick (dx, dy, dz); a brick the
// source does not hold, or one that is not selected, is INVALID_SLOT (rule 2).
__device__ __forceinline__ uint32_t child_slot(const Table& Ts, const CoarsenSel& sel, int dx,
                                               int dy, int dz, int j) {
    const int bx = 2 * dx + (j & 1), by = 2 * dy + ((j >> 1) & 1), bz = 2 * dz + (j >> 2);
    if (!coarsen_selected(sel, bx, by, bz)) return INVALID_SLOT;
    return brick_slot(Ts, bx, by, bz);
}

// flag[b]: 0 no valid coarse voxel; 1 valid ones, dst holds the brick; 3 valid ones, a new brick.
// Validity comes from the source's weights alone (no distance is read).  Lanes 0..7 look the child
// bricks up and lane 64 dst's brick, and hand the slots to the workgroup through LDS.
// cnt: COARSEN_SHARDS shards of (touched bricks, new bricks, coarse voxels, overlap voxels, child
// voxels), each shard on a 128-byte line of its own and taken by blockIdx, as in k_merge_flag.
__global__ __launch_bounds__(BRICK_VOX) void k_coarsen_flag(
    Table Td, Pool Pd, Table Ts, Pool Ps, CoarsenArgs A, const uint64_t* __restrict__ list,
    uint64_t n, uint32_t* __restrict__ flag, unsigned long long* __restrict__ cnt) {
    const int l = threadIdx.x;
    const int j = coarsen_child_brick(l), base = coarsen_child_base(l);
    __shared__ uint32_t s_slot[9];
    __shared__ uint32_t s_children;
    for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {  // uniform trip count
        const uint64_t key = list[b];
        const int dx = ckey_coord(key, 0), dy = ckey_coord(key, 1), dz = ckey_coord(key, 2);
        if (l < 8) s_slot[l] = child_slot(Ts, A.sel, dx, dy, dz, l);
        if (l == 64) s_slot[8] = brick_slot(Td, dx, dy, dz);
        // (lane 0 alone zeroes and, after the barriers, reads the sum: program order)
        if (l == 0) s_children = 0;
        __syncthreads();
        // (the two counting barriers below separate these reads from the next round's writes)
        const uint32_t cs = s_slot[j], slot = s_slot[8];
        int nc = 0;
        if (cs != INVALID_SLOT) {
            const float* w = Ps.weight + (size_t)cs * BRICK_VOX + base;
#pragma unroll
            for (int q = 0; q < 4; q++) {  // the pair (a = 0, 1) of b + 2 c = q
                const float2 p = *reinterpret_cast<const float2*>(w + coarsen_child_offset(2 * q));
                nc += (child_ok(p.x, A.min_w) ? 1 : 0) + (child_ok(p.y, A.min_w) ? 1 : 0);
            }
        }
        const bool valid = nc >= (int)A.min_children;  // (min_children >= 1: nc = 0 never passes)
        const bool held = slot != INVALID_SLOT;
        const bool over = valid && held && Pd.weight[(size_t)slot * BRICK_VOX + l] > 0.0f;
        int cv = valid ? nc : 0;
#pragma unroll
        for (int o = 32; o; o >>= 1) cv += __shfl_xor(cv, o);
        if ((l & 63) == 0 && cv) atomicAdd(&s_children, (uint32_t)cv);
        const int nv = __syncthreads_count(valid ? 1 : 0);
        const int no = __syncthreads_count(over ? 1 : 0);
        if (l == 0) {
            flag[b] = nv ? (held ? 1u : 3u) : 0u;
            if (nv) {
                unsigned long long* c =
                    cnt + (size_t)(blockIdx.x % COARSEN_SHARDS) * COARSEN_SHARD_WORDS;
                atomicAdd(&c[0], 1ull);
                if (!held) atomicAdd(&c[1], 1ull);
                atomicAdd(&c[2], (unsigned long long)nv);
                if (no) atomicAdd(&c[3], (unsigned long long)no);
                atomicAdd(&c[4], (unsigned long long)s_children);
            }
        }
    }
}

// rules 5 and 6: the children in the order k = a + 2 b + 4 c, then tsdf_import_bricks' merge
// (k_merge_apply's) with (s, w) in the incoming voxel's place
__global__ __launch_bounds__(BRICK_VOX) void k_coarsen_apply(
    Pool Pd, uint32_t dst_bricks, Table Ts, Pool Ps, CoarsenArgs A,
    const uint64_t* __restrict__ list, uint64_t n, const uint32_t* __restrict__ tslot) {
    const int l = threadIdx.x;
    const int j = coarsen_child_brick(l), base = coarsen_child_base(l);
    __shared__ uint32_t s_slot[8];
    for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {
        const uint32_t slot = tslot[b];
        if (slot >= dst_bricks) continue;  // uniform: not flagged (or no room, reported by insert)
        const uint64_t key = list[b];
        if (l < 8)
            s_slot[l] = child_slot(Ts, A.sel, ckey_coord(key, 0), ckey_coord(key, 1),
                                   ckey_coord(key, 2), l);
        __syncthreads();
        const uint32_t cs = s_slot[j];
        __syncthreads();  // (before the next round's writes)
        if (cs == INVALID_SLOT) continue;
        const float* cw = Ps.weight + (size_t)cs * BRICK_VOX + base;
        const float* cd = Ps.sdf + (size_t)cs * BRICK_VOX + base;
        float sw = 0.0f, ssw = 0.0f;
        int nc = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {  // k = 2 q, 2 q + 1
            const int o = coarsen_child_offset(2 * q);
            const float2 pw = *reinterpret_cast<const float2*>(cw + o);
            const float2 pd = *reinterpret_cast<const float2*>(cd + o);
            if (child_ok(pw.x, A.min_w)) {
                ssw = ssw + pd.x * pw.x;
                sw = sw + pw.x;
                nc++;
            }
            if (child_ok(pw.y, A.min_w)) {
                ssw = ssw + pd.y * pw.y;
                sw = sw + pw.y;
                nc++;
            }
        }
        if (nc < (int)A.min_children) continue;
        const float s = ssw / sw, w = sw / (float)nc;
        float* S = Pd.sdf + (size_t)slot * BRICK_VOX + l;
        float* W = Pd.weight + (size_t)slot * BRICK_VOX + l;
        const float w0 = *W;
        if (w0 == 0.0f) {  // unobserved: copy
            *S = s;
            *W = w;
            continue;
        }
        const float nw = w0 + w;
        *S = (*S * w0 + s * w) / nw;
        *W = nw > A.max_w ? A.max_w : nw;
    }
}

uint32_t capped_grid(uint64_t items, uint64_t per_block, uint32_t cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return (uint32_t)(g < 1 ? 1 : (g > cap ? cap : g));
}

CoarsenArgs coarsen_args_of(const CoarsenSel& sel, uint32_t min_children, float min_w,
                            float max_w) {
    CoarsenArgs A;
    A.sel = sel;
    A.min_children = min_children;
    A.min_w = min_w;
    A.max_w = max_w;
    return A;
}

}  // namespace

hipError_t launch_coarsen_parents(const uint64_t* d_src_keys, uint32_t n_src, const CoarsenSel& sel,
                                  uint64_t* d_set, uint64_t set_slots, uint64_t* d_list,
                                  unsigned long long* d_ctr, hipStream_t st) {
    if (!n_src) return hipSuccess;
    k_coarsen_parents<<<capped_grid(n_src, CS_PAR_THREADS, 4096), CS_PAR_THREADS, 0, st>>>(
        d_src_keys, n_src, sel, d_set, set_slots - 1, d_list, d_ctr);
    return hipGetLastError();
}

hipError_t launch_coarsen_flag(const Table& Td, const Pool& Pd, const Table& Ts, const Pool& Ps,
                               const CoarsenSel& sel, uint32_t min_children, float min_w,
                               const uint64_t* d_list, uint64_t n, unsigned long long* d_ctr,
                               uint32_t* d_flag, hipStream_t st) {
    if (!n) return hipSuccess;
    k_coarsen_flag<<<capped_grid(n, 1, COARSEN_GRID_CAP), BRICK_VOX, 0, st>>>(
        Td, Pd, Ts, Ps, coarsen_args_of(sel, min_children, min_w, 0.0f), d_list, n, d_flag,
        d_ctr + COARSEN_CTR_HEAD);
    return hipGetLastError();
}

hipError_t launch_coarsen_apply(const Table& Td, const Pool& Pd, const Table& Ts, const Pool& Ps,
                                const CoarsenSel& sel, uint32_t min_children, float min_w,
                                float max_w, const uint64_t* d_list, uint64_t n,
                                const uint32_t* d_tslot, hipStream_t st) {
    if (!n) return hipSuccess;
    k_coarsen_apply<<<capped_grid(n, 1, COARSEN_GRID_CAP), BRICK_VOX, 0, st>>>(
        Pd, Td.max_bricks, Ts, Ps, coarsen_args_of(sel, min_children, min_w, max_w), d_list, n,
        d_tslot);
    return hipGetLastError();
}

}  // namespace tsdf
