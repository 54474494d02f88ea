// tsdf_merge.hip — one map merged into another under a rigid transform (include/tsdf_hip_merge.h;
// DESIGN.md §15).  The host (tsdf_capi.cpp) runs, on the destination's stream and with both
// contexts drained:
//   k_merge_candidates<false>  one lane per source pool slot: the destination bricks the brick's
//                              image may reach (merge_plan.h), counted -- the size of the set
//   k_merge_candidates<true>   the same bricks' keys into a scratch hash set (64-bit CAS on the
//                              key); the lane that wins a key appends it to the candidate list
//   k_merge_flag<MODE>         one workgroup per candidate brick, one lane per voxel: the sample's
//                              validity, whether dst holds the brick, the integer counts
//   (the host reads the counts, and grows dst or refuses)
//   k_merge_insert             the flagged candidates into dst's table and pool (k_import_insert's
//                              logic on device keys)
//   k_merge_apply<MODE>        one workgroup per flagged brick: sample and fuse in place in dst's
//                              pool, each voxel by its own lane and nobody else
// Flat launches, no workgroup waits for another.  The order of the candidate list depends on the
// CAS order, and so does the pool slot a new brick takes; no result does: every destination voxel
// is a pure function of its own coordinates and the source field, and exports, meshes and halo
// lists are ordered by brick coordinate.  The counts are integer atomics.
//
// The sample comes from tsdf_sample_dev.h, the one definition tsdf_sample.hip and tsdf_raycast.hip
// use: a merged voxel holds exactly what tsdf_sample_device returns at its preimage.
#define MERGE_FN __host__ __device__ inline
#include "merge_plan.h"
#include "tsdf_sample_dev.h"

namespace tsdf {

namespace {

constexpr int MG_CAND_THREADS = 256;
constexpr uint32_t MERGE_GRID_CAP = 8192;  // workgroups of the per-brick kernels (they stride)

__device__ __forceinline__ int mkey_coord(uint64_t key, int axis) {
    return (int)((key >> (21 * axis)) & 0x1FFFFFull) - BRICK_COORD_BIAS;
}

// ctr[0]: candidate pairs (INSERT = false); ctr[1]: distinct candidates = list entries
template <bool INSERT>
__global__ __launch_bounds__(MG_CAND_THREADS) void k_merge_candidates(
    const uint64_t* __restrict__ src_keys, uint32_t n_src, MergeXform X, int mode,
    uint64_t* __restrict__ set, uint64_t set_mask, uint64_t* __restrict__ list, uint64_t list_cap,
    unsigned long long* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * MG_CAND_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * MG_CAND_THREADS + threadIdx.x; i < n_src; i += stride) {
        const uint64_t sk = src_keys[i];
        const int32_t B[3] = {mkey_coord(sk, 0), mkey_coord(sk, 1), mkey_coord(sk, 2)};
        MergeBox bx;
        merge_brick_box(X, B, mode, &bx);
        if (!INSERT) {
            const uint64_t n = merge_box_pairs(bx);
            if (n) atomicAdd(&ctr[0], (unsigned long long)n);
            continue;
        }
        for (int32_t z = bx.lo[2]; z < bx.hi[2]; z++)
            for (int32_t y = bx.lo[1]; y < bx.hi[1]; y++)
                for (int32_t x = bx.lo[0]; x < bx.hi[0]; x++) {
                    if (!merge_reaches(bx, x, y, z)) continue;
                    const uint64_t key = pack_brick(x, y, z);
                    uint64_t h = mix64(key) & set_mask;
                    // (the set holds at most half its slots: an EMPTY slot is always met)
                    for (uint64_t probe = 0; probe <= set_mask; probe++) {
                        const uint64_t k = set[h];
                        if (k == key) break;
                        if (k == EMPTY_KEY) {
                            const unsigned long long old =
                                atomicCAS((unsigned long long*)&set[h],
                                          (unsigned long long)EMPTY_KEY, (unsigned long long)key);
                            if (old == EMPTY_KEY) {
                                const unsigned long long at = atomicAdd(&ctr[1], 1ull);
                                if (at < list_cap) list[at] = key;
                                break;
                            }
                            if (old == key) break;
                        }
                        h = (h + 1) & set_mask;
                    }
                }
    }
}

struct MergeArgs {
    float m[12];  // dst -> src, fp32 (rule 1)
    float vs, inv, bg, min_w, max_w;
};

// The sample of the source field at the preimage of destination voxel (8 D + local) of lane l:
// rules 2 and 3.  Every lane of the workgroup calls it.  VALUES = false: weight and validity alone.
template <int MODE, bool VALUES>
__device__ __forceinline__ Sample merge_sample(const Table& Ts, const Pool& Ps, const MergeArgs& A,
                                               int dx, int dy, int dz, int l) {
    const int vx = 8 * dx + (l & 7), vy = 8 * dy + ((l >> 3) & 7), vz = 8 * dz + (l >> 6);
    const bool live = vx > -VOX_LIMIT && vx < VOX_LIMIT && vy > -VOX_LIMIT && vy < VOX_LIMIT &&
                      vz > -VOX_LIMIT && vz < VOX_LIMIT;
    const float cx = ((float)vx + 0.5f) * A.vs, cy = ((float)vy + 0.5f) * A.vs,
                cz = ((float)vz + 0.5f) * A.vs;
    const float qx = ((A.m[0] * cx + A.m[1] * cy) + A.m[2] * cz) + A.m[3];
    const float qy = ((A.m[4] * cx + A.m[5] * cy) + A.m[6] * cz) + A.m[7];
    const float qz = ((A.m[8] * cx + A.m[9] * cy) + A.m[10] * cz) + A.m[11];
    Sample r = MODE == 0
                   ? sample_nearest<VALUES>(Ts, Ps, A.inv, A.bg, A.min_w, live, qx, qy, qz)
                   : sample_trilinear<VALUES>(Ts, Ps, A.inv, A.bg, A.min_w, live, qx, qy, qz);
    r.valid = r.valid && live;
    return r;
}

// flag[b]: 0 no valid sample; 1 valid samples, dst holds the brick; 3 valid samples, a new brick.
// Validity comes from the source's weights alone (no distance is read).  Lane 0 looks dst's brick
// up and hands the slot to the workgroup through LDS.
// cnt: MERGE_SHARDS shards of (touched bricks, new bricks, merged voxels, overlap voxels), each
// shard on a 128-byte line of its own and taken by blockIdx, so that the workgroups' atomics do
// not queue on four words.  The host adds the shards.
template <int MODE>
__global__ __launch_bounds__(BRICK_VOX) void k_merge_flag(
    Table Td, Pool Pd, Table Ts, Pool Ps, MergeArgs A, const uint64_t* __restrict__ list,
    uint64_t list_cap, const unsigned long long* __restrict__ n_list, uint32_t* __restrict__ flag,
    unsigned long long* __restrict__ cnt) {
    const unsigned long long nl = *n_list;
    const uint64_t n = nl < list_cap ? nl : list_cap;
    const int l = threadIdx.x;
    __shared__ uint32_t s_slot;
    for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {  // uniform trip count
        const uint64_t key = list[b];
        const int dx = mkey_coord(key, 0), dy = mkey_coord(key, 1), dz = mkey_coord(key, 2);
        if (l == 0) s_slot = brick_slot(Td, dx, dy, dz);
        const Sample r = merge_sample<MODE, false>(Ts, Ps, A, dx, dy, dz, l);
        __syncthreads();
        // (the two counting barriers below separate this read from the next round's write)
        const uint32_t slot = s_slot;
        const bool held = slot != INVALID_SLOT;
        const bool over = r.valid && held && Pd.weight[(size_t)slot * BRICK_VOX + l] > 0.0f;
        const int nv = __syncthreads_count(r.valid ? 1 : 0);
        const int no = __syncthreads_count(over ? 1 : 0);
        if (l == 0) {
            flag[b] = nv ? (held ? 1u : 3u) : 0u;
            if (nv) {
                unsigned long long* c = cnt + (size_t)(blockIdx.x % MERGE_SHARDS) * MERGE_SHARD_WORDS;
                atomicAdd(&c[0], 1ull);
                if (!held) atomicAdd(&c[1], 1ull);
                atomicAdd(&c[2], (unsigned long long)nv);
                if (no) atomicAdd(&c[3], (unsigned long long)no);
            }
        }
    }
}

// tslot[b] = the pool slot of flagged candidate b in dst (allocated when new), else INVALID_SLOT
__global__ __launch_bounds__(MG_CAND_THREADS) void k_merge_insert(
    Table Td, const uint64_t* __restrict__ list, uint64_t n, const uint32_t* __restrict__ flag,
    uint32_t* __restrict__ tslot, Globals* G) {
    const uint64_t stride = (uint64_t)gridDim.x * MG_CAND_THREADS;
    for (uint64_t b = (uint64_t)blockIdx.x * MG_CAND_THREADS + threadIdx.x; b < n; b += stride) {
        uint32_t slot = INVALID_SLOT;
        if (flag[b]) {
            const uint64_t key = list[b];
            const int64_t h = table_insert(Td, key, &G->overflow);
            if (h >= 0) {
                slot = Td.slots[h];
                if (slot == UNASSIGNED) {  // the candidates are distinct: one lane per key
                    slot = atomicAdd(&G->pool_count, 1u);
                    if (slot < Td.max_bricks) {
                        Td.brick_keys[slot] = key;
                        Td.slots[h] = slot;
                    } else {
                        Td.slots[h] = INVALID_SLOT;
                        atomicOr(&G->overflow, OVF_POOL);
                        slot = INVALID_SLOT;
                    }
                } else if (slot >= Td.max_bricks) {
                    slot = INVALID_SLOT;
                }
            }
        }
        tslot[b] = slot;
    }
}

// rule 4: tsdf_import_bricks' merge (k_import_merge) with the sample in the incoming voxel's place
template <int MODE>
__global__ __launch_bounds__(BRICK_VOX) void k_merge_apply(
    Pool Pd, uint32_t dst_bricks, Table Ts, Pool Ps, MergeArgs A, const uint64_t* __restrict__ list,
    uint64_t n, const uint32_t* __restrict__ tslot) {
    const int l = threadIdx.x;
    for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {
        const uint32_t slot = tslot[b];
        if (slot >= dst_bricks) continue;  // uniform: not flagged (or no room, reported by insert)
        const uint64_t key = list[b];
        const Sample r = merge_sample<MODE, true>(Ts, Ps, A, mkey_coord(key, 0),
                                                  mkey_coord(key, 1), mkey_coord(key, 2), l);
        if (!r.valid) continue;
        float* S = Pd.sdf + (size_t)slot * BRICK_VOX + l;
        float* W = Pd.weight + (size_t)slot * BRICK_VOX + l;
        const float w0 = *W;
        if (w0 == 0.0f) {  // unobserved: copy
            *S = r.s;
            *W = r.w;
            continue;
        }
        const float nw = w0 + r.w;
        *S = (*S * w0 + r.s * r.w) / nw;
        *W = nw > A.max_w ? A.max_w : nw;
    }
}

uint32_t capped_grid(uint64_t items, uint64_t per_block, uint32_t cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return (uint32_t)(g < 1 ? 1 : (g > cap ? cap : g));
}

MergeArgs merge_args(const RayConst& R, const MergeXform& X, float min_w, float max_w) {
    MergeArgs A;
    for (int k = 0; k < 12; k++) A.m[k] = X.m[k];
    A.vs = R.vs;
    A.inv = R.inv_vs;
    A.bg = R.bg;
    A.min_w = min_w;
    A.max_w = max_w;
    return A;
}

}  // namespace

hipError_t launch_merge_pairs(const uint64_t* d_src_keys, uint32_t n_src, const MergeXform& X,
                              int mode, unsigned long long* d_ctr, hipStream_t st) {
    k_merge_candidates<false><<<capped_grid(n_src, MG_CAND_THREADS, 4096), MG_CAND_THREADS, 0, st>>>(
        d_src_keys, n_src, X, mode, nullptr, 0, nullptr, 0, d_ctr);
    return hipGetLastError();
}

hipError_t launch_merge_candidates(const uint64_t* d_src_keys, uint32_t n_src, const MergeXform& X,
                                   int mode, uint64_t* d_set, uint64_t set_slots, uint64_t* d_list,
                                   uint64_t list_cap, unsigned long long* d_ctr, hipStream_t st) {
    k_merge_candidates<true><<<capped_grid(n_src, MG_CAND_THREADS, 4096), MG_CAND_THREADS, 0, st>>>(
        d_src_keys, n_src, X, mode, d_set, set_slots - 1, d_list, list_cap, d_ctr);
    return hipGetLastError();
}

hipError_t launch_merge_flag(const Table& Td, const Pool& Pd, const Table& Ts, const Pool& Ps,
                             const RayConst& R, const MergeXform& X, int mode, float min_w,
                             const uint64_t* d_list, uint64_t list_cap, unsigned long long* d_ctr,
                             uint32_t* d_flag, hipStream_t st) {
    const MergeArgs A = merge_args(R, X, min_w, 0.0f);
    // (the list's length is known on the device only: a capped grid, the workgroups stride)
    const uint32_t grid = capped_grid(list_cap, 1, MERGE_GRID_CAP);
    if (mode == 0)
        k_merge_flag<0><<<grid, BRICK_VOX, 0, st>>>(Td, Pd, Ts, Ps, A, d_list, list_cap, d_ctr + 1,
                                                    d_flag, d_ctr + MERGE_CTR_HEAD);
    else
        k_merge_flag<1><<<grid, BRICK_VOX, 0, st>>>(Td, Pd, Ts, Ps, A, d_list, list_cap, d_ctr + 1,
                                                    d_flag, d_ctr + MERGE_CTR_HEAD);
    return hipGetLastError();
}

hipError_t launch_merge_insert(const Table& Td, const uint64_t* d_list, uint64_t n,
                               const uint32_t* d_flag, uint32_t* d_tslot, Globals* G,
                               hipStream_t st) {
    if (!n) return hipSuccess;
    k_merge_insert<<<capped_grid(n, MG_CAND_THREADS, 4096), MG_CAND_THREADS, 0, st>>>(
        Td, d_list, n, d_flag, d_tslot, G);
    return hipGetLastError();
}

hipError_t launch_merge_apply(const Table& Td, const Pool& Pd, const Table& Ts, const Pool& Ps,
                              const RayConst& R, const MergeXform& X, int mode, float min_w,
                              float max_w, const uint64_t* d_list, uint64_t n,
                              const uint32_t* d_flag, uint32_t* d_tslot, Globals* G,
                              hipStream_t st) {
    if (!n) return hipSuccess;
    const MergeArgs A = merge_args(R, X, min_w, max_w);
    const hipError_t e = launch_merge_insert(Td, d_list, n, d_flag, d_tslot, G, st);
    if (e != hipSuccess) return e;
    const uint32_t grid = capped_grid(n, 1, MERGE_GRID_CAP);
    if (mode == 0)
        k_merge_apply<0><<<grid, BRICK_VOX, 0, st>>>(Pd, Td.max_bricks, Ts, Ps, A, d_list, n, d_tslot);
    else
        k_merge_apply<1><<<grid, BRICK_VOX, 0, st>>>(Pd, Td.max_bricks, Ts, Ps, A, d_list, n, d_tslot);
    return hipGetLastError();
}

}  // namespace tsdf
