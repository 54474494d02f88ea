// tsdf_prune.hip — removing bricks from the pool (include/tsdf_hip_prune.h).
//
// The pool is a dense array of bricks [0, pool_count) and the table maps keys to its slots, so
// removing bricks means compacting the pool and rebuilding the table.  The host (tsdf_capi.cpp)
// runs, on the context's stream and with every batch drained:
//   k_rm_flag_box / k_rm_flag_prune   keep[slot] = 1 when the brick stays
//   k_rm_sum, k_rm_scan, k_rm_apply   the prefix of keep over the slots in three flat phases
//                                     (per-block sums, one wave over the sums, per-block
//                                     ranks): new_count, and per slot its rank among the kept or
//                                     the removed.  No workgroup waits for another one.
//   k_rm_gather                       (evict) the removed bricks' voxels, in the caller's order,
//                                     into a bounded scratch piece
//   k_rm_move                         hole filling: the kept bricks at or above new_count (movers)
//                                     into the removed slots below it (holes).  There are equally
//                                     many of each, sources lie in [new_count, old) and
//                                     destinations in [0, new_count): disjoint, so the move is
//                                     race-free in place, which a stable shift would not be.
// and then refills the freed slots with the background and rebuilds the table (k_rehash).
// apply ranks both lists from the same prefix: the removed slots in slot order (rml) begin with the
// holes, because every removed slot below new_count precedes every one above it; and the kept slot
// of kept-rank r >= (kept below new_count) is mover new_count - 1 - r.
#include "tsdf_device.h"
#include "tsdf_ray.h"

namespace tsdf {

namespace {

constexpr int RM_THREADS = 256;
static_assert(RM_THREADS == (int)RM_BLOCK, "one lane per slot of a scan block");
constexpr int RM_WAVES = RM_THREADS / 64;

// brick coordinates of a key (the device twin of brick_key.h's brick_key_coord)
__device__ __forceinline__ int key_coord(uint64_t key, int axis) {
    return (int)((key >> (21 * axis)) & 0x1FFFFFull) - BRICK_COORD_BIAS;
}

struct Box { int lo[3], hi[3]; };

__global__ __launch_bounds__(RM_THREADS) void k_rm_flag_box(const uint64_t* __restrict__ brick_keys,
                                                            uint32_t n, Box B,
                                                            uint32_t* __restrict__ keep) {
    const uint32_t slot = blockIdx.x * RM_THREADS + threadIdx.x;
    if (slot >= n) return;
    const uint64_t key = brick_keys[slot];
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int b = key_coord(key, a);
        in &= b >= B.lo[a] && b < B.hi[a];
    }
    keep[slot] = in ? 1u : 0u;
}

// One wave per brick, lane l the voxels [8 l, 8 l + 8): two 16-B loads of W; a voxel with
// W < min_w goes back to (bg, 0) in both arrays; keep = any W > 0 left in the brick.
__global__ __launch_bounds__(RM_THREADS) void k_rm_flag_prune(Pool Pl, uint32_t n, float min_w,
                                                              float bg,
                                                              uint32_t* __restrict__ keep) {
    const uint32_t b = blockIdx.x * RM_WAVES + (threadIdx.x >> 6);
    if (b >= n) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    float4* W4 = reinterpret_cast<float4*>(Pl.weight + (size_t)b * BRICK_VOX) + 2 * lane;
    float4* S4 = reinterpret_cast<float4*>(Pl.sdf + (size_t)b * BRICK_VOX) + 2 * lane;
    float4 w[2] = {W4[0], W4[1]};
    bool any = false;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const bool r0 = w[q].x < min_w, r1 = w[q].y < min_w, r2 = w[q].z < min_w, r3 = w[q].w < min_w;
        if (r0 | r1 | r2 | r3) {
            float4 s = S4[q];
            if (r0) { s.x = bg; w[q].x = 0.0f; }
            if (r1) { s.y = bg; w[q].y = 0.0f; }
            if (r2) { s.z = bg; w[q].z = 0.0f; }
            if (r3) { s.w = bg; w[q].w = 0.0f; }
            S4[q] = s;
            W4[q] = w[q];
        }
        any |= w[q].x > 0.0f || w[q].y > 0.0f || w[q].z > 0.0f || w[q].w > 0.0f;
    }
    const bool v = __any(any);
    if (lane == 0) keep[b] = v ? 1u : 0u;
}

// The workgroup's kept flags: this lane's exclusive rank among them and their total
__device__ __forceinline__ uint32_t rm_block_rank(bool k, uint32_t* s_w, uint32_t* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned long long m = __ballot(k);
    if (lane == 0) s_w[wid] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < RM_WAVES; q++) {
        const uint32_t r = s_w[q];
        off += q < wid ? r : 0u;
        tot += r;
    }
    *total = tot;
    return off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(RM_THREADS) void k_rm_sum(const uint32_t* __restrict__ keep,
                                                       uint32_t n, uint32_t* __restrict__ bsum) {
    __shared__ uint32_t s_w[RM_WAVES];
    const uint32_t slot = blockIdx.x * RM_THREADS + threadIdx.x;
    uint32_t tot;
    rm_block_rank(slot < n && keep[slot] != 0u, s_w, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// One wave: the exclusive prefix of the nblk block sums, 64 at a time with a carry, so any pool
// size takes the same code (a pool of 2^20 bricks is 64 rounds).  res[0] = new_count (the kept
// bricks), res[1] = 0 (the moves, written by k_rm_apply when something is removed).
__global__ __launch_bounds__(RM_SCAN_THREADS) void k_rm_scan(const uint32_t* __restrict__ bsum,
                                                             uint32_t nblk,
                                                             uint32_t* __restrict__ boff,
                                                             uint32_t* __restrict__ res) {
    static_assert(RM_SCAN_THREADS == 64, "one wave: the round's total is lane 63's prefix");
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblk; base += RM_SCAN_THREADS) {  // uniform trip count
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i < nblk ? bsum[i] : 0u;
        const uint32_t incl = wave_incl_scan(x);
        if (i < nblk) boff[i] = carry + incl - x;
        carry += __shfl(incl, 63, 64);
    }
    if (threadIdx.x == 0) {
        res[0] = carry;
        res[1] = 0u;
    }
}

// Per slot: its rank.  A removed slot of removed-rank q goes to rml[q]; a kept slot at or above
// new_count is mover[new_count - 1 - kept-rank]; the slot new_count itself knows the number of
// removed slots below it, which is the number of holes and of moves.
__global__ __launch_bounds__(RM_THREADS) void k_rm_apply(const uint32_t* __restrict__ keep,
                                                         uint32_t n,
                                                         const uint32_t* __restrict__ boff,
                                                         uint32_t* __restrict__ res,
                                                         uint32_t* __restrict__ rml,
                                                         uint32_t* __restrict__ mover) {
    __shared__ uint32_t s_w[RM_WAVES];
    const uint32_t slot = blockIdx.x * RM_THREADS + threadIdx.x;
    const bool k = slot < n && keep[slot] != 0u;
    uint32_t tot;
    const uint32_t kr = boff[blockIdx.x] + rm_block_rank(k, s_w, &tot);
    if (slot >= n) return;
    const uint32_t new_count = res[0];
    if (slot == new_count) res[1] = slot - kr;
    if (!k)
        rml[slot - kr] = slot;
    else if (slot >= new_count)
        mover[new_count - 1u - kr] = slot;
}

// One wave per listed brick: its 512 voxels of each wanted array to row i of the scratch piece,
// 16 B per lane and access
__global__ __launch_bounds__(RM_THREADS) void k_rm_gather(Pool Pl, const uint32_t* __restrict__ slots,
                                                          uint32_t m, float* __restrict__ out_s,
                                                          float* __restrict__ out_w) {
    const uint32_t i = blockIdx.x * RM_WAVES + (threadIdx.x >> 6);
    if (i >= m) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const size_t src = (size_t)slots[i] * BRICK_VOX, dst = (size_t)i * BRICK_VOX;
    if (out_s) {
        const float4* s = reinterpret_cast<const float4*>(Pl.sdf + src);
        float4* d = reinterpret_cast<float4*>(out_s + dst);
        const float4 a = s[lane], b = s[lane + 64];
        d[lane] = a;
        d[lane + 64] = b;
    }
    if (out_w) {
        const float4* s = reinterpret_cast<const float4*>(Pl.weight + src);
        float4* d = reinterpret_cast<float4*>(out_w + dst);
        const float4 a = s[lane], b = s[lane + 64];
        d[lane] = a;
        d[lane + 64] = b;
    }
}

// One wave per move i: brick mover[i] -> slot hole[i] (sdf, weight and the slot's key)
__global__ __launch_bounds__(RM_THREADS) void k_rm_move(uint64_t* __restrict__ brick_keys, Pool Pl,
                                                        const uint32_t* __restrict__ hole,
                                                        const uint32_t* __restrict__ mover,
                                                        uint32_t n_moves) {
    const uint32_t i = blockIdx.x * RM_WAVES + (threadIdx.x >> 6);
    if (i >= n_moves) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const uint32_t from = mover[i], to = hole[i];
    const size_t src = (size_t)from * BRICK_VOX, dst = (size_t)to * BRICK_VOX;
    const float4* ss = reinterpret_cast<const float4*>(Pl.sdf + src);
    const float4* sw = reinterpret_cast<const float4*>(Pl.weight + src);
    float4* ds = reinterpret_cast<float4*>(Pl.sdf + dst);
    float4* dw = reinterpret_cast<float4*>(Pl.weight + dst);
    const float4 a = ss[lane], b = ss[lane + 64], c = sw[lane], d = sw[lane + 64];
    ds[lane] = a;
    ds[lane + 64] = b;
    dw[lane] = c;
    dw[lane + 64] = d;
    if (lane == 0) brick_keys[to] = brick_keys[from];
}

uint32_t rm_blocks(uint32_t n) { return (n + RM_BLOCK - 1) / RM_BLOCK; }
uint32_t rm_wave_blocks(uint32_t n) { return (n + RM_WAVES - 1) / RM_WAVES; }

}  // namespace

hipError_t launch_rm_flag_box(const Table& T, uint32_t n, const int32_t lo[3], const int32_t hi[3],
                              uint32_t* d_keep, hipStream_t st) {
    if (!n) return hipSuccess;
    Box B;
    for (int a = 0; a < 3; a++) {
        B.lo[a] = lo[a];
        B.hi[a] = hi[a];
    }
    k_rm_flag_box<<<rm_blocks(n), RM_THREADS, 0, st>>>(T.brick_keys, n, B, d_keep);
    return hipGetLastError();
}

hipError_t launch_rm_flag_prune(const Pool& Pl, uint32_t n, float min_w, float bg, uint32_t* d_keep,
                                hipStream_t st) {
    if (!n) return hipSuccess;
    k_rm_flag_prune<<<rm_wave_blocks(n), RM_THREADS, 0, st>>>(Pl, n, min_w, bg, d_keep);
    return hipGetLastError();
}

hipError_t launch_rm_scan(const uint32_t* d_keep, uint32_t n, uint32_t* d_bsum, uint32_t* d_boff,
                          uint32_t* d_res, uint32_t* d_rml, uint32_t* d_mover, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint32_t nblk = rm_blocks(n);
    k_rm_sum<<<nblk, RM_THREADS, 0, st>>>(d_keep, n, d_bsum);
    k_rm_scan<<<1, RM_SCAN_THREADS, 0, st>>>(d_bsum, nblk, d_boff, d_res);
    k_rm_apply<<<nblk, RM_THREADS, 0, st>>>(d_keep, n, d_boff, d_res, d_rml, d_mover);
    return hipGetLastError();
}

hipError_t launch_rm_gather(const Pool& Pl, const uint32_t* d_slots, uint32_t m, float* d_sdf,
                            float* d_w, hipStream_t st) {
    if (!m || (!d_sdf && !d_w)) return hipSuccess;
    k_rm_gather<<<rm_wave_blocks(m), RM_THREADS, 0, st>>>(Pl, d_slots, m, d_sdf, d_w);
    return hipGetLastError();
}

hipError_t launch_rm_move(const Table& T, const Pool& Pl, const uint32_t* d_hole,
                          const uint32_t* d_mover, uint32_t n_moves, hipStream_t st) {
    if (!n_moves) return hipSuccess;
    k_rm_move<<<rm_wave_blocks(n_moves), RM_THREADS, 0, st>>>(T.brick_keys, Pl, d_hole, d_mover,
                                                              n_moves);
    return hipGetLastError();
}

}  // namespace tsdf
