// tsdf_frontier.hip — the frontier voxels of a map box (include/tsdf_hip_frontier.h): the observed
// free voxels with unknown neighbours, as a list ordered by brick and in-brick voxel.
//
// One 512-lane workgroup per listed brick (in (z, y, x) order, given by the host; the host plan is
// frontier_plan.h), striding under FRONTIER_GRID_CAP.  The first 27 lanes look up the brick and its
// 26 neighbours; a 10^3 tile of voxel classes (unknown, free, other), one byte per cell, is staged
// in LDS: lane l loads voxel l of the brick itself (2 KB rows of S and W), the 488 halo cells come
// from the neighbours, and a brick the map does not hold is unknown.  Lane l then counts the
// unknown cells among the first `conn` offsets of the table around its own voxel.
//   k_frontier_count  frontier and free voxels per brick -> host exclusive prefix -> offsets
//   k_frontier_emit   the classes again; a lane's rank is its position in the wave's ballot plus
//                     the counts of the waves before it: coords, n_unknown and dir at
//                     offset[b] + rank
// Ballots, popcounts and integer sums only: no output position depends on arrival order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frontier_plan.h"
#include "tsdf_device.h"
#include "tsdf_ray.h"

namespace tsdf {

__constant__ FrontierOffsets c_foff = FRONTIER_OFFSET;

constexpr int FT = FRONTIER_TILE;
constexpr int FT_CELLS = FT * FT * FT;
constexpr int FT_HALO = FT_CELLS - BRICK_VOX;  // 488
constexpr uint8_t CLS_UNKNOWN = 0, CLS_FREE = 1, CLS_OTHER = 2;
constexpr int F_WAVES = FRONTIER_THREADS / 64;

struct FrontierArgs {
    MeshBox B;
    float free_band, min_weight;
    int conn, min_unknown;
};

// The class of a voxel that reads (S, W); dom: its index lies inside |i| < 2^23.
__device__ __forceinline__ uint8_t frontier_class(float S, float W, bool dom,
                                                  const FrontierArgs& A) {
    const bool obs = dom && W > 0.0f && W >= A.min_weight;
    return !obs ? CLS_UNKNOWN : (S >= A.free_band ? CLS_FREE : CLS_OTHER);
}

// Halo cell h of the 488: the two z faces (100 cells each), then the y faces of z in 0..7 (80
// each), then the x faces of y, z in 0..7 (64 each); in-brick coordinates in -1 .. 8.
__device__ __forceinline__ void frontier_halo_cell(int h, int& cx, int& cy, int& cz) {
    if (h < 200) {
        cz = h < 100 ? -1 : 8;
        const int r = h % 100;
        cx = r % FT - 1;
        cy = r / FT - 1;
    } else if (h < 360) {
        const int k = h - 200;
        cy = k < 80 ? -1 : 8;
        const int r = k % 80;
        cz = r / FT;
        cx = r % FT - 1;
    } else {
        const int k = h - 360;
        cx = k < 64 ? -1 : 8;
        const int r = k % 64;
        cz = r >> 3;
        cy = r & 7;
    }
}

// Stage the class tile of the brick at (bx, by, bz) and evaluate lane l's voxel: returns whether it
// is a frontier voxel; n its unknown neighbours, d their offsets' sum, is_free whether it is a free
// voxel of the box.  Ends with the tile still in use: the caller syncs before the next brick.
__device__ __forceinline__ bool frontier_eval(const Table& T, const Pool& Pl, int bx, int by, int bz,
                                              const FrontierArgs& A, uint8_t* s_cls,
                                              uint32_t* s_slot, bool& is_free, int& n, int d[3]) {
    const int l = threadIdx.x;
    const int lx = l & 7, ly = (l >> 3) & 7, lz = l >> 6;
    const int gx = bx * 8 + lx, gy = by * 8 + ly, gz = bz * 8 + lz;
    const int tc = (lx + 1) + FT * ((ly + 1) + FT * (lz + 1));
    uint8_t own = CLS_UNKNOWN;
    if (l < 27) {  // the brick and its 26 neighbours
        const int nx = bx + l % 3 - 1, ny = by + (l / 3) % 3 - 1, nz = bz + l / 9 - 1;
        uint32_t slot = INVALID_SLOT;
        // (a coordinate outside the key's range has no key: packed, it would carry into the next
        // field and alias another brick)
        if (nx >= -BRICK_COORD_BIAS && nx < BRICK_COORD_BIAS && ny >= -BRICK_COORD_BIAS &&
            ny < BRICK_COORD_BIAS && nz >= -BRICK_COORD_BIAS && nz < BRICK_COORD_BIAS) {
            const int64_t h = table_find(T, pack_brick(nx, ny, nz));
            if (h >= 0) slot = T.slots[h];
        }
        s_slot[l] = slot < T.max_bricks ? slot : INVALID_SLOT;
    }
    __syncthreads();
    {
        const uint32_t slot = s_slot[13];
        if (slot != INVALID_SLOT) {
            const size_t i = (size_t)slot * BRICK_VOX + l;
            own = frontier_class(Pl.sdf[i], Pl.weight[i],
                                 gx > -VOX_LIMIT && gy > -VOX_LIMIT && gz > -VOX_LIMIT, A);
        }
        s_cls[tc] = own;
    }
    if (l < FT_HALO) {
        int cx, cy, cz;
        frontier_halo_cell(l, cx, cy, cz);
        const uint32_t slot =
            s_slot[((cx + 8) >> 3) + 3 * ((cy + 8) >> 3) + 9 * ((cz + 8) >> 3)];
        uint8_t c = CLS_UNKNOWN;
        if (slot != INVALID_SLOT) {
            const size_t i = (size_t)slot * BRICK_VOX + ((cz & 7) << 6) + ((cy & 7) << 3) + (cx & 7);
            c = frontier_class(Pl.sdf[i], Pl.weight[i],
                               bx * 8 + cx > -VOX_LIMIT && by * 8 + cy > -VOX_LIMIT &&
                                   bz * 8 + cz > -VOX_LIMIT, A);
        }
        s_cls[(cx + 1) + FT * ((cy + 1) + FT * (cz + 1))] = c;
    }
    __syncthreads();
    is_free = own == CLS_FREE && gx >= A.B.lo[0] && gx < A.B.hi[0] && gy >= A.B.lo[1] &&
              gy < A.B.hi[1] && gz >= A.B.lo[2] && gz < A.B.hi[2];
    n = 0;
    d[0] = d[1] = d[2] = 0;
    if (is_free) {
        for (int k = 0; k < A.conn; k++) {
            const int ox = c_foff.d[k][0], oy = c_foff.d[k][1], oz = c_foff.d[k][2];
            if (s_cls[tc + ox + FT * (oy + FT * oz)] == CLS_UNKNOWN) {
                n++;
                d[0] += ox;
                d[1] += oy;
                d[2] += oz;
            }
        }
    }
    return is_free && n >= A.min_unknown;
}

__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_count(
    Table T, Pool Pl, const uint64_t* __restrict__ keys, uint32_t nb, FrontierArgs A,
    uint32_t* __restrict__ cnt, uint32_t* __restrict__ fcnt) {
    __shared__ uint8_t s_cls[FT_CELLS];
    __shared__ uint32_t s_slot[27];
    __shared__ uint32_t s_w[2 * F_WAVES];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint64_t key = keys[b];
        const int bx = (int)(key & 0x1FFFFFu) - BRICK_COORD_BIAS;
        const int by = (int)((key >> 21) & 0x1FFFFFu) - BRICK_COORD_BIAS;
        const int bz = (int)((key >> 42) & 0x1FFFFFu) - BRICK_COORD_BIAS;
        bool is_free;
        int n, d[3];
        const bool fr = frontier_eval(T, Pl, bx, by, bz, A, s_cls, s_slot, is_free, n, d);
        const uint32_t nf = (uint32_t)__popcll(__ballot(fr));
        const uint32_t nfree = (uint32_t)__popcll(__ballot(is_free));
        if (lane == 0) {
            s_w[wid] = nf;
            s_w[F_WAVES + wid] = nfree;
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            uint32_t s = 0;
            for (int q = 0; q < F_WAVES; q++) s += s_w[threadIdx.x * F_WAVES + q];
            (threadIdx.x ? fcnt : cnt)[b] = s;
        }
        __syncthreads();  // the tile, the slots and s_w are reused by the next brick
    }
}

__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_emit(
    Table T, Pool Pl, const uint64_t* __restrict__ keys, uint32_t nb, FrontierArgs A,
    const uint32_t* __restrict__ cnt, const uint64_t* __restrict__ off,
    int32_t* __restrict__ coords, uint8_t* __restrict__ n_unknown, int8_t* __restrict__ dir) {
    __shared__ uint8_t s_cls[FT_CELLS];
    __shared__ uint32_t s_slot[27];
    __shared__ uint32_t s_w[F_WAVES];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        if (cnt[b] == 0u) continue;  // (the whole workgroup)
        const uint64_t key = keys[b];
        const int bx = (int)(key & 0x1FFFFFu) - BRICK_COORD_BIAS;
        const int by = (int)((key >> 21) & 0x1FFFFFu) - BRICK_COORD_BIAS;
        const int bz = (int)((key >> 42) & 0x1FFFFFu) - BRICK_COORD_BIAS;
        bool is_free;
        int n, d[3];
        const bool fr = frontier_eval(T, Pl, bx, by, bz, A, s_cls, s_slot, is_free, n, d);
        const uint64_t m = __ballot(fr);
        if (lane == 0) s_w[wid] = (uint32_t)__popcll(m);
        __syncthreads();
        if (fr) {
            uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            for (int q = 0; q < wid; q++) rank += s_w[q];
            // (rank < cnt[b]: the count pass ran the same arithmetic on the same map)
            const uint64_t o = off[b] + rank;
            const int l = threadIdx.x;
            coords[3 * o] = bx * 8 + (l & 7);
            coords[3 * o + 1] = by * 8 + ((l >> 3) & 7);
            coords[3 * o + 2] = bz * 8 + (l >> 6);
            if (n_unknown) n_unknown[o] = (uint8_t)n;
            if (dir) {
                dir[3 * o] = (int8_t)d[0];
                dir[3 * o + 1] = (int8_t)d[1];
                dir[3 * o + 2] = (int8_t)d[2];
            }
        }
        __syncthreads();  // the tile, the slots and s_w are reused by the next brick
    }
}

static FrontierArgs frontier_args(const MeshBox& B, float free_band, float min_weight, int conn,
                                  int min_unknown) {
    FrontierArgs A;
    A.B = B;
    A.free_band = free_band;
    A.min_weight = min_weight;
    A.conn = conn;
    A.min_unknown = min_unknown;
    return A;
}

hipError_t launch_frontier_count(const Table& T, const Pool& Pl, const uint64_t* d_keys, uint32_t nb,
                                 const MeshBox& B, float free_band, float min_weight, int conn,
                                 int min_unknown, uint32_t* d_cnt, uint32_t* d_fcnt,
                                 hipStream_t st) {
    if (nb == 0) return hipSuccess;
    k_frontier_count<<<frontier_grid(nb), FRONTIER_THREADS, 0, st>>>(
        T, Pl, d_keys, nb, frontier_args(B, free_band, min_weight, conn, min_unknown), d_cnt,
        d_fcnt);
    return hipGetLastError();
}

hipError_t launch_frontier_emit(const Table& T, const Pool& Pl, const uint64_t* d_keys, uint32_t nb,
                                const MeshBox& B, float free_band, float min_weight, int conn,
                                int min_unknown, const uint32_t* d_cnt, const uint64_t* d_off,
                                int32_t* d_coords, uint8_t* d_n_unknown, int8_t* d_dir,
                                hipStream_t st) {
    if (nb == 0) return hipSuccess;
    k_frontier_emit<<<frontier_grid(nb), FRONTIER_THREADS, 0, st>>>(
        T, Pl, d_keys, nb, frontier_args(B, free_band, min_weight, conn, min_unknown), d_cnt, d_off,
        d_coords, d_n_unknown, d_dir);
    return hipGetLastError();
}

}  // namespace tsdf
